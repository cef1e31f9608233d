"""Oracle of the multi-view attention (TEST INFRASTRUCTURE ONLY): the reference's expression, tests/attention_oracle.py,
on keys GATHERED per query view -- what a multi-view backbone feeds ``CrossAttention`` (the other views' tokens copied
into each view's key set, allowed views in ascending order).  The gather is this file's own ``index_select``; autograd
adds the gathered copies' gradients of a key view up, which is what the product's one dk / dv row per key is compared
with.  dtype- and device-generic; the tests run it in float64 on the CPU and in float32 on the device.
"""
from __future__ import annotations

import torch

from tests import attention_oracle as oracle


def allowed(allow, i):
    """Indices of the key views query view ``i`` may read, ascending."""
    return torch.tensor([s for s, on in enumerate(allow[i]) if on], dtype=torch.int64)


def gather_views(x, idx, dim=1):
    """x [b, V, ...] -> the views ``idx`` side by side along the token axis: [b, ..., len(idx) * N, ...] with the token
    axis at ``dim + 1`` of the result's source layout (token-major tensors [b,V,N,C]: dim=1 -> [b, n*N, C])."""
    sel = x.index_select(dim, idx.to(x.device))
    return sel.flatten(dim, dim + 1)


def core_views(q, k, v, qpos, kpos, allow, base=100.0, scale=None, F0=1.0):
    """q [b,Vq,H,Nq,D], k, v [b,Vk,H,Nk,D], qpos [b,Vq,Nq,2], kpos [b,Vk,Nk,2] -> [b,Vq,Nq,H*D]."""
    outs = []
    for i in range(q.shape[1]):
        idx = allowed(allow, i)
        # [b,n,H,Nk,D] -> [b,H,n*Nk,D]
        kg = k.index_select(1, idx.to(k.device)).transpose(1, 2).flatten(2, 3)
        vg = v.index_select(1, idx.to(v.device)).transpose(1, 2).flatten(2, 3)
        kp = gather_views(kpos, idx) if kpos is not None else None
        outs.append(oracle.attention_core(q[:, i], kg, vg, qpos[:, i] if qpos is not None else None, kp, base, scale,
                                          F0))
    return torch.stack(outs, dim=1)


def core_views_with_grads(q, k, v, qpos, kpos, allow, dout, base=100.0, scale=None, dtype=torch.float64, F0=1.0):
    """(out, dq, dk, dv) of core_views in ``dtype`` on the inputs' device; dk, dv: the sums over the gathered copies."""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    out = core_views(q, k, v, qpos, kpos, allow, base, scale, F0)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout.to(dtype), allow_unused=True)
    dk = torch.zeros_like(k) if dk is None else dk
    dv = torch.zeros_like(v) if dv is None else dv
    return out.detach(), dq, dk, dv


def module_views(query, key, qpos, kpos, allow, w: dict, num_heads: int, base=100.0, F0=1.0):
    """``CrossAttention.forward`` per query view on the gathered key views (key = value): query [b,Vq,Nq,C],
    key [b,Vk,Nk,C] -> [b,Vq,Nq,C]."""
    outs = []
    for i in range(query.shape[1]):
        idx = allowed(allow, i)
        mem = gather_views(key, idx)
        outs.append(oracle.cross_attention(query[:, i], mem, mem, qpos[:, i], gather_views(kpos, idx), w, num_heads, base,
                                            F0))
    return torch.stack(outs, dim=1)


def golden_case(case: dict, dtype=torch.float64):
    """Evaluate attention_views_goldens.pt's case with the oracle: (out, {name: gradient}) for the tokens ``x`` and every
    weight; loss 0.5 * sum(out^2).  The case's query / key view ranges and ``allow`` are those of its decoder block."""
    w = {k: v.to(dtype).requires_grad_(True) for k, v in case["weights"].items()}
    x = case["x"].to(dtype).requires_grad_(True)
    (q0, q1), (k0, k1) = case["query_views"], case["key_views"]
    out = module_views(x[:, q0:q1], x[:, k0:k1], case["pos"][:, q0:q1], case["pos"][:, k0:k1], case["allow"].tolist(), w,
                       case["num_heads"], case["base"])
    names = ["x"] + list(w)
    grads = torch.autograd.grad(0.5 * (out * out).sum(), [x] + list(w.values()))
    return out.detach(), dict(zip(names, grads))
