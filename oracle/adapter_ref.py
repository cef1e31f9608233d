"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference's Gaussian adapter.

Follows UnifiedGaussianAdapter.forward (src/model/encoder/common/gaussian_adapter.py:122-150 of the reference):

    scales    = clamp_max(0.001 * softplus(raw[..., 0:3]), 0.3)
    rotations = q / (|q| + eps),  q = raw[..., 3:7]
    harmonics = raw[..., 7:].view(..., 3, K) * sh_mask

in plain torch, dtype-generic: float64 is the arbiter of the HIP kernels, float32 is "what a correct float32
implementation achieves" (the yardstick the kernels' tolerances are derived from).  Gradients are autograd's.  Pinned to
the reference's own class by tests/golden/adapter_goldens.pt (tests/test_adapter_oracle.py).  Only tests/ may import
this module; the product never does.
"""
import torch
import torch.nn.functional as F


def sh_mask(sh_degree: int, dtype=torch.float32) -> torch.Tensor:
    """gaussian_adapter.py:41-48: band l >= 1 is scaled by 0.1 * 0.25 ** l (built in float32 like the reference's
    buffer, then cast: the arbiter sees the very mask values the kernels multiply by)."""
    mask = torch.ones(((sh_degree + 1) ** 2,), dtype=torch.float32)
    for degree in range(1, sh_degree + 1):
        mask[degree ** 2:(degree + 1) ** 2] = 0.1 * 0.25 ** degree
    return mask.to(dtype)


def adapter_forward(raw: torch.Tensor, mask: torch.Tensor, eps: float = 1e-8):
    """raw [..., 7 + 3K], mask [K] (K = 0: the geometric channels alone) -> scales [..., 3], rotations [..., 4],
    harmonics [..., 3, K], in raw's dtype."""
    K = mask.numel()
    if raw.shape[-1] != 7 + 3 * K:
        raise ValueError(f"raw has {raw.shape[-1]} channels, the mask asks for {7 + 3 * K}")
    scales = (0.001 * F.softplus(raw[..., :3])).clamp_max(0.3)
    q = raw[..., 3:7]
    rotations = q / (q.norm(dim=-1, keepdim=True) + eps)
    harmonics = raw[..., 7:].reshape(*raw.shape[:-1], 3, K) * mask
    return scales, rotations, harmonics


def adapter_reference(raw: torch.Tensor, mask: torch.Tensor, eps: float = 1e-8, g_scales=None, g_rotations=None,
                      g_harmonics=None, dtype=torch.float64, chunk_rows: int = 1 << 16) -> dict:
    """Outputs and dL/draw of the adapter over rows `raw` [N, 7 + 3K], evaluated in `dtype` on the CPU in chunks of
    `chunk_rows` rows (2 M rows x 82 channels in float64 never exist at once: only the results do).  The upstream
    gradients ([N, 3], [N, 4], [N, 3, K]; None = zero) may be of any dtype; without any, `raw_grad` is None."""
    raw = raw.detach().cpu()
    if raw.dim() != 2:
        raise ValueError("adapter_reference takes rows [N, 7 + 3K]")
    N, K = raw.shape[0], mask.numel()
    m = mask.detach().cpu().to(dtype)
    ups = (g_scales, g_rotations, g_harmonics)
    want_grad = any(g is not None for g in ups)
    out = {"scales": torch.empty((N, 3), dtype=dtype), "rotations": torch.empty((N, 4), dtype=dtype),
           "harmonics": torch.empty((N, 3, K), dtype=dtype),
           "raw_grad": torch.empty((N, 7 + 3 * K), dtype=dtype) if want_grad else None}
    for a in range(0, N, chunk_rows):
        b = min(N, a + chunk_rows)
        r = raw[a:b].to(dtype).requires_grad_(want_grad)
        res = adapter_forward(r, m, eps)
        for name, t in zip(("scales", "rotations", "harmonics"), res):
            out[name][a:b] = t.detach()
        if want_grad:
            pairs = [(t, g[a:b].detach().cpu().to(dtype).reshape(t.shape)) for t, g in zip(res, ups) if g is not None]
            (gr,) = torch.autograd.grad([t for t, _ in pairs], r, [g for _, g in pairs])
            out["raw_grad"][a:b] = gr
    return out
