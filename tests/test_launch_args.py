"""_lib.cargs / _lib.ptr: the argument conversion of _lib.launch, on CPU tensors (no GPU; nothing is launched)."""
import ctypes as C

import torch

from spfsplatv2_amd import _lib


def test_tensor_goes_as_its_pointer_and_none_as_null():
    t = torch.arange(6, dtype=torch.float32)[2:]
    p = _lib.ptr(t)
    assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()
    assert _lib.ptr(None) is None                               # (None is ctypes' null pointer)
    got = _lib.cargs((t, None, torch.nn.Parameter(t)))
    assert isinstance(got[0], C.c_void_p) and got[0].value == t.data_ptr()
    assert C.cast(got[1], C.c_void_p).value is None
    assert isinstance(got[2], C.c_void_p) and got[2].value == t.data_ptr()


def test_scalars_and_arrays_pass_through():
    arr = (C.c_float * 3)(1, 2, 3)
    scalar = C.c_int64(7)
    args = (3, True, 0.25, arr, scalar)
    got = _lib.cargs(args)
    assert len(got) == len(args) and all(g is a for g, a in zip(got, args))
    assert type(got[1]) is bool and type(got[2]) is float


def test_structure_goes_by_reference(hip_lib):
    # written through: spf_raster_state_layout fills the structure it is handed
    lay = _lib.SpfStateLayout()
    assert hip_lib.spf_raster_state_layout(*_lib.cargs((64, 100, 2, lay))) == 0
    assert lay.rect_words > 0 and lay.tiles_words > 0 and lay.pair_idx_words > 0
    # read through: a refusal that quotes the fields, raised before anything is launched (float included)
    x = torch.zeros(2 * 3 * 5 * 7)
    a = _lib.SpfSsim(_lib.ptr(x), None, 2, 3, 5, 7, 4, 0.5, 0.5, 1.0, 0, 0)
    rc = hip_lib.spf_ssim_forward(*_lib.cargs((a, x, x, x)), None)
    assert rc == -1 and b"window size must be odd (got N 2 C 3 H 5 W 7 ws 4)" in hip_lib.spf_last_error()
    a.ws = 3                                                    # sizes pass now; the null Y is found next
    rc = hip_lib.spf_ssim_forward(*_lib.cargs((a, x, x, x)), None)
    assert rc == -1 and hip_lib.spf_last_error() == b"ssim: null pointer"


def test_launch_is_here_and_every_launching_entry_point_takes_its_stream_last():
    assert callable(_lib.launch) and callable(_lib.stream_ptr)
    launching = [n for n in _lib.SYMBOLS                       # (spf_last_error reads the message: no arguments at all)
                 if (n.endswith(("forward", "backward", "_step", "_estimate", "_error")) or n.startswith("spf_rope2d"))
                 and n != "spf_last_error"]
    assert len(launching) > 40 and "spf_pose_error" in launching and "spf_optim_step" in launching
    for name in launching:
        assert _lib.SYMBOLS[name][1][-1] is C.c_void_p, name
