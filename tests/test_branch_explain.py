"""The forced-branch comparison (tests/branch_explain.py, util.BranchForcing) on the CPU: the float32 evaluation of the
oracle stands in for the product.

Acceptance: on BASELINE config 2 (seed 5, K = 1 and K = 16) and on a small multi-view case with a non-zero background,
explain -> float64 oracle forced onto the stand-in's branches -> `compare` with only the residual masked passes every
gate of the suite, nothing is unexplained, the residual is inside its cap, and on the two C2 cases at least one pixel is
on the branch the float64 oracle did NOT take (otherwise the forcing path would not be exercised).

The `keep_light` refinement (an undecidable pixel whose candidate rows differ only in entries of weight alpha * T < 1e-4
is compared on the oracle's own branch instead of masked) is accepted the same way, on a fuzz draw with footprints x 250
where 67 of 90 flagged pixels are undecidable.

Rejection: the same harness must fail for three planted defects of the stand-in (C2, K = 1):
  * one flagged pixel's marginal entry composited at HALF its alpha -- neither branch: `unexplained`;
  * the gradients taken with the flagged pixels switched off while the image keeps them (forward and backward
    disagreeing about a marginal contributor): `g_*` / `gel_*` under forcing;
  * ALPHA_MIN = 1/250 in the stand-in: pixels nobody flagged are off.
All three trip the gate on that input; none needed another one.
"""
import pytest
import torch

from oracle import splat_ref
from spfsplatv2_amd import synthetic as syn
from tests import branch_explain, util

C2 = dict(config="C2", n_scenes=1, n_views=1, seed=5)
CASES = {
    "c2_k1": (dict(C2, K=1), (0.0, 0.0, 0.0), True),
    "c2_k16": (dict(C2, K=16), (0.0, 0.0, 0.0), True),
    "test_bg": (dict(config="TEST", n_scenes=2, n_views=2, seed=3, s_mult=8.0, G=1500, K=4, image_hw=(40, 56)),
                (0.1, 0.2, 0.3), False),
}


def _stand_in(batch, ref, bg, si, before_explain=lambda: None):
    forcing = util.BranchForcing(batch, ref, background=bg, scale_invariant=si)
    st = util.run_oracle(batch, torch.float32, background=bg, scale_invariant=si, want_fragile=False,
                         pixel_mask=ref["pixel_mask"],
                         after_forward=lambda res: (before_explain(), forcing.mask_for(res))[1])
    st["radii"] = None            # (integer work is the float64 oracle's own flag business: util.float32_resolvable)
    return forcing, st


def _case(name):
    kw, bg, si = CASES[name]
    batch = syn.make_batch(**kw)
    ref = util.run_oracle(batch, torch.float64, background=bg, scale_invariant=si, mask_fragile=True, decisions=True)
    forcing, st = _stand_in(batch, ref, bg, si)
    return batch, ref, forcing, st, bg, si


@pytest.fixture(scope="module")
def c2_k1():
    return _case("c2_k1")


def _accept(forcing, st, c2_flagged=None):
    rep = forcing.compare(st)
    assert not rep["fails"], rep
    # no pixel inside a window is lost: each is explained, undecidable, has too many entries, or is masked for another reason
    assert rep["unexplained"] == 0, rep
    assert rep["explained"] + rep["undecidable"] + rep["too_many_ambiguous"] + rep["also_other"] == rep["flagged_by_window"], rep
    assert rep["residual"] <= rep["flagged"] - rep["explained"] - rep["undecidable_light"], rep
    if c2_flagged is not None:      # BASELINE config 2: every flag is a window's, every pixel is explained, some on the other branch
        assert rep["flagged"] == rep["flagged_by_window"] == rep["explained"] == c2_flagged, rep
        assert rep["residual"] == 0 and rep["took_other_branch"] >= 1, rep
    return rep


def test_float32_stand_in_passes_every_gate_on_its_own_branches_c2_k1(c2_k1):
    _accept(c2_k1[2], c2_k1[3], c2_flagged=31)


def test_float32_stand_in_passes_every_gate_on_its_own_branches_c2_k16():
    _batch, _ref, forcing, st, *_ = _case("c2_k16")
    _accept(forcing, st, c2_flagged=39)


def test_float32_stand_in_passes_every_gate_with_background_and_views():
    _batch, ref, forcing, st, *_ = _case("test_bg")
    rep = _accept(forcing, st)
    assert rep["flagged"] == int(ref["fragile"].sum())


def test_float32_stand_in_passes_every_gate_with_light_undecidable_pixels_unmasked():
    batch, bg, si, _desc = util.random_fuzz_case(112)
    ref = util.run_oracle(batch, torch.float64, background=bg, scale_invariant=si, mask_fragile=True, decisions=True)
    forcing = util.BranchForcing(batch, ref, keep_light=True, background=bg, scale_invariant=si)
    st = util.run_oracle(batch, torch.float32, background=bg, scale_invariant=si, want_fragile=False,
                         pixel_mask=ref["pixel_mask"], after_forward=forcing.mask_for)
    st["radii"] = None
    rep = _accept(forcing, st)
    assert rep["undecidable_light"] >= 10 and rep["residual"] < rep["undecidable"], rep


def test_forced_keep_of_the_oracles_own_rows_changes_nothing(c2_k1):
    """`force_keep` with the recorded keep masks is the unforced evaluation bit for bit (and `explain` only replaces
    rows)."""
    batch, ref = c2_k1[0], c2_k1[1]
    own = [{t: rec["keep"] for t, rec in ref["decisions"][0]["tiles"].items()}]
    again = util.run_oracle(batch, torch.float64, mask_fragile=True, force_keep=own)
    assert torch.equal(again["color"], ref["color"]) and torch.equal(again["alpha"], ref["alpha"])
    for n in util.GRAD_NAMES:
        assert torch.equal(again["grads"][n], ref["grads"][n]), n


def test_rejects_a_marginal_entry_composited_at_half_its_alpha(c2_k1):
    batch, ref, _forcing, st, bg, si = c2_k1
    dec = ref["decisions"][0]
    h, w = batch.image_shape
    # the flagged pixel whose threshold entry weighs most (a 1/510 layer under transmittance T moves alpha by T / 510:
    # T > 0.06 puts it more than 1e-4 from BOTH branches)
    best = None
    for (tx, ty), rec in dec["tiles"].items():
        for r, row in enumerate(rec["rows"].tolist()):
            x, y = tx * 16 + row % 16, ty * 16 + row // 16
            for e in torch.nonzero(rec["near_alpha"][r] & rec["keep"][row]).flatten().tolist():
                keep = rec["keep"][row]
                _c, _a, wts = branch_explain.composite_row(rec["alpha"][r].double(), keep, rec["rgb"].double(),
                                                           torch.tensor(bg, dtype=torch.float64))
                if x < w and y < h and (best is None or float(wts[e]) > best[0]):
                    best = (float(wts[e]), x, y, rec, r, row, e)
    assert best is not None and best[0] > 2.5e-4, best
    _wt, x, y, rec, r, row, e = best
    scale = torch.ones_like(rec["alpha"][r].double())
    scale[e] = 0.5
    c, a, _ = branch_explain.composite_row(rec["alpha"][r].double(), rec["keep"][row], rec["rgb"].double(),
                                           torch.tensor(bg, dtype=torch.float64), scale)
    bad = dict(st, color=st["color"].clone(), alpha=st["alpha"].clone())
    bad["color"][0, 0, :, y, x] = c.float()
    bad["alpha"][0, 0, 0, y, x] = float(a)
    forcing = util.BranchForcing(batch, ref, background=bg, scale_invariant=si)
    bad["forced_mask"] = forcing.mask_for(bad)
    assert forcing.counters["unexplained"] == 1 and forcing.unexplained[0][2:4] == (x, y), forcing.unexplained
    rep = forcing.compare(bad)
    assert "unexplained" in rep["fails"], rep


def test_rejects_gradients_that_drop_the_flagged_pixels_the_image_keeps(c2_k1):
    _batch, _ref, forcing, st, *_ = c2_k1
    bad = dict(st, grads_forced=st["grads"])          # the backward of the loss WITHOUT the knife-edge pixels
    rep = forcing.compare(bad)
    print(rep)
    assert any(f.startswith(("g_", "gel_")) for f in rep["fails"]), rep
    assert "unexplained" not in rep["fails"] and "rgb_max" not in rep["fails"], rep     # (the image itself is fine)


def test_rejects_another_alpha_threshold(c2_k1, monkeypatch):
    batch, ref, _forcing, _st, bg, si = c2_k1
    monkeypatch.setattr(splat_ref, "ALPHA_MIN", 1.0 / 250.0)
    forcing, st = _stand_in(batch, ref, bg, si, before_explain=monkeypatch.undo)    # (the defect is the stand-in's alone)
    assert splat_ref.ALPHA_MIN == 1.0 / 255.0
    rep = forcing.compare(st)
    print(rep)
    assert {"rgb_max", "alpha_max"} & set(rep["fails"]), rep           # pixels that nobody flagged are off
