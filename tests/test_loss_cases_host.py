"""Conditions on the perceptual-loss case table (tests/loss_cases.py), from the host restatements alone (tests/loss_ref.py): no
device figure enters.

* Anchor: the explicit float64 restatement equals ``test_loss_grad_host.per_clip_autograd`` (torch.stft) in float64 to 1e-12
  relative on every case, its gradient to 1e-10.
* Tie-free: at every |Xp| - |Xq|, every live Mp - Mq and every pred - target the float64 and float32 library-order restatements
  agree in sign and the float64 gap is at least 16 times their difference; only entries whose gap is exactly 0 in both (the far
  field of the bursts, the pred == target clip) are excused.
* Sensitive: each listed mutation of the restatement moves an asserted statistic of a case to at least 10 times that statistic's
  bound (4 x the measured float32 floor), while the ``rand * 3`` inputs of test_perceptual_loss_per_clip leave at least 15
  filterbank rows below their 2e-4.
* Coverage: the launch regimes the table names are the ones its shapes reach.

``python tests/test_loss_cases_host.py`` prints the sensitivity table of profiles/loss_cases.md.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as C  # noqa: E402
import loss_ref as R  # noqa: E402
from test_loss_grad_host import per_clip_autograd  # noqa: E402


# ---- anchor ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.GRAD_CASES)
def test_explicit_restatement_equals_the_stft_one(name):
    c = C.case(name)
    dev = R.deviations(C.reference(name), R.run(per_clip_autograd, c.pred, c.target, c.W, torch.float64))
    for k, v in dev.items():
        assert float(v.max()) <= (1e-12 if k in R.STATS[:4] else 1e-10), (name, k, float(v.max()))


@pytest.mark.parametrize("elems", C.L1_ELEMS)
def test_l1_kernel_order_is_the_mean(elems):
    a, b = C.l1_inputs(elems)
    ref = R.l1_float64(a, b)
    assert float(((R.l1_kernel_order(a, b).double() - ref).abs() / ref).max()) <= 1e-6


# ---- tie-free --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.GRAD_CASES)
def test_no_sign_hangs_on_rounding(name):
    c = C.case(name)
    g64, g32 = [], []
    with torch.no_grad():
        R.per_clip(c.pred.double(), c.target.double(), gaps=g64)
        R.per_clip(c.pred, c.target, gaps=g32)
    assert len(g64) == 5
    excused = 0
    for what, a, b in zip(("|X| 63", "|X| 32", "|X| 16", "mel", "l1"), g64, g32):
        b = b.double()
        zero = (a == 0) & (b == 0)
        excused += int(zero.sum())
        bad = ~zero & ((torch.sign(a) != torch.sign(b)) | (a.abs() < 16.0 * (a - b).abs()))
        assert not bool(bad.any()), (name, what, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
    if c.bursts is None and not c.identical:
        assert excused == 0, (name, excused)


# ---- sensitive -------------------------------------------------------------------------------------------------------------------
def moved(name, mut, grad=False):
    """Largest (deviation of the mutated float64 restatement from the plain one) / (the statistic's bound) over statistics and
    clips, with the statistic it was seen on."""
    c = C.case(name)
    ref = C.reference(name)
    got = R.run(R.per_clip, c.pred, c.target, c.W if grad else None, torch.float64, mut=mut)
    if not grad:
        ref = (ref[0], None, None)
    bound = C.bounds(name)
    best = max(((float(v.max()) / bound[k], k) for k, v in R.deviations(got, ref).items()))
    return best


def _frames_of(name, term):
    n, hop = (R.SCALES + ((63, 16),))[term]
    return R.n_frames(C.case(name).shape[3], n, hop)


def tb_positions(name):
    """Series positions on both sides of every kind of block boundary of loss_grad_series_kernel in a tb case."""
    B, _, _, T = C.case(name).shape
    tb = C.expected_tb(B, T)
    nblk = (T + tb - 1) // tb
    pos = {0, T - 1}
    if nblk > 1:
        pos |= {tb - 1, tb, (nblk - 1) * tb - 1, (nblk - 1) * tb}
    return sorted(pos)


def mutations():
    """(label, [case names], mut, needs gradient) of every mutation the issue of this table lists."""
    out = []
    for k in R.live_rows():
        out.append((f"filterbank row {k} x 1.01", ["bins"], {"fb_row": (int(k), 1.01)}, False))
    for sc, (n, _) in enumerate(R.SCALES):
        for k in range(n // 2 + 1):
            out.append((f"scale {n} bin {k} x 1.01", ["bins"], {"bin": (sc, k, 1.01)}, False))
    for term in range(4):
        nfr = _frames_of("bins", term)
        for fr in (0, nfr - 1):
            out.append((f"term {term} frame {fr} x 1.01", ["bins"], {"frame": (term, [fr], 1.01)}, False))
    for fr in (255, 256, 257):
        out.append((f"mel frame {fr} x 1.01", ["bursts:6785", "bursts:8209"], {"frame": (R.MEL, [fr], 1.01)}, False))
    for name in ("bursts:6785", "bursts:8209"):
        nfr = _frames_of(name, R.MEL)
        last = list(range(nfr - nfr % C.MEL_FB, nfr))
        out.append((f"{name} last mel block ({len(last)} frames) x 1.01", [name], {"frame": (R.MEL, last, 1.01)}, False))
    out.append(("reflect with edge repeat, left", ["short:32", "bursts:6784"], {"edge_repeat": "left"}, False))
    out.append(("reflect with edge repeat, right", ["short:32", "bursts:6784"], {"edge_repeat": "right"}, False))
    out.append(("reflect padding in the STFT term", ["short:32"], {"stft_reflect": True}, False))
    for name in C.TB:
        T = C.case(name).shape[3]
        for i, pos in enumerate(tb_positions(name)):
            term = (0, R.MEL, 1, 2)[i % 4]
            n, hop = (R.SCALES + ((63, 16),))[term]
            fr = min((pos + n // 2) // hop, R.n_frames(T, n, hop) - 1)      # the last frame that reads the position
            out.append((f"{name} (tb {C.expected_tb(*C.case(name).shape[::3])}): term {term} frame {fr} dropped at position {pos}",
                        [name], {"drop_grad": (term, fr, pos)}, True))
    return out


MUTATIONS = mutations()


@pytest.mark.parametrize("label,names,mut,grad", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_mutation_lands_ten_bounds_out(label, names, mut, grad):
    best = max(moved(name, mut, grad) for name in names)
    assert best[0] >= 10.0, (label, best)


def _old_inputs(b, f, t):
    g = torch.Generator().manual_seed(5)                     # test_gpu_parity.test_perceptual_loss_per_clip
    return torch.rand((b, 1, f, t), generator=g) * 3, torch.rand((b, 1, f, t), generator=g) * 3


def rows_missed_by_the_old_inputs(b, f, t):
    pred, tgt = _old_inputs(b, f, t)
    ref = R.run(R.per_clip, pred, tgt, None, torch.float64)
    missed = 0
    for k in range(32):
        got = R.run(R.per_clip, pred, tgt, None, torch.float64, mut={"fb_row": (k, 1.01)})
        missed += int(float(R.deviations(got, ref)["mel"].max()) < 2e-4)
    return missed


@pytest.mark.parametrize("shape", [(3, 40, 96), (2, 16, 63)])
def test_the_old_inputs_miss_the_filterbank_mutation(shape):
    """The gap this table closes: on rand * 3 inputs a 1 % error in a filterbank row moves the mel column by less than the 2e-4 of
    test_perceptual_loss_per_clip for at least 15 of the 32 rows."""
    assert rows_missed_by_the_old_inputs(*shape) >= 15


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_series_block_regimes():
    shapes = [C.case(n).shape for n in C.TB]
    tbs = [C.expected_tb(s[0], s[3]) for s in shapes]
    assert [C.case(n).info["tb"] for n in C.TB] == tbs == [64, 128, 256, 256]
    assert set(tbs) == {64, 128, 256}
    last = [s[3] - (s[3] - 1) // tb * tb for s, tb in zip(shapes, tbs)]
    assert any(0 < w < 32 and s[3] > tb for w, s, tb in zip(last, shapes, tbs))     # right reflection range spans two blocks
    assert any(s[3] < tb for s, tb in zip(shapes, tbs))
    assert {tb for s, tb, w in zip(shapes, tbs, last) if w < 32 and s[3] > tb} == {64, 128, 256}    # a short last block at each


def test_the_other_regimes():
    assert C.case("clips").shape[0] > 65535                                   # loss_grad_input_kernel: clip += gridDim.y
    assert len(torch.unique(C.case("clips").pred.reshape(65537, -1), dim=0)) == 65537
    assert (C.case("rows:8225").shape[2] + 31) // 32 > 256                    # loss_finish_kernel: s += 256 over the slabs
    for name, blocks in (("bursts:6784", None), ("bursts:6785", [256, 169]), ("bursts:8209", [256, 256, 2])):
        T = C.case(name).shape[3]
        nfr = R.n_frames(T, 63, 16)
        if blocks is None:
            assert T == C.LDS_T
        else:
            assert T > C.LDS_T and [min(C.MEL_FB, nfr - f) for f in range(0, nfr, C.MEL_FB)] == blocks
    assert C.case("align:64").shape[3] % 4 == 0 and C.case("align:63").shape[3] % 4 != 0
    for name in C.GRAD_CASES:
        c = C.case(name)
        assert float(c.pred.min()) < 0 < float(c.pred.max())
        w = c.W
        assert len(torch.unique(w[w != 0])) == int((w != 0).sum()) and bool((w < 0).any()) and int((w == 0).sum()) >= 1
    far = C.far_field(C.case("bursts:6784"))
    assert bool(far.any(dim=1).all())
    for name in C.BURSTS:                                                      # outside the bursts both tensors are exactly zero
        c = C.case(name)
        for b, centre in enumerate(c.bursts):
            lo, hi = C.burst_span(centre, c.shape[3])
            keep = torch.ones(c.shape[3], dtype=torch.bool)
            keep[lo:hi] = False
            assert float(c.pred[b][..., keep].abs().max()) == 0.0 and float(c.target[b][..., keep].abs().max()) == 0.0


def test_far_field_gradient_of_the_reference_is_exactly_zero():
    for name in C.BURSTS:
        c = C.case(name)
        far = C.far_field(c)[:, None, None, :].expand(c.shape)
        _, gp, gq = C.reference(name)
        assert float(gp[far].abs().max()) == 0.0 and float(gq[far].abs().max()) == 0.0
        near = ~C.far_field(c)
        assert bool((gp[:, 0, 0][near] != 0).any())


if __name__ == "__main__":
    print("| mutation | case | statistic | moved, in bounds |\n|---|---|---|---|")
    for label, names, mut, grad in MUTATIONS:
        (ratio, stat), name = max((moved(n, mut, grad), n) for n in names)
        print(f"| {label} | {name} | {stat} | {ratio:.3g} |")
    for shape in ((3, 40, 96), (4, 513, 256), (2, 16, 63)):
        print(f"old inputs {shape}: {rows_missed_by_the_old_inputs(*shape)} of 32 rows below 2e-4")
