"""The per-bin bound of tests/solver_bounds.py on the host (no GPU): what tests/test_gpu_dereverb.py, test_gpu_dereverb_mc.py and
test_gpu_beamform.py hold the device to, applied to the restatements themselves.

* Both float32 restatements (pairwise and sequential sums over t) of every parity, tilted and power-of-two case pass the bound; by
  construction they sit at a quarter of it or less.  Each case prints the ratio of the two orders' floors.
* The power-of-two scale per bin, 2^-((5 b) mod 13), goes through the float32 restatements bit for bit, and no non-zero
  component's square leaves the normal range: the argument the device pins rest on is checked, not assumed.
* The bound catches what the clip-wide one (4 FLOOR max |d64|) misses.  The float32 sequential restatement of a tilted case stands in
  for the device and is mutated: (a) its quietest bin returned as the input row, (b) 1e-3 of its own scale added to the last bin,
  (c) two adjacent bins of the quietest quarter swapped, (d) for MVDR the mask column of one frame taken from the next frame in one
  bin.  Every mutation passes the clip-wide assertion and exceeds the per-bin bound by 10 x or more.  (b) is 1e-3 against a
  bound of 4 floors, so it separates by 10 x only where the floor is under 2.5e-5: that holds for MVDR at the defaults (floor 6e-6), for
  WPE at one tap and one iteration (5e-7) and for joint WPE at two channels, one tap and one iteration (1.2e-5), which is where
  (b) is held to 10 x; at the defaults of WPE and joint WPE (floors 4e-5 and 1.1e-4 to 1.6e-4: the Cholesky solve of 20 to 32
  unknowns) it is still caught, by 6 x and by 1.6 x to 2.3 x, which is asserted as "fails the bound".
* The slips the layouts of tests/variant_cover.py could make, on one variant case per operator (untilted, T 97, group / clip 0
  recomputed with the slip in the float32 sequential restatement); each lands outside the bound, by the printed multiple:
    wpe_mc (5, 6), the last channel's column of P dropped (G's last column zero):            E 4.6,    7800 x
    wpe_mc (5, 6), a repeated last channel kept (bin b's column C is bin b + 1's column 0):  E 4.5e6,  7.6e9 x
    wpe K 29, the last tap of the partial eighth block row dropped (the filter of 28 taps):  E 0.30,   1600 x
    mvdr C 7, Phi_n[6, 6] (the last triangle entry) misses the last frame's term:            E 0.086,  3100 x at both reference channels
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_ref as bf  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_ref as mr  # noqa: E402
import dereverb_ref as dr  # noqa: E402
import solver_bounds as sb  # noqa: E402

HOST_CASES = tuple(sb.host_cases())
T = sb.TILTED_FRAMES
SEPARATION = 10.0
ONE_TAP = dict(taps=1, delay=1, iterations=1)


def test_the_statistic_itself():
    ref = np.zeros((2, 3, 4), np.complex128)
    ref[0, :, 0], ref[0, 1, 1], ref[1, 2, 3] = (1.0, -2.0, 0.5), 1e-4j, 3.0
    got = ref.copy()
    assert np.array_equal(sb.per_bin(got, ref), np.zeros((2, 4)))
    got[0, 0, 0] += 0.5                                                             # 0.5 of the bin's own 2.0
    got[0, 2, 1] += 1e-5                                                            # a tenth of a quiet bin
    e = sb.per_bin(got, ref)
    assert e[0, 0] == 0.25 and abs(e[0, 1] - 0.1) < 1e-12 and sb.worst(got, ref) == (0.25, 0, 0)
    got[1, 0, 2] = 1e-30                                                            # a dead bin must be exactly zero
    assert sb.per_bin(got, ref)[1, 2] == np.inf
    got[1, 0, 2], got[1, 1, 3] = 0.0, np.nan
    assert sb.per_bin(got, ref)[1, 3] == np.inf
    spec = sb.wpe_spec(64, 5)
    assert sb.wpe_bounds(spec) is sb.wpe_bounds(spec.copy())                        # cached on the bits of the input


@pytest.mark.parametrize("label,case", HOST_CASES, ids=[label for label, _ in HOST_CASES])
def test_both_float32_restatements_pass_the_per_bin_bound(label, case):
    b = case()
    assert b.floor >= sb.EPS and b.floor >= max(b.floors.values())
    for order in sb.ORDERS:
        for _, got, ref in b.views(order):
            e, r, col = sb.worst(got, ref)
            assert e <= b.floor <= sb.MARGIN * b.floor / 4.0, (order, e, r, col)
    ratio = b.floors["sequential"] / b.floors["pairwise"] if b.floors["pairwise"] > 0 else float("nan")
    print(f"{label}: floor pairwise {b.floors['pairwise']:.3g} sequential {b.floors['sequential']:.3g}, sequential / pairwise {ratio:.2f}")


# ---- the power-of-two scale goes through the float32 restatements bit for bit -------------------------------------------------------
def _times(z, factor):
    """complex64 / float32 (..., F) times an exact float32 factor per bin, each component on its own."""
    f = factor.astype(np.float32)
    if not np.iscomplexobj(z):
        return z * f
    out = np.empty_like(z)
    out.real, out.imag = z.real * f, z.imag * f
    return out


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _mag_of(d):
    return np.sqrt(dr._power(d, np.float32))


def _pow2_pairs():
    f = sb.pow2(33)
    spec = sb.wpe_spec(64, T)
    yield "wpe", sb.wpe_bounds(spec), sb.wpe_bounds(sb.scale_spec(spec, f)), (sb.scale_spec(spec, f),)
    for ck in sb.TILTED_MC:
        spec = sb.mc_spec(64, T, ck[0])
        yield (f"wpe_mc {ck}", sb.wpe_mc_bounds(spec, ck[0], mc.params_of(ck)),
               sb.wpe_mc_bounds(sb.scale_spec(spec, f), ck[0], mc.params_of(ck)), (sb.scale_spec(spec, f),))
    for channels in sb.TILTED_MVDR:
        spec, mags = sb.mvdr_inputs(64, T, channels)
        s_spec, s_mags = sb.scale_spec(spec, f), sb.scale_mags(mags, f)
        yield (f"mvdr C {channels}", sb.mvdr_bounds(spec, mags, channels, bc.params_of({}, 0)),
               sb.mvdr_bounds(s_spec, s_mags, channels, bc.params_of({}, 0)), (s_spec, s_mags))


def test_a_power_of_two_per_bin_goes_through_the_float32_restatements_bit_for_bit():
    f = sb.pow2(33)
    assert set(np.log2(f)) == {-float(k) for k in range(13)}                        # every exponent 0 ... 12 is there
    for label, plain, scaled, inputs in _pow2_pairs():
        sb.assert_squares_stay_normal(*inputs)
        for order in sb.ORDERS:
            for (_, a, _), (_, b, _) in zip(plain.views(order), scaled.views(order)):
                sb.assert_squares_stay_normal(b)
                assert _bits_equal(b, _times(a, f)), (label, order)
                assert _bits_equal(_mag_of(b), _times(_mag_of(a), f)), (label, order)
    with pytest.raises(AssertionError):
        sb.assert_squares_stay_normal(np.array([1.0, 1e-20], np.float32))


# ---- mutations: the clip-wide bound passes them, the per-bin bound does not ------------------------------------------------------------
def _clip_wide_passes(got, ref, rows_per_group, floor):
    """Today's assertion: per clip / group, max |got - ref| <= 4 FLOOR max |ref|."""
    g = got.astype(np.complex128).reshape(-1, rows_per_group * got.shape[1] * got.shape[2])
    r = ref.reshape(g.shape)
    return bool((np.abs(g - r).max(axis=1) <= 4.0 * floor * np.abs(r).max(axis=1)).all())


class _Tilted:
    """A tilted case: `views` = [(got: float32 sequential restatement, ref, the input rows, rows per group)], one per reference
    channel for MVDR."""

    def __init__(self, op, arg, kw=None):
        self.op, self.arg = op, arg
        if op == "wpe":
            self.spec = sb.scale_spec(sb.wpe_spec(arg, T), sb.tilt(arg // 2 + 1))
            self.bounds, self.clip_floor, per = sb.wpe_bounds(self.spec, kw), dr.FLOOR, 1
        elif op == "wpe_mc":
            self.spec = sb.scale_spec(sb.mc_spec(64, T, arg[0]), sb.tilt(33))
            self.bounds, self.clip_floor, per = sb.wpe_mc_bounds(self.spec, arg[0], dict(kw or {}, taps=arg[1])), mc.floor_for(None), arg[0]
        else:
            spec, mags = sb.mvdr_inputs(64, T, arg)
            self.spec, self.mags = sb.scale_spec(spec, sb.tilt(33)), sb.scale_mags(mags, sb.tilt(33))
            self.bounds, self.clip_floor, per = sb.mvdr_bounds(self.spec, self.mags, arg, bc.params_of({}, 0)), bc.floor_for(T, arg, {}), 1
        self.views = [(k, got, ref, self.spec if k is None else self.spec[k::arg], per)
                      for k, got, ref in self.bounds.views("sequential")]

    def judge(self, what, mutate, separation=SEPARATION):
        """Mutate every view in turn; -> the smallest E / bound over the views, asserted >= separation, the clip-wide one passing."""
        smallest = np.inf
        for k, got, ref, rows_in, per in self.views:
            assert _clip_wide_passes(got, ref, per, self.clip_floor) and sb.worst(got, ref)[0] <= self.bounds.floor
            bad = mutate(got.copy(), ref, rows_in, k)
            e, r, b = sb.worst(bad, ref)
            over = e / (sb.MARGIN * self.bounds.floor)
            print(f"{self.op} {self.arg} ref {k} {what}: E {e:.3g} at row {r} bin {b} = {over:.3g} x the per-bin bound "
                  f"(floor {self.bounds.floor:.3g}); the clip-wide bound of {4 * self.clip_floor:.3g} of the maximum passes it")
            assert _clip_wide_passes(bad, ref, per, self.clip_floor), (what, k)
            assert over >= separation, (what, k, over)
            smallest = min(smallest, over)
        return smallest


def _quietest(ref, row):
    return int(np.argmin(np.abs(ref[row]).max(axis=0)))


def _input_row(got, ref, rows_in, k):
    b = _quietest(ref, 0)
    got[0, :, b] = rows_in[0, :, b]
    return got


def _last_bin(got, ref, rows_in, k):
    got[2, got.shape[1] // 2, -1] += 1e-3 * np.abs(ref[2, :, -1]).max()
    return got


def _swap(got, ref, rows_in, k):
    scale = np.abs(ref[0]).max(axis=0)
    f = scale.shape[0]
    quiet = set(np.argsort(scale)[:f // 4].tolist())
    assert {f - 3, f - 2} <= quiet
    got[0, :, [f - 3, f - 2]] = got[0, :, [f - 2, f - 3]]
    return got


TILTED = ([("wpe", n_fft) for n_fft in sb.TILTED_WPE] + [("wpe_mc", ck) for ck in sb.TILTED_MC]
          + [("mvdr", c) for c in sb.TILTED_MVDR])


@pytest.mark.parametrize("op,arg", TILTED, ids=[f"{op}-{arg}" for op, arg in TILTED])
def test_the_per_bin_bound_catches_what_the_clip_wide_bound_passes(op, arg):
    case = _Tilted(op, arg)
    case.judge("(a) quietest bin returned as the input row", _input_row)
    case.judge("(c) two adjacent quiet bins swapped", _swap)
    if op == "mvdr":
        case.judge("(b) 1e-3 of its own scale in bin F - 1", _last_bin)
    else:                                                  # the floor of the defaults is above 2.5e-5: caught, but not by 10 x
        case.judge("(b) 1e-3 of its own scale in bin F - 1", _last_bin, separation=1.0)
        _Tilted(op, arg if op == "wpe" else (2, 1), ONE_TAP).judge("(b) 1e-3 of its own scale in bin F - 1, one tap", _last_bin)


# ---- the slips the variant layouts could make (tests/variant_cover.py) land outside the bound ---------------------------------------
def _slipped(what, bounds, rows, run):
    """The float32 sequential restatement of a variant case stands in for the device; `run()` recomputes `rows` of it with the
    slip.  -> by how many bounds the slipped result misses, asserted > 1; the unslipped one passes."""
    got = bounds.f32["sequential"]
    assert sb.worst(got, bounds.ref)[0] <= bounds.floor
    bad = got.copy()
    bad[rows] = run()
    assert not np.array_equal(bad, got)
    e, r, b = sb.worst(bad, bounds.ref)
    over = e / (sb.MARGIN * bounds.floor)
    print(f"{what}: E {e:.3g} at row {r} bin {b} = {over:.3g} x the per-bin bound (floor {bounds.floor:.3g})")
    assert over > 1.0, (what, over)
    return over


def test_a_dropped_or_a_kept_column_of_p_is_caught_at_two_p_block_columns():
    """(C, K) = (5, 6): the second P block column holds channel 4 and three repeats of it.  (1) The last channel's column of P is
    dropped: G's last column is zero.  (2) A repeat is kept and not discarded: column `C` of a bin is the next bin's column 0 in
    the kernel's LDS, so bin b + 1 solves channel 0 with bin b's last column of P."""
    ck = (5, 6)
    c, kw = ck[0], mc.params_of(ck)
    spec = sb.mc_spec(64, T, c)
    bounds = sb.wpe_mc_bounds(spec, c, kw)
    assert sb.mc_label(64, T, ck, None, "variant") in [label for label, _ in sb.variant_cases()]

    def dropped(R, P):
        P = P.copy()
        P[:, :, c - 1] = 0
        return R, P

    def kept(R, P):
        P = P.copy()
        P[1:, :, 0] = P[:-1, :, c - 1]
        return R, P

    for what, slip in (("the last channel's column of P dropped", dropped), ("a repeated last channel kept", kept)):
        _slipped(f"wpe_mc {ck} T {T}, {what}", bounds, slice(0, c),
                 lambda slip=slip: mr.wpe_mc(spec[:c], kw, dtype=np.float32, order="sequential", slip=slip))


def test_a_dropped_last_tap_of_a_partial_block_row_is_caught():
    """adn_wpe at K = 29: the eighth block row holds tap 28 alone.  Dropped, the filter is the one of 28 taps."""
    kw = dict(taps=29)
    spec = sb.wpe_spec(64, T)
    bounds = sb.wpe_bounds(spec, kw)
    assert sb.wpe_label(64, T, kw, "variant") in [label for label, _ in sb.variant_cases()]
    _slipped(f"wpe K 29 T {T}, the last tap dropped", bounds, slice(0, 1),
             lambda: dr.wpe(spec[0], dict(taps=28), dtype=np.float32, order="sequential")[None])


def test_a_last_triangle_entry_of_phi_n_that_is_not_updated_is_caught():
    """adn_mvdr at C = 7: 28 triangle entries over 8 lanes, four rounds, the last one partial: entry 27 is Phi_n[6, 6].  The
    smallest form of the slip: that one entry misses the last frame's term (left at zero instead, the factorisation has no real
    root and the result is NaN, which the bound refuses outright)."""
    c = 7
    spec, mags = sb.mvdr_inputs(64, T, c)
    bounds = sb.mvdr_bounds(spec, mags, c)
    assert sb.mvdr_label(64, T, c, None, "variant") in [label for label, _ in sb.variant_cases()]
    seen = {}

    def record(phi_s, phi_n):
        seen["entry"] = phi_n[:, c - 1, c - 1].copy()
        return phi_s, phi_n

    bf.mvdr(spec[:c, :T - 1], mags[:c, :, :T - 1], None, dtype=np.float32, order="sequential", slip=record)      # the sums over T - 1 frames

    def stale(phi_s, phi_n):
        phi_n = phi_n.copy()
        assert not np.array_equal(phi_n[:, c - 1, c - 1], seen["entry"])
        phi_n[:, c - 1, c - 1] = seen["entry"]
        return phi_s, phi_n

    for ref in bc.refs_of(c):
        got, want = bounds.f32["sequential"][ref], bounds.ref[ref]
        assert sb.worst(got, want)[0] <= bounds.floor
        bad = got.copy()
        bad[0] = bf.mvdr(spec[:c], mags[:c], dict(ref_channel=ref), dtype=np.float32, order="sequential", slip=stale)
        e, r, b = sb.worst(bad, want)
        over = e / (sb.MARGIN * bounds.floor)
        print(f"mvdr C {c} T {T} ref {ref}, Phi_n[{c - 1}, {c - 1}] not updated: E {e:.3g} at row {r} bin {b} = {over:.3g} x the per-bin "
              f"bound (floor {bounds.floor:.3g})")
        assert over > 1.0, (ref, over)


@pytest.mark.parametrize("channels", sb.TILTED_MVDR, ids=lambda c: f"C{c}")
def test_a_mask_column_from_the_neighbouring_frame_is_caught(channels):
    case = _Tilted("mvdr", channels)
    c, group = channels, 1

    def wrong_column(got, ref, rows_in, k):
        b = _quietest(ref, group)
        spec = case.spec[group * c:(group + 1) * c][:, :, b:b + 1]
        mags = case.mags[group * c:(group + 1) * c][:, b:b + 1].copy()
        m = bf.mask(spec, mags, bf.DEFAULTS["mask_floor"])[0]
        t = int(np.argmax(np.abs(m[1:] - m[:-1])))                                  # the frame whose neighbour differs the most
        mags[:, 0, t] = mags[:, 0, t + 1]
        got[group, :, b] = bf.mvdr(spec, mags, dict(ref_channel=k), dtype=np.float32, order="sequential")[:, 0]
        return got

    case.judge("(d) one frame's mask column from its neighbour", wrong_column)
