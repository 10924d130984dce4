"""The per-bin bound of tests/recursive_bounds.py on the host (no GPU): what tests/test_gpu_baseline.py, test_gpu_dereverb_stream.py
and test_gpu_dereverb_mc_stream.py hold the device to, applied to the restatements themselves.

* Both float32 arithmetics ("plain": every product rounded; "fma": the header's pairing and order of every multiply-add) of every
  parity, tilted and power-of-two case pass the bound, and every case's floor is under the cap of 1e-4.  Each case prints the ratio
  of the two floors.
* "fma" really is another arithmetic: on every T = 97 case of the two WPE recursions its result differs from "plain" in at least
  one bit, it is a float32 result (it differs from float64), and it agrees with float64 to its own floor, which is held to the
  cap and to 4 x the plain floor -- two float32 evaluations of the same statements, the fused one with fewer roundings, a
  project's margin apart at the most.
* The power-of-two scale per bin, 2^-((5 b) mod 13), goes through the float32 restatement of the spectral gain bit for bit: M
  scaled by the factor, the state by its square, and no non-zero value's square leaves the normal range.
* The bound catches what today's assertions (restated here with their written constants: per clip / row / group,
  max |got - ref| <= 4 FLOOR max |ref|) pass.  The float32 restatement stands in for the device, in each arithmetic in turn, and
  is mutated; every figure below is the smallest E over the mutated (row, bin)s and the arithmetics, as a multiple of the per-bin
  bound 4 floor, and today's assertion passes every one of them:
    spectral gain, tilted, T 97, the last bin of every clip run with one parameter changed (M and the state both):
      gain_floor 0.09 for 0.1      n_fft 64: E 5.5e-3, 1440 x     n_fft 512: E 3.9e-3,  481 x
      gamma 0.9981 for 0.998       n_fft 64: E 3.3e-2, 8660 x     n_fft 512: E 3.0e-2, 3760 x
      alpha 0.9801 for 0.98        n_fft 64: E 2.2e-3,  571 x     n_fft 512: E 1.5e-3,  180 x
      (every figure here is the clip or row that shows the change the LEAST; the one that shows it the most sits 1.2 to 3 x higher)
    wpe_online, tilted, T 97, defaults, the last bin of every row returns its input:
                                   n_fft 64: E 0.15, 12200 x      n_fft 512: E 0.13, 45400 x
    wpe_mc_online, tilted, n_fft 64, T 97, (C, K) = (2, 16), the last bin of every channel returns its input:
                                   E 0.16, 14800 x
    1e-5 of the last bin's own scale added to one frame of that bin, untilted, defaults:
      wpe_online n_fft 64, T 23:              20.6 x              wpe_mc_online (2, 16), n_fft 64, T 23:  15.2 x
      wpe_online n_fft 512, T 40:              8.1 x  (asserted as "fails the bound": 1e-5 against 4 x a floor of 3.1e-7)
    wpe_mc_online, the variant case (C, K) = (7, 4), n_fft 64, T 97 (tests/variant_cover.py), the last channel's column of G never
    updated, so that the channel returns its input -- what the offline kernel's dropped last column of P becomes here:
                                   E 0.14, 15300 x in the bin that shows it the least
  A separation of 10 x is asserted for every line but the one at n_fft 512, T 40.  Not caught, and not claimed: the same 1e-5 on a T = 97 case, whose
  floor of 3e-6 puts the bound at 1.2e-5.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recursive_bounds as rb  # noqa: E402
import solver_bounds as sb  # noqa: E402
import baseline_ref as br  # noqa: E402
import dereverb_mc_stream_cases as msc  # noqa: E402
import dereverb_mc_stream_ref as ms  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402

HOST_CASES = tuple(rb.host_cases())
T = rb.TILTED_FRAMES
SEPARATION = 10.0


def test_the_module_shares_solver_bounds_and_caches_on_the_bits():
    assert rb.sb is sb and rb.CAP == 1e-4 and sb.MARGIN == 4.0
    spec = rb.gain_spec(64, 5)
    assert rb.spectral_bounds(spec) is rb.spectral_bounds(spec.copy())
    assert rb.wpe_online_bounds(rb.online_spec(64, 5)) is rb.wpe_online_bounds(rb.online_spec(64, 5).copy())
    b = rb.spectral_bounds(spec)
    assert b.ref.shape == (3, 5, 33) and b.state.ref.shape == (9, 1, 33) and b.floors["pairwise"] == b.floors["sequential"]
    # a reference entry of 0 has to be exactly 0
    ref = np.zeros((3, 3, 4))
    ref[:, 0, :] = 1.0
    got = ref.copy()
    got[2, 1, 3] = 1e-30
    assert sb.per_bin(rb.state_rows(got), rb.state_rows(ref))[7, 3] == np.inf and sb.per_bin(rb.state_rows(ref), rb.state_rows(ref)).max() == 0


@pytest.mark.parametrize("label,case", HOST_CASES, ids=[label for label, _ in HOST_CASES])
def test_both_float32_arithmetics_pass_the_bound_and_the_cap(label, case):
    b = case()
    rb.assert_cap(label, b)
    assert b.floor >= sb.EPS and b.floor >= max(b.floors.values())
    for a in rb.ARITHMETICS:
        e, r, col = sb.worst(b.f32[a], b.ref)
        assert e == b.by_arithmetic[a] <= b.floor <= sb.MARGIN * b.floor / 4.0, (a, e, r, col)
    plain, fma = b.by_arithmetic["plain"], b.by_arithmetic["fma"]
    print(f"{label}: floor plain {plain:.3g} fma {fma:.3g}, fma / plain {fma / plain if plain > 0 else float('nan'):.2f}")


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


RECURSIONS_T97 = tuple((label, case) for label, case in HOST_CASES if label.startswith("wpe_") and f" T {T} " in label)


@pytest.mark.parametrize("label,case", RECURSIONS_T97, ids=[label for label, _ in RECURSIONS_T97])
def test_fma_is_another_float32_arithmetic(label, case):
    b = case()
    plain, fma = b.f32["plain"], b.f32["fma"]
    assert plain.dtype == fma.dtype == np.complex64 and not _bits_equal(plain, fma)
    assert 0.0 < b.by_arithmetic["fma"] <= min(rb.CAP, sb.MARGIN * max(b.by_arithmetic["plain"], sb.EPS))
    # the first D frames come back bit for bit in both
    delay = 8 if "'delay': 8" in label else 1 if "'delay': 1" in label else 3
    assert _bits_equal(plain[:, :delay], fma[:, :delay])


def test_fma_of_the_restatement_is_one_rounding():
    a, b, c = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12), np.float32(-1.0)
    assert float(ds.fma(a, b, c)) == 2.0 ** -11 + 2.0 ** -24                          # the product's last bit survives
    assert float(np.float32(a * b) + c) == 2.0 ** -11                                 # ... and is lost with a rounded product
    z, w, acc = (np.array([v], np.complex64) for v in (1 + 2j, 3 - 1j, 0.5 + 0.25j))
    assert ds.cfma(z, w, acc)[0] == acc[0] + z[0] * w[0] and ds.cfma_conj(z, w, acc)[0] == acc[0] + z[0] * np.conj(w[0])
    zero = ds.cx(np.float32(-0.0), np.float32(0.0))
    assert np.signbit(zero.real) and not np.signbit(zero.imag)


# ---- the power-of-two scale goes through the spectral gain's float32 restatement bit for bit ------------------------------------------
def test_a_power_of_two_per_bin_goes_through_the_spectral_gain_bit_for_bit():
    f = sb.pow2(rb.POW2_GAIN // 2 + 1)
    assert set(np.log2(f)) == {-float(k) for k in range(13)}                        # every exponent 0 ... 12 is there
    base = rb.gain_spec(rb.POW2_GAIN, T)
    scaled = sb.scale_spec(base, f)
    sb.assert_squares_stay_normal(base, scaled)
    f32 = f.astype(np.float32)
    for c in range(3):
        m, st = br.spectral_gain(base[c], dtype=np.float32)
        ms_, sts = br.spectral_gain(scaled[c], dtype=np.float32)
        sb.assert_squares_stay_normal(m, ms_, st, sts)
        assert _bits_equal(ms_, m * f32[:, None]), c
        assert _bits_equal(sts, st * (f32 * f32)[None, :]), c
    plain, there = rb.spectral_bounds(base), rb.spectral_bounds(scaled)
    assert _bits_equal(there.f32["plain"], plain.f32["plain"] * f32) and _bits_equal(there.state.f32["plain"], plain.state.f32["plain"] * (f32 * f32))


# ---- mutations: today's assertions pass them, the per-bin bound does not ----------------------------------------------------------------
def _wide_passes(got, ref, rows_per_group, floor):
    """Today's assertion: per clip / row / group, max |got - ref| <= 4 FLOOR max |ref|."""
    g = np.asarray(got).astype(np.complex128).reshape(-1, rows_per_group * got.shape[1] * got.shape[2])
    r = np.asarray(ref).astype(np.complex128).reshape(g.shape)
    return bool((np.abs(g - r).max(axis=1) <= 4.0 * floor * np.abs(r).max(axis=1)).all())


def _magnitudes(d):
    """mag_out of a result d (rows, T, F), laid out like d: today's assertion holds it against |d64| on the row's scale."""
    return np.sqrt(ds._power(d, np.float32))


def _judge(what, bounds, todays, mutate, cells, separation=SEPARATION):
    """For each arithmetic: the float32 restatement passes `todays` and the bound; mutated, it still passes `todays` and every
    mutated (row, bin) of `cells` exceeds the bound by `separation`.  -> the smallest E / bound."""
    smallest = np.inf
    for a in rb.ARITHMETICS:
        got = bounds.f32[a]
        assert todays(got) and sb.worst(got, bounds.ref)[0] <= bounds.floor
        bad = mutate(got.copy())
        e = sb.per_bin(bad, bounds.ref)
        at = min(cells, key=lambda rc: e[rc])
        over = float(e[at]) / (sb.MARGIN * bounds.floor)
        print(f"{what} [{a}]: E {float(e[at]):.3g} at row {at[0]} bin {at[1] % e.shape[1]} = {over:.3g} x the per-bin bound (floor {bounds.floor:.3g}); "
              "today's assertion passes it")
        assert todays(bad), (what, a)
        assert over >= separation, (what, a, over)
        smallest = min(smallest, over)
    return smallest


GAIN_CHANGES = (dict(gain_floor=0.09), dict(gamma=0.9981), dict(alpha=0.9801))


@pytest.mark.parametrize("change", GAIN_CHANGES, ids=lambda c: "-".join(c))
@pytest.mark.parametrize("n_fft", rb.TILTED_GAIN)
def test_a_wrong_parameter_in_the_last_bin_of_the_spectral_gain_is_caught(n_fft, change):
    spec = sb.scale_spec(rb.gain_spec(n_fft, T), sb.tilt(n_fft // 2 + 1))
    bounds = rb.spectral_bounds(spec)
    wrong = [br.spectral_gain(s[:, -1:], change, dtype=np.float32) for s in spec]      # the last bin alone, one parameter changed

    def mutate(got):
        got[:, :, -1] = np.stack([m[0] for m, _ in wrong])
        return got

    _judge(f"spectral gain n_fft {n_fft} {change} in the last bin", bounds, lambda got: _wide_passes(got, bounds.ref, 1, br.FLOOR),
           mutate, [(c, -1) for c in range(3)])
    # the state that comes with those magnitudes: today's assertion (each row of P, Pmin, S against the row's largest value, as
    # (clips * 3, F)) passes it too, and its own per-bin bound does not
    state = bounds.state.f32["plain"]
    bad_state = state.copy()
    bad_state[:, 0, -1] = np.concatenate([st[:, 0] for _, st in wrong])
    per_row = lambda st: _wide_passes(st.transpose(0, 2, 1), bounds.state.ref.transpose(0, 2, 1), 1, br.FLOOR)  # noqa: E731
    assert per_row(state) and per_row(bad_state) and not np.array_equal(bad_state, state)
    assert sb.per_bin(bad_state, bounds.state.ref)[:, -1].max() > sb.MARGIN * bounds.state.floor


def _online_todays(bounds, per, floor):
    def todays(got):
        mags = np.abs(np.asarray(bounds.ref))
        return _wide_passes(got, bounds.ref, per, floor) and _wide_passes(_magnitudes(got), mags, per, floor)
    return todays


@pytest.mark.parametrize("n_fft", rb.TILTED_ONLINE)
def test_a_last_bin_that_returns_its_input_is_caught_wpe_online(n_fft):
    spec = sb.scale_spec(rb.online_spec(n_fft, T), sb.tilt(n_fft // 2 + 1))
    bounds = rb.wpe_online_bounds(spec)

    def mutate(got):
        got[:, :, -1] = spec[:, :, -1]
        return got

    _judge(f"wpe_online n_fft {n_fft} last bin returned as the input", bounds, _online_todays(bounds, 1, ds.FLOOR), mutate,
           [(r, -1) for r in range(3)])


def test_a_last_bin_that_returns_its_input_is_caught_wpe_mc_online():
    ck = rb.TILTED_MC[0]
    spec = sb.scale_spec(rb.mc_spec(64, T, ck[0]), sb.tilt(33))
    bounds = rb.wpe_mc_online_bounds(spec, ck[0], msc.params_of(ck))

    def mutate(got):
        got[:, :, -1] = spec[:, :, -1]
        return got

    _judge(f"wpe_mc_online {ck} last bin returned as the input", bounds, _online_todays(bounds, ck[0], ms.FLOOR), mutate,
           [(r, -1) for r in range(3 * ck[0])])


def test_a_last_channel_whose_taps_are_never_updated_is_caught_wpe_mc_online():
    """(C, K) = (7, 4), a variant case (tests/variant_cover.py): N = 28, the last four rows of the 32-row layout idle.  The slip
    the offline kernel's "last column of P dropped" becomes here: the last channel's column of G stays what frame 0 made it, zero,
    so that channel returns its input.  Run frame by frame through the state, in both arithmetics."""
    ck = (7, 4)
    c, kw = ck[0], msc.params_of(ck)
    spec = rb.mc_spec(64, T, c)
    bounds = rb.wpe_mc_online_bounds(spec, c, kw)
    label = rb.mc_label(64, T, ck, None, "variant")
    assert label in [name for name, _ in rb.variant_cases()]
    rb.assert_cap(label, bounds)
    for a in rb.ARITHMETICS:
        got = bounds.f32[a]
        assert sb.worst(got, bounds.ref)[0] <= bounds.floor
        state, frames = None, []
        for t in range(T):
            d, state = ms.wpe_mc_online(spec[:c, t:t + 1], kw, dtype=np.float32, state=state, first_frame=t, with_state=True, arithmetic=a)
            state["G"][:, c - 1] = 0
            frames.append(d)
        bad = got.copy()
        bad[:c] = np.concatenate(frames, axis=1)
        e = sb.per_bin(bad, bounds.ref)[c - 1]                                     # the last channel of group 0, every bin
        over = float(e.min()) / (sb.MARGIN * bounds.floor)
        print(f"wpe_mc_online {ck} T {T}, the last channel's taps never updated [{a}]: the bin that shows it the least has E {float(e.min()):.3g} "
              f"= {over:.3g} x the per-bin bound (floor {bounds.floor:.3g})")
        assert over >= SEPARATION, (a, over)
        assert np.array_equal(bad[c - 1, 3:], spec[c - 1, 3:])                     # that channel is its input


def _added(bounds, row):
    def mutate(got):
        got[row, got.shape[1] // 2, -1] += 1e-5 * np.abs(bounds.ref[row, :, -1]).max()
        return got
    return mutate


@pytest.mark.parametrize("n_fft,n_frames,separation", ((64, 23, SEPARATION), (512, 40, 1.0)), ids=("64-T23", "512-T40"))
def test_1e_5_of_its_own_scale_in_the_last_bin_is_caught_wpe_online(n_fft, n_frames, separation):
    bounds = rb.wpe_online_bounds(rb.online_spec(n_fft, n_frames))
    over = _judge(f"wpe_online n_fft {n_fft} T {n_frames} 1e-5 of its own scale in bin F - 1", bounds,
                  _online_todays(bounds, 1, ds.FLOOR), _added(bounds, 2), [(2, -1)], separation)
    assert separation >= SEPARATION or 1.0 < over < SEPARATION                      # T 40: caught, the arithmetic caps it below 10 x


def test_1e_5_of_its_own_scale_in_the_last_bin_is_caught_wpe_mc_online():
    ck, n_frames = (2, 16), 23
    bounds = rb.wpe_mc_online_bounds(rb.mc_spec(64, n_frames, ck[0]), ck[0], msc.params_of(ck))
    row = 2 * ck[0] + 1
    _judge(f"wpe_mc_online {ck} T {n_frames} 1e-5 of its own scale in bin F - 1", bounds, _online_todays(bounds, ck[0], ms.FLOOR),
           _added(bounds, row), [(row, -1)])
