"""tests/spectral_ref.py checked on the host: the new float64 pieces against np.fft, denoise_ref and the oracle, the zero rule of
the scales, the frame counts of the cases, and the two float32 host forms against each other.

Why floor() takes the larger of two factorisations.  Measured here over the seven sizes with the per-frame scale, for the complex
forward transform: numpy's float32 FFT (pocketfft) 2.1 - 2.7e-7, the radix-2 form 4.5 - 7.3e-7, a ratio of up to 3.0; for the
magnitudes 3.8 - 5.5e-7 against 5.7 - 9.3e-7.  The inverse entries lie within a factor 1.5 of each other (0.7 - 3.0e-6: the window,
the overlap-add and the division weigh as much as the transform).  Four times pocketfft alone would leave a legitimate float32 FFT of
another factorisation almost no room; profiles/spectral_grid.md has every figure.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dref  # noqa: E402
import spectral_ref as sp  # noqa: E402
import stream_ref as sref  # noqa: E402

EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------- float64 pieces
@pytest.mark.parametrize("n_fft", (64, 512))
def test_forward_reference(n_fft):
    from oracle import stft_numpy
    for center in (True, False):
        for hop, length, t in sp.forward_cases(n_fft, center):
            if t > 33:
                continue
            x = sp.audio(n_fft, hop, length)[2]
            got = sp.stft64(x, n_fft, hop, center)
            assert got.shape == (t, n_fft // 2 + 1) and t == stft_numpy.n_frames(length, n_fft, hop, center)
            if center:
                assert np.array_equal(got, dref.stft(x, n_fft, hop))
            xp = np.pad(x.astype(np.float64), n_fft // 2) if center else x.astype(np.float64)
            for f in (0, t // 2, t - 1):                       # frame by frame with np.fft, hop > n_fft included
                frame = dref.hann(n_fft) * xp[f * hop:f * hop + n_fft]
                assert np.array_equal(got[f], np.fft.rfft(frame))
                assert sp.forward_scale(x, n_fft, hop, center)[f] == np.sqrt((frame ** 2).sum())
            # the oracle rounds the float64 spectrum to complex64 (2^-24 per component) and takes a float32 modulus, taken here
            # as good to two units in the last place (2 x 2^-23): 5 x 2^-24 in all
            want = stft_numpy.stft_mag(x, n_fft, hop, center).T.astype(np.float64)
            assert np.all(np.abs(want - np.abs(got)) <= 5.0 * EPS * np.abs(got) + 2.0 ** -126)


@pytest.mark.parametrize("n_fft", (64, 512))
def test_inverse_reference(n_fft):
    """The oracle's inverse accumulates the windowed frames into a float32 signal and the squared windows into a float32 divisor:
    c = ceil(n_fft / hop) rounded additions each, and one rounded division, every one within 2^-24 of sum_f |w frame_f| / wss --
    its own accuracy, (2 c + 2) 2^-24 of that sum."""
    from oracle import griffin_lim_numpy as gl
    for hop, t in sp.istft_cases(n_fft):
        z = sp.spectra(n_fft, hop, t)[0]
        z64 = z.astype(np.complex128)
        got = sp.istft64(z64, hop)
        assert got.shape == (hop * (t - 1),)
        # by hand with np.fft: overlap-add of windowed irfft frames over the window sum-of-squares
        frames = np.fft.irfft(z64, n=n_fft, axis=1) * dref.hann(n_fft)
        y, a, wss = np.zeros(n_fft + hop * (t - 1)), np.zeros(n_fft + hop * (t - 1)), np.zeros(n_fft + hop * (t - 1))
        for f in range(t):
            y[f * hop:f * hop + n_fft] += frames[f]
            a[f * hop:f * hop + n_fft] += np.abs(frames[f])
            wss[f * hop:f * hop + n_fft] += dref.hann(n_fft) ** 2
        big = wss > sp.FLT_MIN
        y[big] /= wss[big]
        a[big] /= wss[big]
        sl = slice(n_fft // 2, n_fft // 2 + hop * (t - 1))
        assert np.allclose(got, y[sl], rtol=1e-13, atol=0)
        want = gl.istft(z64.T, hop).astype(np.float64)          # complex128 in: the oracle's irfft then runs in float64
        assert np.all(np.abs(want - got) <= (2 * -(-n_fft // hop) + 2) * EPS * a[sl] + 2.0 ** -126)
        # imaginary parts at DC and Nyquist are ignored
        z0 = z64.copy()
        z0[:, 0], z0[:, -1] = z0[:, 0].real, z0[:, -1].real
        assert np.array_equal(sp.istft64(z0, hop), got) and np.abs(z64[:, 0].imag).min() > 0


@pytest.mark.parametrize("n_fft", (64, 512))
def test_griffin_lim_reference(n_fft):
    """Iteration 0 is the inverse of the polar start.  With iterations the oracle rounds every pass (float32 signal, complex64
    spectrum, and from the second pass on numpy's irfft of a complex64 spectrum runs in float32: log2(n_fft) stages, taken at 4
    roundings each as in test_radix2_is_an_fft); STFT after inverse STFT is a projection, so the roundings of the passes add and
    do not grow: (iterations + 1) passes of (2 c + 3 + 4 log2 n_fft) 2^-24 each, of the largest sample."""
    from oracle import griffin_lim_numpy as gl
    for hop, t in sp.gl_cases(n_fft):
        mag, rnd = sp.gl_input(n_fft, hop, t)
        m, r = mag[0], rnd[0]
        assert np.array_equal(sp.griffin_lim64(m, r, n_fft, hop, 0), sp.istft64(sp.polar64(m, r), hop))
        one = sp.griffin_lim64(m, r, n_fft, hop, 1)
        by_hand = sp.istft64(dref.stft(sp.istft64(sp.polar64(m, r), hop), n_fft, hop), hop)
        assert np.array_equal(one, by_hand)
        for iterations in (0, 2):
            got = sp.griffin_lim64(m, r, n_fft, hop, iterations)
            want = gl.griffin_lim(m, n_fft, hop, iterations, r.astype(np.float64)).astype(np.float64)
            tol = (iterations + 1) * (2 * -(-n_fft // hop) + 3 + 4 * np.log2(n_fft)) * EPS * np.abs(got).max()
            assert np.abs(want - got).max() <= tol, (hop, t, iterations, float(np.abs(want - got).max()), tol)


def test_radix2_is_an_fft():
    rng = np.random.default_rng(3)
    for n in (2, 8, 64, 4096):
        x = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))).astype(np.complex64)
        got = sp.fft_radix2(x)
        want = np.fft.fft(x.astype(np.complex128))
        assert got.dtype == np.complex64
        # log2(n) stages of one rounded product and one rounded sum each, against the l2 norm of the row
        assert np.all(np.abs(got - want) <= 4.0 * np.log2(n) * EPS * np.sqrt((np.abs(x) ** 2).sum(axis=1, keepdims=True)))
    x = rng.standard_normal((4, 256)).astype(np.float32)
    for form in sp.FORMS:
        spec = sp.rfft32(x, form)
        assert spec.dtype == np.complex64 and np.allclose(spec, np.fft.rfft(x.astype(np.float64)), atol=1e-4)
        back = sp.irfft32(spec, form)
        assert back.dtype == np.float32 and np.allclose(back, x, atol=1e-5)
        spec_i = spec.copy()
        spec_i[:, 0] += 3j
        spec_i[:, -1] -= 2j
        assert np.array_equal(sp.irfft32(spec_i, form), back)


# ---------------------------------------------------------------------------------------------------------------------- zero rule
@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_zero_scale_is_zero_reference(n_fft):
    silent_frames = silent_samples = 0
    for center in (True, False):
        for hop, length, _ in sp.forward_cases(n_fft, center):
            x = sp.audio(n_fft, hop, length)
            for c in range(sp.N_CLIPS):
                zero = sp.forward_scale(x[c], n_fft, hop, center) == 0
                assert np.array_equal(zero, np.abs(sp.stft64(x[c], n_fft, hop, center)).max(axis=1) == 0), (center, hop, length, c)
                silent_frames += int(zero.sum())
    assert silent_frames > 0
    for hop, t in sp.istft_cases(n_fft):
        z = sp.spectra(n_fft, hop, t).astype(np.complex128)
        for c in range(sp.N_CLIPS):
            zero = sp.inverse_scale(z[c], hop, hop * (t - 1)) == 0
            assert np.array_equal(zero, sp.istft64(z[c], hop) == 0), (hop, t, c)
            assert zero.sum() == (t - 1 if hop == n_fft else 0)      # hop = n_fft: the samples whose only tap is w[0] = 0
            silent_samples += int(zero.sum())
    assert silent_samples > 0
    for hop, t in sp.gl_cases(n_fft):
        mag, rnd = sp.gl_input(n_fft, hop, t)
        hat = sp.polar64(mag[1], rnd[1])
        assert np.array_equal(sp.inverse_scale(hat, hop, hop * (t - 1)) == 0, sp.istft64(hat, hop) == 0)
    for w, v, hop, length in sp.denoise_cases(n_fft):
        x = sp.audio(n_fft, hop, length)[1]
        _, y, spec, _ = sp.denoise_host(x, n_fft, hop, w, v, "numpy")
        s64 = spec.astype(np.complex128)
        hat = dref.rephase(dref.stitch(y.astype(np.float64), s64.shape[0], w, v, clamp=True), s64)
        assert np.array_equal(sp.inverse_scale(hat, hop, length) == 0, dref.istft(hat, hop, length) == 0), (w, v, hop, length)
    for w, b, a, hop, length in sp.stream_cases(n_fft):
        x = sp.audio(n_fft, hop, length)[1]
        _, y, _, _ = sp.stream_host(x, n_fft, hop, w, b, a, "numpy")
        s64 = dref.stft(x, n_fft, hop)
        hat = dref.rephase(sref.join(y.astype(np.float64), s64.shape[0], w, b, a), s64)
        assert np.array_equal(sp.inverse_scale(hat, hop, length) == 0, dref.istft(hat, hop, length) == 0), (w, b, a, hop, length)


# ---------------------------------------------------------------------------------------------------------------------- cases
def _staging_floats(n_fft, hop):
    """Floats of LDS stft_mag_kernel asks for (csrc/stft_kernels.hip, launch_m), re-derived from its text."""
    m = n_fft // 2
    fpw = 512 // (m // 8)
    fpb = 8192 // m
    fb = min(fpw, fpb)
    tbl = n_fft + 2 * m + (m + 2)
    mag = (m + 1) * (fpb + 1)
    return tbl + mag + (mag & 1) + max((fb - 1) * hop + n_fft, fb * m * 2)


@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_cases_are_the_intended_ones(n_fft):
    for center in (True, False):
        cases = sp.forward_cases(n_fft, center)
        for hop in sp.forward_hops(n_fft):
            mine = [(length, t) for h, length, t in cases if h == hop]
            assert {t for _, t in mine} == set(sp.FORWARD_T)
            for t in sp.FORWARD_T:
                ls = [length for length, tt in mine if tt == t]
                first, last = min(ls), max(ls)
                # the first and the last length that give T (a centred clip has at least one sample)
                assert first == 1 or sp.n_frames(first - 1, n_fft, hop, center) == (t - 1 if first - 1 >= (0 if center else n_fft) else 0)
                assert sp.n_frames(last + 1, n_fft, hop, center) == t + 1
            if center and 2 * hop - 1 < n_fft:
                assert (2 * hop - 1, 2) in mine
        assert (sp.audio(n_fft, n_fft // 4, 20 * n_fft + 37)[1] == 0).sum() >= 2 * n_fft
        if n_fft in sp.MAX_HOP:
            hop = sp.MAX_HOP[n_fft]
            assert _staging_floats(n_fft, hop) * 4 <= 160 * 1024 < _staging_floats(n_fft, hop + 1) * 4
            t = [tt for h, _, tt in cases if h == hop]
            assert t == [8192 // (n_fft // 2) + 1]                 # one frame more than a workgroup runs
    fb = 8192 // n_fft
    cases = sp.istft_cases(n_fft)
    assert {h for h, _ in cases} == {n_fft // 4, n_fft // 2, n_fft // 8 + 1, 3 * n_fft // 4 + 1, n_fft}
    for hop in sp.istft_hops(n_fft):
        assert {t for h, t in cases if h == hop} == {2, max(fb, 2), fb + 1, 11}
        # hop (T - 1) with an even hop and these T cannot avoid every multiple of 256; the two odd hops do, at every T
        if hop % 2:
            assert all((hop * (t - 1)) % 256 for h, t in cases if h == hop)
    assert all(t % 32 for _, t in sp.gl_cases(n_fft)) and {h for h, _ in sp.gl_cases(n_fft)} == {n_fft // 4, n_fft // 2}
    dn = sp.denoise_cases(n_fft)
    assert {(w, v) for w, v, _, _ in dn} == set(sp.DENOISE_PLANS)
    assert {h for _, _, h, _ in dn} == {n_fft // 4, n_fft // 8 + 1, n_fft // 16} | ({1, 3} if n_fft == 64 else set())
    for hop in sp.denoise_hops(n_fft):
        want = {20 * n_fft + 37, 37, 1, hop - 1, 2 * hop - 1} | ({9000} if n_fft < 512 else set())
        assert {length for w, v, h, length in dn if h == hop and (w, v) == (32, 16)} == {length for length in want if length >= 1}
    assert max(length for *_, length in dn) == max(20 * n_fft + 37, 9000 if n_fft < 512 else 0)
    if n_fft >= 512:
        assert 20 * n_fft + 37 > 2 * 4096                           # more than two 4096-sample spans of dn_resynth_kernel
    assert dref.plan(1 + (20 * n_fft + 37) // (n_fft // 4), 32, 16)[0] > 1
    st = sp.stream_cases(n_fft)
    assert {(w, b, a) for w, b, a, _, _ in st} == set(sp.STREAM_PLANS) and {h for *_, h, _ in st} == {n_fft // 4, n_fft // 8 + 1}
    for w, b, a in sp.STREAM_PLANS:
        for hop in (n_fft // 4, n_fft // 8 + 1):
            assert {length for ww, bb, aa, h, length in st if (ww, bb, aa, h) == (w, b, a, hop)} == {20 * n_fft + 37, b * hop, hop - 1, 1}


# ---------------------------------------------------------------------------------------------------------------------- host forms
@pytest.mark.parametrize("n_fft", sp.N_FFTS)
@pytest.mark.parametrize("entry", sp.ENTRIES)
def test_host_forms_agree(entry, n_fft):
    """Neither host form is broken: the two floors of an (entry, n_fft) lie within a factor 8 of each other, and both are float32
    figures -- above half a rounding, and below 1e-5 of the local scale, a tenth of the tree's global 1e-4."""
    f = dict(sp.floors(entry, n_fft))
    print(f"floor {entry} n_fft {n_fft}: " + ", ".join(f"{form} {f[form]:.3g}" for form in sp.FORMS))
    lo, hi = min(f.values()), max(f.values())
    assert lo > 0 and hi <= 8.0 * lo, f
    assert 0.5 * EPS <= lo and hi <= 1e-5, f
    assert sp.floor(entry, n_fft) == hi


# ---------------------------------------------------------------------------------------------------------------------- the bound itself
def test_local_bound_sees_what_the_global_one_passes():
    """A float32 host result passes check(); the same result with a loud frame's values at 1e-5 of their level in a quiet frame, an
    inverse whose quietest frame enters the sum 1 % low, or a denormal where the exact result is zero passes the tree's global 1e-4 of
    max |ref| and misses the local bound."""
    n_fft, hop = 512, 128
    x = sp.audio(n_fft, hop, 20 * n_fft + 37)[1]
    ref, scale = sp.stft64(x, n_fft, hop), sp.forward_scale(x, n_fft, hop)
    got = sp.stft32(x, n_fft, hop, True, "radix2").astype(np.complex128)
    failures = []
    assert sp.check(got, ref, scale[:, None], "stft_complex", n_fft, "host", failures) <= 1.0 / sp.MARGIN and not failures
    loud, quiet = int(np.argmax(scale)), int(np.argmin(np.where(scale > 0, scale, np.inf)))
    silent = int(np.flatnonzero(scale == 0)[0])
    for frame, value in ((quiet, 1e-5 * ref[loud]), (silent, 1e-40)):
        bad, failures = got.copy(), []
        bad[frame] += value
        assert np.abs(bad - ref).max() <= 1e-4 * np.abs(ref).max()
        sp.check(bad, ref, scale[:, None], "stft_complex", n_fft, "leak", failures)
        assert len(failures) == 1, failures
    t = 11
    z = sp.spectra(n_fft, hop, t)[0]
    z64 = z.astype(np.complex128)
    ref, scale = sp.istft64(z64, hop), sp.inverse_scale(z64, hop, hop * (t - 1))
    failures = []
    assert sp.check(sp.istft32(z, hop, hop * (t - 1), "radix2"), ref, scale, "istft", n_fft, "host", failures) <= 1.0 / sp.MARGIN
    assert not failures
    quietest = int(np.argmin(np.abs(z64).sum(axis=1)))
    late = z64.copy()
    late[quietest] *= 0.99                                         # one quiet frame enters the sum 1 % low
    bad = sp.istft64(late, hop)
    assert np.abs(bad - ref).max() <= 1e-4 * np.abs(ref).max()
    sp.check(bad, ref, scale, "istft", n_fft, "frame 1 % low", failures)
    assert len(failures) == 1, failures
