"""Cases, float64 references, local error scales and float32 host floors of the spectral entry points -- TEST INFRASTRUCTURE.

Every spectral entry point (stft_magnitude, stft_complex, istft, Griffin-Lim, Denoiser.windows / resynth, StreamDenoiser) is
checked at all seven n_fft by tests/test_gpu_spectral_grid.py against the float64 definitions of include/adn.h.  This file holds
what that file and tests/test_spectral_ref_host.py share; it is numpy only.  denoise_ref / stream_ref already state stft, istft,
rephase, stitch, windows, join and resynth in float64: they are imported, not restated.  New here:

* signals whose level changes from frame to frame (steps of 2^(-12 u), one per n_fft / 2 samples; clip 1 with a stretch of exact
  zeros), and spectra whose level changes per frame, so that a value that leaks from a loud frame into a quiet one shows;
* the float64 magnitude STFT under adn_stft_n_frames' frame rule (center on and off, hop > n_fft included), the inverse STFT to
  hop (T - 1) samples, and the Griffin-Lim loop of adn_griffin_lim;
* LOCAL scales.  Forward: every bin of frame f is measured against || w x_f ||_2, the l2 norm of the windowed frame.  Inverse:
  sample n at p = n + n_fft / 2 against  sum_f w[p - f hop] rms_f / wss[n]  over the frames that cover p, rms_f =
  || irfft(X^_f) ||_2 / sqrt(n_fft) with X^_f the spectrum the frame is inverted from (the division dropped where wss <= FLT_MIN,
  as in the definition).  Where a scale is zero the exact result is zero and the device has to return exactly zero;
* two float32 HOST forms of every operation: (a) numpy's float32 FFT (pocketfft), (b) a plain radix-2 FFT in complex64 with
  float32 twiddles, its inverse the conjugate of the forward.  Both multiply by a float32 window, overlap-add in float32 and
  divide in float32;
* floor(entry, n_fft): the worst |host32 - ref64| / scale over all of this file's cases of that entry and size and over both
  host forms -- what a legitimate float32 implementation of the operation costs, in units of the local scale.  The device bound
  is 4 x floor x scale, element by element (the margin of tests/quality_ref.py::BOUND).  The floor takes the larger of two
  factorisations because pocketfft alone is an unusually accurate one (see tests/test_spectral_ref_host.py).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dref  # noqa: E402
import stream_ref as sref  # noqa: E402

N_FFTS = (64, 128, 256, 512, 1024, 2048, 4096)
N_CLIPS = 3
MARGIN = 4.0                                   # device bound = MARGIN * floor * scale
FLT_MIN = float(np.finfo(np.float32).tiny)
FORMS = ("numpy", "radix2")
ENTRIES = ("stft_magnitude", "stft_complex", "istft", "griffin_lim", "denoise_windows", "denoise_resynth", "stream_windows",
           "stream_audio")

# Largest hop stft_magnitude accepts at the two sizes that stage a batch of frames in LDS (csrc/stft_kernels.hip, launch_m):
# floats = TBL + mag + (mag & 1) + max(span, 2 FB M) <= 160 KiB / 4 = 40960, with M = n_fft / 2, TBL = 5 M + 2,
# FB = min(512 / (M / 8), 8192 / M) frames per batch, mag = (M + 1) (8192 / M + 1) and span = (FB - 1) hop + n_fft.
#   n_fft 2048: TBL 5122, mag 9225 (+1), FB 4: 3 hop + 2048 <= 40960 - 14348 = 26612  ->  hop <= 8188
#   n_fft 4096: TBL 10242, mag 10245 (+1), FB 2: hop + 4096 <= 40960 - 20488 = 20472  ->  hop <= 16376
MAX_HOP = {2048: 8188, 4096: 16376}


# ---------------------------------------------------------------------------------------------------------------------- signals
def audio(n_fft, hop, length, salt=0):
    """(N_CLIPS, length) float32: uniform [-1, 1] under a step envelope 2^(-12 u), one step per n_fft / 2 samples.  Clip 1 holds
    2 n_fft + hop exact zeros from a third of its length on wherever the clip is long enough to keep n_fft samples behind them."""
    rng = np.random.default_rng([n_fft, hop, length, salt])
    x = rng.uniform(-1.0, 1.0, (N_CLIPS, length))
    step = n_fft // 2
    env = 2.0 ** (-12.0 * rng.random((N_CLIPS, -(-length // step))))
    x *= np.repeat(env, step, axis=1)[:, :length]
    quiet = 2 * n_fft + hop
    if length >= length // 3 + quiet + n_fft:
        x[1, length // 3:length // 3 + quiet] = 0.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def spectra(n_fft, hop, n_frames, salt=0):
    """(N_CLIPS, T, F) complex64: complex normal times 2^(-12 u) per frame.  The imaginary parts at DC and Nyquist are non-zero:
    the inverse transform ignores them, as numpy's irfft does."""
    rng = np.random.default_rng([n_fft, hop, n_frames, salt, 1])
    shape = (N_CLIPS, n_frames, n_fft // 2 + 1)
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    z *= 2.0 ** (-12.0 * rng.random((N_CLIPS, n_frames, 1)))
    z = z.astype(np.complex64)
    z.setflags(write=False)
    return z


def gain_offset(n_bins, width):
    """The elementwise map that stands where the network does: y = x * gain + offset, gain in [-0.25, 1.25), offset in [-0.1, 0.1),
    (n_bins, width) float32 each -- the same for every window, so that a window's y does not depend on the batch it is in.  Negative
    values reach the clamp, and offsets on silent frames reach the zero-magnitude rule of the phase."""
    rng = np.random.default_rng([n_bins, width, 11])
    return ((rng.random((n_bins, width)) * 1.5 - 0.25).astype(np.float32), (rng.random((n_bins, width)) * 0.2 - 0.1).astype(np.float32))


def apply_map(win):
    """(K, F, width) float32 -> float32, two rounded operations like the device's x * g + o."""
    g, o = gain_offset(win.shape[-2], win.shape[-1])
    return (win.astype(np.float32) * g).astype(np.float32) + o


# ---------------------------------------------------------------------------------------------------------------------- float64
def n_frames(length, n_fft, hop, center):
    """adn_stft_n_frames."""
    lp = length + 2 * (n_fft // 2) if center else length
    return 0 if lp < n_fft else 1 + (lp - n_fft) // hop


def _frame_index(length, n_fft, hop, center):
    t = n_frames(length, n_fft, hop, center)
    assert t >= 1, (length, n_fft, hop, center)
    return hop * np.arange(t)[:, None] + np.arange(n_fft)[None, :]


def frames64(x, n_fft, hop, center=True):
    """(L,) -> (T, n_fft) float64 windowed frames, zero padded by n_fft / 2 on both sides when centred."""
    xp = np.asarray(x, np.float64)
    if center:
        xp = np.pad(xp, n_fft // 2)
    return dref.hann(n_fft) * xp[_frame_index(len(x), n_fft, hop, center)]


def stft64(x, n_fft, hop, center=True):
    """(L,) -> (T, F) complex128 under adn_stft_n_frames' frame rule; centred it is denoise_ref.stft."""
    return np.fft.rfft(frames64(x, n_fft, hop, center), axis=1)


def forward_scale(x, n_fft, hop, center=True):
    """(T,): || w x_f ||_2, the scale of every bin of frame f."""
    return np.sqrt((frames64(x, n_fft, hop, center) ** 2).sum(axis=1))


def istft64(spec, hop):
    """(T, F) complex -> (hop (T - 1),) float64."""
    return dref.istft(spec, hop, hop * (spec.shape[0] - 1))


def _overlap_add(rows, hop):
    t, n = rows.shape
    y = np.zeros(n + hop * (t - 1), dtype=rows.dtype)
    for f in range(t):
        y[f * hop:f * hop + n] += rows[f]
    return y


def inverse_scale(spec_hat, hop, length):
    """(T, F) complex, the spectra the frames are inverted from -> (length,): sum_f w[p - f hop] rms_f / wss at p = n + n_fft / 2."""
    t, n_fft = spec_hat.shape[0], 2 * (spec_hat.shape[1] - 1)
    rms = np.sqrt((np.fft.irfft(spec_hat, n=n_fft, axis=1) ** 2).sum(axis=1) / n_fft)
    y = _overlap_add(dref.hann(n_fft)[None, :] * rms[:, None], hop)
    wss = dref.window_sumsquare(t, n_fft, hop)
    y = np.where(wss > FLT_MIN, y / np.where(wss > 0, wss, 1.0), y)
    return y[n_fft // 2:n_fft // 2 + length]


def polar64(mag, rnd):
    """(F, T) magnitudes and uniforms -> (T, F) complex128: the start of adn_griffin_lim."""
    return (np.asarray(mag, np.float64) * np.exp(2j * np.pi * np.asarray(rnd, np.float64))).T


def griffin_lim64(mag, rnd, n_fft, hop, iterations):
    """adn_griffin_lim in float64: polar start, then audio = istft(S), S = stft(audio), `iterations` times, and a last istft.  The
    target magnitude is never re-imposed (include/adn.h)."""
    spec = polar64(mag, rnd)
    length = hop * (spec.shape[0] - 1)
    for it in range(iterations + 1):
        out = dref.istft(spec, hop, length)
        if it < iterations:
            spec = dref.stft(out, n_fft, hop)
    return out


# ---------------------------------------------------------------------------------------------------------------------- float32 host forms
@functools.lru_cache(maxsize=None)
def _r2_tables(n):
    rev = np.zeros(n, dtype=np.int64)
    bits = n.bit_length() - 1
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    tw = np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)       # float32 twiddles, rounded once from float64
    return rev, tw


def fft_radix2(x):
    """(..., n) complex64 -> complex64: decimation in time, radix 2, every operation in complex64."""
    x = np.asarray(x)
    assert x.dtype == np.complex64
    n = x.shape[-1]
    rev, tw = _r2_tables(n)
    lead = x.shape[:-1]
    x = x.reshape(-1, n)[:, rev]
    m = 1
    while m < n:
        x = x.reshape(-1, n // (2 * m), 2, m)
        a, b = x[:, :, 0, :], x[:, :, 1, :] * tw[::n // (2 * m)]
        out = np.empty_like(x)
        np.add(a, b, out=out[:, :, 0, :])
        np.subtract(a, b, out=out[:, :, 1, :])
        x = out
        m *= 2
    return x.reshape(lead + (n,))


def rfft32(frames, form):
    """(T, n) float32 -> (T, n / 2 + 1) complex64."""
    assert frames.dtype == np.float32
    if form == "numpy":
        out = np.fft.rfft(frames, axis=-1)
    else:
        out = fft_radix2(frames.astype(np.complex64))[..., :frames.shape[-1] // 2 + 1]
    assert out.dtype == np.complex64, out.dtype
    return out


def irfft32(spec, form):
    """(T, F) complex64 -> (T, n) float32; the imaginary parts at DC and Nyquist are ignored."""
    assert spec.dtype == np.complex64
    m = spec.shape[-1] - 1
    n = 2 * m
    if form == "numpy":
        out = np.fft.irfft(spec, n=n, axis=-1)
    else:
        full = np.empty(spec.shape[:-1] + (n,), dtype=np.complex64)
        full[..., :m + 1] = spec
        full[..., 0] = spec[..., 0].real
        full[..., m] = spec[..., m].real
        full[..., m + 1:] = np.conj(spec[..., m - 1:0:-1])
        out = np.conj(fft_radix2(np.conj(full))).real * np.float32(1.0 / n)
    assert out.dtype == np.float32, out.dtype
    return out


def hann32(n_fft):
    return dref.hann(n_fft).astype(np.float32)


def stft32(x, n_fft, hop, center, form):
    xp = np.asarray(x, np.float32)
    if center:
        xp = np.pad(xp, n_fft // 2)
    return rfft32(hann32(n_fft) * xp[_frame_index(len(x), n_fft, hop, center)], form)


def istft32(spec, hop, length, form):
    """(T, F) complex64 -> (length,) float32: float32 window, float32 overlap-add in ascending frame order, float32 division."""
    t, n_fft = spec.shape[0], 2 * (spec.shape[1] - 1)
    w = hann32(n_fft)
    y = _overlap_add(irfft32(spec, form) * w, hop)
    wss = _overlap_add(np.broadcast_to(w * w, (t, n_fft)), hop)
    assert y.dtype == np.float32 and wss.dtype == np.float32
    y = np.where(wss > np.float32(FLT_MIN), y / np.where(wss > 0, wss, np.float32(1.0)), y)
    return y[n_fft // 2:n_fft // 2 + length]


def polar32(mag, rnd):
    return (np.asarray(mag, np.float32) * np.exp(2j * np.pi * np.asarray(rnd, np.float64)).astype(np.complex64)).T.astype(np.complex64)


def rephase32(m, spec):
    """m (F, T) float32, spec (T, F) complex64 -> complex64."""
    mag = np.abs(spec)
    assert mag.dtype == np.float32
    s = m.T.astype(np.float32) / np.where(mag > 0, mag, np.float32(1.0))
    return np.where(mag > 0, spec * s, m.T.astype(np.complex64)).astype(np.complex64)


def stitch32(y, n_frames_, window, overlap):
    """denoise_ref.stitch (clamped) with float32 weights, products and sums."""
    k, width = dref.plan(n_frames_, window, overlap)
    out = np.zeros((y.shape[1], n_frames_), dtype=np.float32)
    for i in range(k):
        lo = i * (window - overlap)
        n = min(width, n_frames_ - lo)
        out[:, lo:lo + n] += dref.weights(i, k, width, overlap)[:n].astype(np.float32) * y[i, :, :n]
    return np.maximum(out, np.float32(0.0))


# ---------------------------------------------------------------------------------------------------------------------- cases
def _unique(seq):
    seen, out = set(), []
    for c in seq:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


FORWARD_T = (1, 2, 33, 129, 130)           # cross every frames-per-workgroup value (2 ... 128) and the 16- / 32-frame groups


def forward_hops(n_fft):
    return (n_fft // 4, n_fft // 2, n_fft // 8 + 1, n_fft, n_fft + 3)


def forward_cases(n_fft, center):
    """(hop, length, T): every T of FORWARD_T at the first and the last length that gives it; centred also L = 2 hop - 1 < n_fft; at
    n_fft 2048 and 4096 the largest hop the staging kernel accepts, with more frames than one workgroup runs."""
    out = []
    for hop in forward_hops(n_fft):
        for t in FORWARD_T:
            lo, hi = ((t - 1) * hop, t * hop - 1) if center else (n_fft + (t - 1) * hop, n_fft + t * hop - 1)
            out += [(hop, max(lo, 1)), (hop, hi)]
        if center and 2 * hop - 1 < n_fft:
            out.append((hop, 2 * hop - 1))
    if n_fft in MAX_HOP:
        t = 8192 // (n_fft // 2) + 1
        out.append((MAX_HOP[n_fft], ((t - 1) * MAX_HOP[n_fft]) if center else n_fft + (t - 1) * MAX_HOP[n_fft]))
    return [(hop, length, n_frames(length, n_fft, hop, center)) for hop, length in _unique(out) if length >= 1]


def istft_hops(n_fft):
    return (n_fft // 4, n_fft // 2, n_fft // 8 + 1, 3 * n_fft // 4 + 1, n_fft)


def istft_cases(n_fft):
    """(hop, T), T in {2, FB, FB + 1, 11} with FB = 8192 / n_fft frames per pass of istft_frames_kernel."""
    fb = 8192 // n_fft
    return [(hop, t) for hop in istft_hops(n_fft) for t in _unique((2, max(fb, 2), fb + 1, 11))]


GL_ITERATIONS = (0, 1, 3)


def gl_cases(n_fft):
    """(hop, T): no T is a multiple of the 32-wide tile of gl_polar_kernel."""
    return [(hop, t) for hop in (n_fft // 4, n_fft // 2) for t in (2, 31, 40)]


def gl_input(n_fft, hop, t):
    """magnitude and rnd, (N_CLIPS, F, T) float32 each; the magnitude's level changes per frame."""
    mag = np.ascontiguousarray(np.abs(spectra(n_fft, hop, t, salt=5)).transpose(0, 2, 1)).astype(np.float32)
    rnd = np.random.default_rng([n_fft, hop, t, 6]).random(mag.shape).astype(np.float32)
    return mag, rnd


DENOISE_PLANS = ((32, 16), (16, 0))            # window, overlap


def denoise_hops(n_fft):
    return (n_fft // 4, n_fft // 8 + 1, n_fft // 16) + ((1, 3) if n_fft == 64 else ())


def denoise_cases(n_fft):
    """(window, overlap, hop, length)."""
    out = []
    for w, v in DENOISE_PLANS:
        for hop in denoise_hops(n_fft):
            lengths = (20 * n_fft + 37,) + ((9000,) if n_fft < 512 else ()) + (37, 1, hop - 1, 2 * hop - 1)
            out += [(w, v, hop, length) for length in lengths if length >= 1]
    return _unique(out)


STREAM_PLANS = ((32, 8, 4), (16, 1, 0))        # window, block, look-ahead


def stream_cases(n_fft):
    """(window, block, lookahead, hop, length)."""
    out = []
    for w, b, a in STREAM_PLANS:
        for hop in (n_fft // 4, n_fft // 8 + 1):
            out += [(w, b, a, hop, length) for length in (20 * n_fft + 37, b * hop, hop - 1, 1) if length >= 1]
    return _unique(out)


# ---------------------------------------------------------------------------------------------------------------------- comparisons
def ratio(err, scale):
    """Worst err / scale where the scale is positive (0 when it is positive nowhere)."""
    err, scale = np.broadcast_arrays(np.abs(err), scale)
    ok = scale > 0
    return float((err[ok] / scale[ok]).max()) if ok.any() else 0.0


def windows_scale(frame_scale, shape, first):
    """Per-frame scales (T,) -> the scale of every element of a stack of windows `shape` = (K, F, width) whose element [k, :, j]
    is frame first[k] + j (zero outside [0, T))."""
    k, _, width = shape
    idx = np.asarray(first)[:, None] + np.arange(width)[None, :]
    ok = (idx >= 0) & (idx < len(frame_scale))
    return np.broadcast_to(np.where(ok, frame_scale[np.clip(idx, 0, len(frame_scale) - 1)], 0.0)[:, None, :], shape)


def denoise_first(t, window, overlap):
    k, _ = dref.plan(t, window, overlap)
    return np.arange(k) * (window - overlap)


def stream_first(t, window, block, lookahead):
    return np.arange(sref.n_steps(t, block)) * block + block + lookahead - window


@functools.lru_cache(maxsize=None)
def _forward_ratios(n_fft, center):
    """-> ((form, worst ratio of the magnitudes, worst ratio of the complex values), ...) over forward_cases."""
    worst = {form: [0.0, 0.0] for form in FORMS}
    for hop, length, _ in forward_cases(n_fft, center):
        x = audio(n_fft, hop, length)
        for c in range(N_CLIPS):
            ref, scale = stft64(x[c], n_fft, hop, center), forward_scale(x[c], n_fft, hop, center)[:, None]
            for form in FORMS:
                got = stft32(x[c], n_fft, hop, center, form)
                worst[form][0] = max(worst[form][0], ratio(np.abs(got).astype(np.float64) - np.abs(ref), scale))
                worst[form][1] = max(worst[form][1], ratio(got.astype(np.complex128) - ref, scale))
    return tuple((form, r[0], r[1]) for form, r in worst.items())


def denoise_host(x, n_fft, hop, window, overlap, form):
    """One clip through the float32 host form of the denoiser with the map in the network's place ->
    windows32 (K, F, width), y32, spec32 (T, F), audio32 (L,)."""
    spec = stft32(x, n_fft, hop, True, form)
    win = dref.windows(np.abs(spec), window, overlap)
    y = apply_map(win)
    out = istft32(rephase32(stitch32(y, spec.shape[0], window, overlap), spec), hop, len(x), form)
    return win, y, spec, out


def stream_host(x, n_fft, hop, window, block, lookahead, form):
    spec = stft32(x, n_fft, hop, True, form)
    win = sref.windows(np.abs(spec), window, block, lookahead)
    y = apply_map(win)
    m = sref.join(y, spec.shape[0], window, block, lookahead).astype(np.float32)
    return win, y, spec, istft32(rephase32(m, spec), hop, len(x), form)


def _denoise_ratios(n_fft, what):
    worst = dict.fromkeys(FORMS, 0.0)
    for w, v, hop, length in denoise_cases(n_fft):
        x = audio(n_fft, hop, length)
        for c in range(N_CLIPS):
            spec64, fscale = dref.stft(x[c], n_fft, hop), forward_scale(x[c], n_fft, hop)
            for form in FORMS:
                win, y, spec, out = denoise_host(x[c], n_fft, hop, w, v, form)
                if what == "windows":
                    want = dref.windows(np.abs(spec64), w, v)
                    r = ratio(win.astype(np.float64) - want, windows_scale(fscale, want.shape, denoise_first(len(fscale), w, v)))
                else:
                    y64, s64 = y.astype(np.float64), spec.astype(np.complex128)
                    hat = dref.rephase(dref.stitch(y64, s64.shape[0], w, v, clamp=True), s64)
                    r = ratio(out.astype(np.float64) - dref.istft(hat, hop, length), inverse_scale(hat, hop, length))
                worst[form] = max(worst[form], r)
    return worst


def _stream_ratios(n_fft, what):
    """The stream's audio is measured against the restatement fed the float64 STFT of the signal -- the stream keeps its spectrum
    to itself -- so the phase error of the forward transform is part of this floor, as it is of the device's error."""
    worst = dict.fromkeys(FORMS, 0.0)
    for w, b, a, hop, length in stream_cases(n_fft):
        x = audio(n_fft, hop, length)
        for c in range(N_CLIPS):
            spec64, fscale = dref.stft(x[c], n_fft, hop), forward_scale(x[c], n_fft, hop)
            for form in FORMS:
                win, y, _, out = stream_host(x[c], n_fft, hop, w, b, a, form)
                if what == "windows":
                    want = sref.windows(np.abs(spec64), w, b, a)
                    r = ratio(win.astype(np.float64) - want, windows_scale(fscale, want.shape, stream_first(len(fscale), w, b, a)))
                else:
                    hat = dref.rephase(sref.join(y.astype(np.float64), spec64.shape[0], w, b, a), spec64)
                    r = ratio(out.astype(np.float64) - dref.istft(hat, hop, length), inverse_scale(hat, hop, length))
                worst[form] = max(worst[form], r)
    return worst


@functools.lru_cache(maxsize=None)
def floors(entry, n_fft):
    """-> ((form, worst |host32 - ref64| / scale), ...) over all of this file's cases of `entry` at `n_fft`."""
    worst = dict.fromkeys(FORMS, 0.0)
    if entry == "stft_magnitude":
        for center in (True, False):
            for form, r, _ in _forward_ratios(n_fft, center):
                worst[form] = max(worst[form], r)
    elif entry == "stft_complex":
        worst = {form: r for form, _, r in _forward_ratios(n_fft, True)}
    elif entry == "istft":
        for hop, t in istft_cases(n_fft):
            z = spectra(n_fft, hop, t)
            for c in range(N_CLIPS):
                z64 = z[c].astype(np.complex128)
                ref, scale = istft64(z64, hop), inverse_scale(z64, hop, hop * (t - 1))
                for form in FORMS:
                    worst[form] = max(worst[form], ratio(istft32(z[c], hop, hop * (t - 1), form).astype(np.float64) - ref, scale))
    elif entry == "griffin_lim":
        for hop, t in gl_cases(n_fft):
            mag, rnd = gl_input(n_fft, hop, t)
            for c in range(N_CLIPS):
                hat = polar64(mag[c], rnd[c])
                ref, scale = istft64(hat, hop), inverse_scale(hat, hop, hop * (t - 1))
                for form in FORMS:
                    got = istft32(polar32(mag[c], rnd[c]), hop, hop * (t - 1), form)
                    worst[form] = max(worst[form], ratio(got.astype(np.float64) - ref, scale))
    elif entry in ("denoise_windows", "denoise_resynth"):
        worst = _denoise_ratios(n_fft, entry.split("_")[1])
    elif entry in ("stream_windows", "stream_audio"):
        worst = _stream_ratios(n_fft, entry.split("_")[1])
    else:
        raise KeyError(entry)
    return tuple(worst.items())


def floor(entry, n_fft):
    return max(r for _, r in floors(entry, n_fft))


def check(got, ref, scale, entry, n_fft, what, failures):
    """The device bound: |got - ref| <= MARGIN floor(entry, n_fft) scale element by element, exactly zero where the scale is zero.
    -> the largest share of the bound used.  A miss is appended to `failures` with its worst element, so that a test can walk all
    of its cases, print every share and assert at the end."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err, scale = np.broadcast_arrays(np.abs(got - ref), scale)
    zero = scale == 0
    if not np.all(got[zero] == 0):
        failures.append(f"{entry} n_fft {n_fft} {what}: {int((got[zero] != 0).sum())} values are not zero where the exact result is zero")
    if zero.all():
        return 0.0
    part = np.where(zero, 0.0, err / np.where(zero, 1.0, MARGIN * floor(entry, n_fft) * scale))
    share = float(part.max())
    if not share <= 1.0:
        at = np.unravel_index(np.argmax(np.where(np.isnan(part), np.inf, part)), part.shape)
        failures.append(f"{entry} n_fft {n_fft} {what}: {share:.3f} of the bound at index {tuple(int(i) for i in at)} "
                        f"(error {err[at]:.3g}, scale {scale[at]:.3g}, floor {floor(entry, n_fft):.3g})")
    return share
