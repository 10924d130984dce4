"""numpy restatement of the streaming dereverberator of include/adn.h ("dereverb stream") -- TEST INFRASTRUCTURE, written from the
header text.  float64 is the reference; dtype=np.float32 carries every statement out in float32 (every sum term by term in the
header's order), which is how the float32 host floors FLOOR and FLOOR_AUDIO below were measured (python
tests/dereverb_stream_cases.py).  That float32 form rounds every product (numpy's complex64 arithmetic: arithmetic="plain"); with
arithmetic="fma" the multiply-adds are the header's, two fmaf per component in its pairing and order (`fma`, `cfma`, `cfma_conj`
below), and tests/recursive_bounds.py takes a case's floor over both.  Vectorised over bins; spectrograms are frame-major (T, F) like the device's; the end-to-end form
is built on tests/denoise_ref.py's stft / istft / rephase and on tests/baseline_ref.py's gain."""
import numpy as np

import baseline_ref
import denoise_ref

DEFAULTS = dict(taps=20, delay=3, forget=0.99, loading=300.0, power_floor=0.01, smooth=0.9)
FIELDS = ("taps", "delay", "forget", "loading", "power_floor", "smooth")

# The float32 host floors: the worst max|d32 - d64| / max|d64| per row over the GPU parity cases of tests/dereverb_stream_cases.py
# (FLOOR: the spectrum d of wpe_online; FLOOR_AUDIO: the audio of the end-to-end stream form), measured on the host from this
# restatement (never from the device) and written here by `python tests/dereverb_stream_cases.py`.
FLOOR = 2.9e-06
FLOOR_AUDIO = 2.1e-06


def check_params(p):
    """The legal ranges of the header; ValueError (naming the field) outside them.  A NaN fails every comparison."""
    for name, lo, hi in (("taps", 1, 32), ("delay", 1, 8)):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(name)
    if not 0.95 <= np.float32(p["forget"]) <= 1.0:
        raise ValueError("forget")
    if not 1.0 <= p["loading"] <= 1e6:
        raise ValueError("loading")
    if not 0.0 < p["power_floor"] <= 1.0:
        raise ValueError("power_floor")
    if not 0.0 <= p["smooth"] < 1.0 or not np.float32(p["smooth"]) < 1.0:
        raise ValueError("smooth")


def _max(x, c):
    """max(x, c) of the header: x < c ? c : x -- a NaN x stays NaN."""
    return np.where(x < c, c, x)


def _power(z, dt):
    """fmaf(re, re, im * im) in `dt` (in float32 through float64, as tests/baseline_ref.py does)."""
    if dt is np.float32:
        im2 = (z.imag * z.imag).astype(np.float32)
        return (z.real.astype(np.float64) * z.real.astype(np.float64) + im2.astype(np.float64)).astype(np.float32)
    return z.real * z.real + z.imag * z.imag


ARITHMETICS = ("plain", "fma")


def fma(a, b, c):
    """fmaf(a, b, c) of float32 arrays as float32(float64(a) * float64(b) + float64(c)): the product is exact in float64, the sum
    rounds once there and once to float32 (the device of tests/baseline_ref.py for fmaf(re, re, im * im))."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def cx(re, im):
    """complex64 from its two float32 components, neither touched by an arithmetic operation."""
    out = np.empty(np.broadcast(re, im).shape, np.complex64)
    out.real, out.imag = re, im
    return out


def cfma(a, b, acc):
    """acc + a b as the header pairs it: two fmaf per component, the real-part product first."""
    return cx(fma(-a.imag, b.imag, fma(a.real, b.real, acc.real)), fma(a.imag, b.real, fma(a.real, b.imag, acc.imag)))


def cfma_conj(a, b, acc):
    """acc + a conj(b), likewise."""
    return cx(fma(a.imag, b.imag, fma(a.real, b.real, acc.real)), fma(a.imag, b.real, fma(-a.real, b.imag, acc.imag)))


def wpe_online(spec, params=None, dtype=np.float64, state=None, first_frame=0, with_state=False, with_lam=False, arithmetic="plain"):
    """spec (T, F) complex, the frames first_frame ... first_frame + T - 1 of every row -> d (T, F) complex in `dtype`'s precision.
    `state` is what an earlier call returned (with_state=True) for the frames before first_frame; first_frame = 0 starts fresh
    whatever `state` holds.  with_state: also the state after the last frame, a dict g (F, K), P (F, K, K), s (F,), past
    (F, D + K - 1) = the last raw frames, oldest first.  with_lam: also lam (T, F).
    arithmetic (float32 only): "plain" rounds every product and every sum (numpy's complex64 arithmetic, what FLOOR was measured
    with); "fma" follows the header's "Arithmetic" paragraph statement for statement: every complex multiply-add as two fmaf per
    component in its pairing and order, the divisions by den and by alpha componentwise and correctly rounded."""
    p = dict(DEFAULTS)
    p.update(params or {})
    check_params(p)
    dt = np.dtype(dtype).type
    assert arithmetic in ARITHMETICS and (arithmetic == "plain" or dt is np.float32)
    fused = arithmetic == "fma"
    ct = np.complex64 if dt is np.float32 else np.complex128
    K, D = int(p["taps"]), int(p["delay"])
    alpha, delta, rho, beta = (dt(np.float32(p[name])) for name in ("forget", "loading", "power_floor", "smooth"))
    # the two derived constants are computed once, in fp32, as the header says
    one_minus_beta = dt(np.float32(1.0) - np.float32(p["smooth"]))
    p0 = dt(np.float32(1.0) / np.float32(p["loading"]))
    tiny = dt(1e-30)
    X = np.asarray(spec).astype(ct)
    T, F = X.shape
    H = D + K - 1
    if first_frame == 0:
        g = np.zeros((F, K), ct)
        P = np.zeros((F, K, K), ct)
        P[:, np.arange(K), np.arange(K)] = p0
        s = np.zeros(F, dt)
        past = np.zeros((F, H), ct)
    else:
        g, P, s, past = (np.array(state[name]) for name in ("g", "P", "s", "past"))
        assert g.dtype == ct and past.shape == (F, H)
    full = np.concatenate([past, X.T], axis=1)                   # (F, H + T): frame t of the call at column H + t
    d = np.empty((T, F), ct)
    lams = np.empty((T, F), dt)
    low = np.tril(np.ones((K, K), bool))
    with np.errstate(all="ignore"):
        for t in range(T):
            x = full[:, H + t]
            pw = _power(x, dt)
            s = pw if first_frame + t == 0 else (beta * s + one_minus_beta * pw).astype(dt)
            phi = _max(rho * s, tiny)
            xt = full[:, H + t - D - K + 1:H + t - D + 1][:, ::-1]  # (F, K): column j = X_{t-D-j}
            if fused:                                            # term by term, in the header's order and pairing
                pred = np.zeros(F, ct)
                for j in range(K):
                    pred = cfma_conj(xt[:, j], g[:, j], pred)
                e = cx(x.real - pred.real, x.imag - pred.imag)
                u = np.zeros((F, K), ct)
                for k in range(K):
                    u = cfma(P[:, :, k], xt[:, k, None], u)
                q = np.zeros(F, dt)
                for j in range(K):
                    q = fma(xt[:, j].imag, u[:, j].imag, fma(xt[:, j].real, u[:, j].real, q))
            elif dt is np.float32:                               # term by term, in the header's order
                pred = np.zeros(F, ct)
                for j in range(K):
                    pred = pred + np.conj(g[:, j]) * xt[:, j]
                e = x - pred
                u = np.zeros((F, K), ct)
                for k in range(K):
                    u = u + P[:, :, k] * xt[:, k, None]
                q = np.zeros(F, dt)
                for j in range(K):
                    q = q + (np.conj(xt[:, j]) * u[:, j]).real
            else:
                e = x - np.einsum("fj,fj->f", np.conj(g), xt)
                u = np.einsum("fjk,fk->fj", P, xt)
                q = np.einsum("fj,fj->f", np.conj(xt), u).real
            e = e.astype(ct)
            lam = _max(_power(e, dt), phi)
            den = (alpha * lam + q).astype(dt)
            if fused:
                kk = cx(u.real / den[:, None], u.imag / den[:, None])
                Pn = cfma_conj(-kk[:, :, None], u[:, None, :], P)
                Pn = cx(Pn.real / alpha, Pn.imag / alpha)
            else:
                kk = (u / den[:, None]).astype(ct)
                Pn = ((P - kk[:, :, None] * np.conj(u)[:, None, :]) / alpha).astype(ct)
            Pn = np.where(low, Pn, np.conj(np.swapaxes(Pn, 1, 2)))           # the upper triangle is the lower one's conjugate
            idx = np.arange(K)
            Pn[:, idx, idx] = Pn[:, idx, idx].real
            P = Pn
            g = cfma_conj(kk, e[:, None], g) if fused else (g + kk * np.conj(e)[:, None]).astype(ct)
            d[t] = e
            lams[t] = lam
    out = [d]
    if with_state:
        out.append(dict(g=g, P=P, s=np.asarray(s, dt), past=np.ascontiguousarray(full[:, T:])))
    if with_lam:
        out.append(lams)
    return out[0] if len(out) == 1 else tuple(out)


def magnitude(d, dtype=np.float64):
    """M_t = sqrtf(fmaf(re, re, im * im)) of d (T, F) -> (F, T), the network-output layout."""
    dt = np.dtype(dtype).type
    return np.sqrt(_power(d, dt)).astype(dt).T


def _fft32(a):
    """The DFT along the last axis (a power of two) carried out in complex64: iterative radix-2, decimation in time, the twiddles
    computed in float64 and rounded once -- a float32 transform's rounding, which numpy.fft (float64 inside) does not have."""
    a = np.asarray(a, np.complex64)
    n = a.shape[-1]
    bits = n.bit_length() - 1
    assert n == 1 << bits
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)]) if bits else np.zeros(1, int)
    a = a[..., rev].copy()
    half = 1
    while half < n:
        w = np.exp(-1j * np.pi * np.arange(half) / half).astype(np.complex64)
        a = a.reshape(a.shape[:-1] + (n // (2 * half), 2, half))
        lo, hi = a[..., 0, :], (a[..., 1, :] * w).astype(np.complex64)
        a = np.stack([lo + hi, lo - hi], axis=-2).astype(np.complex64).reshape(a.shape[:-3] + (n,))
        half *= 2
    return a


def stft32(x, n_fft, hop):
    """denoise_ref.stft with every statement in float32: (L,) -> (T, F) complex64."""
    xp = np.pad(np.asarray(x, np.float32), n_fft // 2)
    idx = hop * np.arange(1 + len(x) // hop)[:, None] + np.arange(n_fft)[None, :]
    frames = (denoise_ref.hann(n_fft).astype(np.float32) * xp[idx]).astype(np.float32)
    return _fft32(frames)[:, :n_fft // 2 + 1]


def istft32(spec, hop, length):
    """denoise_ref.istft with every statement in float32 (Im X[0] and Im X[n_fft/2] ignored, as irfft does; a sample is the sum
    of its frames in ascending frame order)."""
    spec = np.asarray(spec, np.complex64)
    n_frames, n_fft = spec.shape[0], 2 * (spec.shape[1] - 1)
    full = np.concatenate([spec, np.conj(spec[:, -2:0:-1])], axis=1)
    full[:, 0] = full[:, 0].real
    full[:, n_fft // 2] = full[:, n_fft // 2].real
    win = denoise_ref.hann(n_fft).astype(np.float32)
    frames = ((np.conj(_fft32(np.conj(full))).real.astype(np.float32) * np.float32(1.0 / n_fft)).astype(np.float32) * win).astype(np.float32)
    y = np.zeros(n_fft + hop * (n_frames - 1), np.float32)
    wss = np.zeros_like(y)
    for t in range(n_frames):
        y[t * hop:t * hop + n_fft] += frames[t]
        wss[t * hop:t * hop + n_fft] += win * win
    y = np.where(wss > np.finfo(np.float32).tiny, y / np.where(wss > 0, wss, np.float32(1.0)), y).astype(np.float32)
    return y[n_fft // 2:n_fft // 2 + length]


def stream_dereverb(x, n_fft=512, hop=128, params=None, gain=False, gain_params=None, dtype=np.float64):
    """End to end, what StreamDereverberator returns for the finished signal x: STFT, the recursion, M = |d| -- with gain=True the
    magnitude form of the spectral gain of "baseline" on M -- M with the phase of d, the inverse STFT of the input's length.  The
    cut into steps does not enter: a step only says when a frame is computed.  dtype=np.float32 carries EVERY statement out in
    float32, the two transforms included (stft32 / istft32 above)."""
    f32 = np.dtype(dtype) == np.float32
    spec = stft32(x, n_fft, hop) if f32 else denoise_ref.stft(x, n_fft, hop)
    d = wpe_online(spec, params, dtype=dtype)
    mag = magnitude(d, dtype)
    if gain:
        mag, _ = baseline_ref.spectral_gain(mag.T.astype(d.dtype), gain_params, dtype=dtype)
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(mag), mag, np.maximum(mag, 0)).astype(dtype)       # adn_stream_emit clamps what it reads
        if not f32:
            return denoise_ref.istft(denoise_ref.rephase(m, d), hop, len(x))
        size = magnitude(d, dtype).T                                             # rephase of "denoise", rule 5, in float32
        scale = (m.T / np.where(size > 0, size, np.float32(1.0))).astype(np.float32)
        s = np.where(size > 0, (d * scale).astype(np.complex64), (m.T + 0j).astype(np.complex64))
        return istft32(s, hop, len(x))


si_sdr = baseline_ref.si_sdr
