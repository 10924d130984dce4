"""numpy restatement of the echo canceller of include/adn_echo.h ("echo stream") -- TEST INFRASTRUCTURE, written from the header text.
float64 is the reference; dtype=np.float32 carries every statement out in float32, every sum term by term in the header's order, in
the two arithmetics of tests/dereverb_stream_ref.py: "plain" rounds every product (numpy's complex64 arithmetic), "fma" follows the
header statement for statement (two fmaf per component in its pairing and order, componentwise correctly rounded divisions).
Vectorised over bins; spectrograms are frame-major (T, F) like the device's; the end-to-end form is built on tests/denoise_ref.py's
stft / istft / rephase and on tests/baseline_ref.py's gain, as dereverb_stream_ref.stream_dereverb is."""
import numpy as np

import baseline_ref
import denoise_ref
from dereverb_stream_ref import ARITHMETICS, _power, cfma, cfma_conj, cx, fma, istft32, magnitude, stft32

DEFAULTS = dict(taps=8, delay=0, forget=0.995, loading=10.0, quiet=1e-8)
FIELDS = ("taps", "delay", "forget", "loading", "quiet")


def check_params(p):
    """The legal ranges of the header; ValueError (naming the field) outside them.  A NaN fails every comparison."""
    for name, lo, hi in (("taps", 1, 32), ("delay", 0, 8)):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(name)
    if not np.float32(0.95) <= np.float32(p["forget"]) <= 1.0:
        raise ValueError("forget")
    if not np.float32(1e-3) <= np.float32(p["loading"]) <= 1e6:
        raise ValueError("loading")
    if not 0.0 <= np.float32(p["quiet"]) <= 1.0:
        raise ValueError("quiet")
    if not 2.0 * p["taps"] * (1.0 - float(np.float32(p["forget"]))) <= 1.0:
        raise ValueError("forget")


def aec_online(mic, far, params=None, dtype=np.float64, arithmetic="plain", state=None, first_frame=0, with_state=False):
    """mic, far (T, F) complex, the frames first_frame ... first_frame + T - 1 of a row -> e (T, F) complex in `dtype`'s precision.
    `state` is what an earlier call returned (with_state=True) for the frames before first_frame; first_frame = 0 starts fresh
    whatever `state` holds.  with_state: also the state after the last frame, a dict h (F, K), P (F, K, K), past (F, D + K - 1) =
    the last far-end frames, oldest first.  arithmetic (float32 only): see the module text."""
    p = dict(DEFAULTS)
    p.update(params or {})
    check_params(p)
    dt = np.dtype(dtype).type
    assert arithmetic in ARITHMETICS and (arithmetic == "plain" or dt is np.float32)
    fused = arithmetic == "fma"
    ct = np.complex64 if dt is np.float32 else np.complex128
    K, D = int(p["taps"]), int(p["delay"])
    alpha, quiet = dt(np.float32(p["forget"])), dt(np.float32(p["quiet"]))
    p0 = dt(np.float32(1.0) / np.float32(p["loading"]))              # once, in fp32, as the header says
    Y, R = np.asarray(mic).astype(ct), np.asarray(far).astype(ct)
    assert Y.shape == R.shape
    T, F = Y.shape
    H = D + K - 1
    if first_frame == 0:
        h = np.zeros((F, K), ct)
        P = np.zeros((F, K, K), ct)
        P[:, np.arange(K), np.arange(K)] = p0
        past = np.zeros((F, H), ct)
    else:
        h, P, past = (np.array(state[name]) for name in ("h", "P", "past"))
        assert h.dtype == ct and past.shape == (F, H)
    full = np.concatenate([past, R.T], axis=1)                       # (F, H + T): far-end frame t of the call at column H + t
    e_out = np.empty((T, F), ct)
    low = np.tril(np.ones((K, K), bool))
    idx = np.arange(K)
    with np.errstate(all="ignore"):
        for t in range(T):
            y = Y[t]
            xt = full[:, H + t - D - K + 1:H + t - D + 1][:, ::-1]  # (F, K): column j = R_{t-D-j}
            if dt is np.float32:                                     # term by term, in the header's order
                pred, r, u, q = np.zeros(F, ct), np.zeros(F, dt), np.zeros((F, K), ct), np.zeros(F, dt)
                for j in range(K):
                    pred = cfma_conj(xt[:, j], h[:, j], pred) if fused else pred + np.conj(h[:, j]) * xt[:, j]
                    r = (r + _power(xt[:, j], dt)).astype(dt)
                e = cx(y.real - pred.real, y.imag - pred.imag) if fused else y - pred
                for k in range(K):
                    u = cfma(P[:, :, k], xt[:, k, None], u) if fused else u + P[:, :, k] * xt[:, k, None]
                for j in range(K):
                    q = (fma(xt[:, j].imag, u[:, j].imag, fma(xt[:, j].real, u[:, j].real, q)) if fused
                         else q + (np.conj(xt[:, j]) * u[:, j]).real)
            else:
                e = y - np.einsum("fj,fj->f", np.conj(h), xt)
                r = np.einsum("fj,fj->f", np.conj(xt), xt).real
                u = np.einsum("fjk,fk->fj", P, xt)
                q = np.einsum("fj,fj->f", np.conj(xt), u).real
            e = e.astype(ct)
            adapt = ~(r <= quiet)                                    # a NaN r adapts
            den = (alpha + q).astype(dt)
            if fused:
                kk = cx(u.real / den[:, None], u.imag / den[:, None])
                Pn = cfma_conj(-kk[:, :, None], u[:, None, :], P)
                Pn = cx(Pn.real / alpha, Pn.imag / alpha)
                hn = cfma_conj(kk, e[:, None], h)
            else:
                kk = (u / den[:, None]).astype(ct)
                Pn = ((P - kk[:, :, None] * np.conj(u)[:, None, :]) / alpha).astype(ct)
                hn = (h + kk * np.conj(e)[:, None]).astype(ct)
            Pn = np.where(low, Pn, np.conj(np.swapaxes(Pn, 1, 2)))   # the upper triangle is the lower one's conjugate
            Pn[:, idx, idx] = Pn[:, idx, idx].real
            P = np.where(adapt[:, None, None], Pn, P)                # the gate: a quiet frame leaves P and h as they are
            h = np.where(adapt[:, None], hn, h)
            e_out[t] = e
    if with_state:
        return e_out, dict(h=h, P=P, past=np.ascontiguousarray(full[:, T:]))
    return e_out


def normal_equations(mic, far, params=None):
    """h (F, K) in float64 solving (delta I + sum_t x~_t x~_t^H) h = sum_t x~_t conj(Y_t) over all frames of (T, F) spectrograms:
    what aec_online's h is after T frames at forget = 1 when no frame is gated.  delta is the one the recursion starts from: P_0 is
    the fp32 quotient 1 / loading (once per call, the header), so delta = 1 / P_0, which differs from `loading` by up to 2^-24."""
    p = dict(DEFAULTS)
    p.update(params or {})
    K, D = int(p["taps"]), int(p["delay"])
    Y, R = np.asarray(mic, np.complex128), np.asarray(far, np.complex128)
    T, F = Y.shape
    H = D + K - 1
    full = np.concatenate([np.zeros((F, H), np.complex128), R.T], axis=1)
    delta = 1.0 / float(np.float32(1.0) / np.float32(p["loading"]))
    A = np.tile(delta * np.eye(K, dtype=np.complex128), (F, 1, 1))
    b = np.zeros((F, K), np.complex128)
    for t in range(T):
        xt = full[:, H + t - D - K + 1:H + t - D + 1][:, ::-1]
        A += xt[:, :, None] * np.conj(xt)[:, None, :]
        b += xt * np.conj(Y[t])[:, None]
    return np.linalg.solve(A, b[:, :, None])[:, :, 0]


def echo_cancel(mic, far, n_fft=512, hop=128, params=None, gain=False, gain_params=None, dtype=np.float64, arithmetic="plain"):
    """End to end, what EchoCanceller.cancel and StreamEchoCanceller return for the finished signals mic and far at the working
    rate: the STFT of both, the recursion, M = |e| -- with gain=True the magnitude form of the spectral gain of "baseline" on M -- M
    with the phase of e, the inverse STFT of the input's length.  dtype=np.float32 carries EVERY statement out in float32, the
    transforms included."""
    f32 = np.dtype(dtype) == np.float32
    tf = (lambda a: stft32(a, n_fft, hop)) if f32 else (lambda a: denoise_ref.stft(a, n_fft, hop))
    e = aec_online(tf(mic), tf(far), params, dtype=dtype, arithmetic=arithmetic)
    mag = magnitude(e, dtype)
    if gain:
        mag, _ = baseline_ref.spectral_gain(mag.T.astype(e.dtype), gain_params, dtype=dtype)
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(mag), mag, np.maximum(mag, 0)).astype(dtype)       # the resynthesis clamps what it reads
        if not f32:
            return denoise_ref.istft(denoise_ref.rephase(m, e), hop, len(mic))
        size = magnitude(e, dtype).T
        scale = (m.T / np.where(size > 0, size, np.float32(1.0))).astype(np.float32)
        s = np.where(size > 0, (e * scale).astype(np.complex64), (m.T + 0j).astype(np.complex64))
        return istft32(s, hop, len(mic))
