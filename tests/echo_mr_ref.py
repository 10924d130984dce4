"""numpy restatement of the multi-reference echo canceller of include/adn_call.h ("echo stream multireference") -- TEST
INFRASTRUCTURE, written from the header text: "echo stream" of include/adn_echo.h on the stacked vector x~_r = R_{t-D-j, q} at
r = q K + j.  float64 is the reference; dtype=np.float32 carries every statement out in float32, every sum term by term in the
header's order, in the two arithmetics of tests/dereverb_stream_ref.py ("plain" rounds every product, "fma" follows the header
statement for statement).  Vectorised over bins; spectrograms are frame-major: the microphone (T, F), the far end (Q, T, F).  With
Q = 1 every function here gives tests/echo_ref.py's bits (tests/test_echo_mr_host.py)."""
import numpy as np

import baseline_ref
import denoise_ref
from dereverb_stream_ref import ARITHMETICS, _power, cfma, cfma_conj, cx, fma, istft32, magnitude, stft32
from echo_ref import DEFAULTS as PARENT_DEFAULTS, FIELDS, check_params as check_parent_params

MAX_REFS, MAX_STACK = 8, 32


def defaults(refs):
    """The header's params = NULL: 8 taps for one reference, 16 / refs per channel for more; the other fields are the parent's."""
    return dict(PARENT_DEFAULTS, taps=8 if refs == 1 else 16 // refs)


def check_params(refs, p):
    """The legal ranges of the header; ValueError (naming the field) outside them."""
    if isinstance(refs, bool) or not isinstance(refs, (int, np.integer)) or not 1 <= refs <= MAX_REFS:
        raise ValueError("refs")
    check_parent_params(p)
    if refs * p["taps"] > MAX_STACK:
        raise ValueError("refs taps")
    if not 2.0 * refs * p["taps"] * (1.0 - float(np.float32(p["forget"]))) <= 1.0:
        raise ValueError("forget (refs taps)")


def _stack(full, at, K, D):
    """full (Q, F, H + T), far-end frame t of the call at column H + t -> x~ (F, Q K): column q K + j = R_{t-D-j, q}."""
    H = D + K - 1
    return np.concatenate([ch[:, H + at - D - K + 1:H + at - D + 1][:, ::-1] for ch in full], axis=1)


def aec_mr_online(mic, far, params=None, dtype=np.float64, arithmetic="plain", state=None, first_frame=0, with_state=False):
    """mic (T, F), far (Q, T, F) complex, the frames first_frame ... first_frame + T - 1 of a group -> e (T, F) complex in `dtype`'s
    precision.  `state` is what an earlier call returned (with_state=True) for the frames before first_frame; first_frame = 0 starts
    fresh whatever `state` holds.  with_state: also the state after the last frame, a dict h (F, N), P (F, N, N), past (Q, F, D + K -
    1) = the last far-end frames of every channel, oldest first.  arithmetic (float32 only): see the module text."""
    far = np.asarray(far)
    assert far.ndim == 3
    Q = far.shape[0]
    p = defaults(Q)
    p.update(params or {})
    check_params(Q, p)
    dt = np.dtype(dtype).type
    assert arithmetic in ARITHMETICS and (arithmetic == "plain" or dt is np.float32)
    fused = arithmetic == "fma"
    ct = np.complex64 if dt is np.float32 else np.complex128
    K, D = int(p["taps"]), int(p["delay"])
    N = Q * K
    alpha, quiet = dt(np.float32(p["forget"])), dt(np.float32(p["quiet"]))
    p0 = dt(np.float32(1.0) / np.float32(p["loading"]))              # once, in fp32, as the header says
    Y, R = np.asarray(mic).astype(ct), far.astype(ct)
    assert Y.shape == R.shape[1:]
    T, F = Y.shape
    H = D + K - 1
    if first_frame == 0:
        h = np.zeros((F, N), ct)
        P = np.zeros((F, N, N), ct)
        P[:, np.arange(N), np.arange(N)] = p0
        past = np.zeros((Q, F, H), ct)
    else:
        h, P, past = (np.array(state[name]) for name in ("h", "P", "past"))
        assert h.dtype == ct and past.shape == (Q, F, H)
    full = np.concatenate([past, np.swapaxes(R, 1, 2)], axis=2)     # (Q, F, H + T)
    e_out = np.empty((T, F), ct)
    low = np.tril(np.ones((N, N), bool))
    idx = np.arange(N)
    with np.errstate(all="ignore"):
        for t in range(T):
            y = Y[t]
            xt = _stack(full, t, K, D)                               # (F, N)
            if dt is np.float32:                                     # term by term, in the header's order
                pred, r, u, q = np.zeros(F, ct), np.zeros(F, dt), np.zeros((F, N), ct), np.zeros(F, dt)
                for j in range(N):
                    pred = cfma_conj(xt[:, j], h[:, j], pred) if fused else pred + np.conj(h[:, j]) * xt[:, j]
                    r = (r + _power(xt[:, j], dt)).astype(dt)
                e = cx(y.real - pred.real, y.imag - pred.imag) if fused else y - pred
                for k in range(N):
                    u = cfma(P[:, :, k], xt[:, k, None], u) if fused else u + P[:, :, k] * xt[:, k, None]
                for j in range(N):
                    q = (fma(xt[:, j].imag, u[:, j].imag, fma(xt[:, j].real, u[:, j].real, q)) if fused
                         else q + (np.conj(xt[:, j]) * u[:, j]).real)
            else:
                e = y - np.einsum("fj,fj->f", np.conj(h), xt)
                r = np.einsum("fj,fj->f", np.conj(xt), xt).real
                u = np.einsum("fjk,fk->fj", P, xt)
                q = np.einsum("fj,fj->f", np.conj(xt), u).real
            e = e.astype(ct)
            adapt = ~(r <= quiet)                                    # a NaN r adapts; the gate is on the stacked power
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
        return e_out, dict(h=h, P=P, past=np.ascontiguousarray(full[:, :, T:]))
    return e_out


def normal_equations(mic, far, params=None):
    """h (F, N) in float64 solving (delta I + sum_t x~_t x~_t^H) h = sum_t x~_t conj(Y_t) over all frames: what aec_mr_online's h is
    after T frames at forget = 1 when no frame is gated.  delta = 1 / P_0, P_0 the fp32 quotient 1 / loading."""
    far = np.asarray(far, np.complex128)
    Q = far.shape[0]
    p = defaults(Q)
    p.update(params or {})
    K, D = int(p["taps"]), int(p["delay"])
    N = Q * K
    Y = np.asarray(mic, np.complex128)
    T, F = Y.shape
    H = D + K - 1
    full = np.concatenate([np.zeros((Q, F, H), np.complex128), np.swapaxes(far, 1, 2)], axis=2)
    delta = 1.0 / float(np.float32(1.0) / np.float32(p["loading"]))
    A = np.tile(delta * np.eye(N, dtype=np.complex128), (F, 1, 1))
    b = np.zeros((F, N), np.complex128)
    for t in range(T):
        xt = _stack(full, t, K, D)
        A += xt[:, :, None] * np.conj(xt)[:, None, :]
        b += xt * np.conj(Y[t])[:, None]
    return np.linalg.solve(A, b[:, :, None])[:, :, 0]


def echo_cancel(mic, far, n_fft=512, hop=128, params=None, gain=False, gain_params=None, dtype=np.float64, arithmetic="plain"):
    """End to end, what EchoCanceller(refs=Q).cancel and StreamEchoCanceller(refs=Q) return for the finished signals mic (L,) and far
    (Q, L) at the working rate: the STFT of all, the recursion, M = |e| -- with gain=True the magnitude form of the spectral gain of
    "baseline" on M -- M with the phase of e, the inverse STFT of the input's length (tests/echo_ref.py's chain)."""
    f32 = np.dtype(dtype) == np.float32
    tf = (lambda a: stft32(a, n_fft, hop)) if f32 else (lambda a: denoise_ref.stft(a, n_fft, hop))
    e = aec_mr_online(tf(mic), np.stack([tf(ch) for ch in far]), params, dtype=dtype, arithmetic=arithmetic)
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


__all__ = ["ARITHMETICS", "FIELDS", "MAX_REFS", "MAX_STACK", "defaults", "check_params", "aec_mr_online", "normal_equations", "echo_cancel"]
