"""numpy restatement of the dereverberation baseline of include/adn.h ("dereverb") -- TEST INFRASTRUCTURE, written from the header
text.  float64 is the reference; dtype=np.float32 carries every statement out in float32, the Cholesky factorisation and the two
substitutions written out (no LAPACK), which is how the float32 host floor FLOOR below was measured (python
tests/dereverb_cases.py).  Vectorised over bins; spectrograms are frame-major (T, F) like the device's; the end-to-end forms are
built on tests/denoise_ref.py's stft / istft and on tests/baseline_ref.py's gain."""
import numpy as np

import baseline_ref
import denoise_ref

DEFAULTS = dict(taps=20, delay=3, iterations=3, loading=1e-3, power_floor=1e-3)
FIELDS = ("taps", "delay", "iterations", "loading", "power_floor")

# The float32 host floor: the worst max|d32 - d64| / max|d64| per clip over the GPU parity cases of tests/dereverb_cases.py,
# measured on the host from this restatement (never from the device) and written here by `python tests/dereverb_cases.py`.
FLOOR = 2.9e-04


def check_params(p):
    """The legal ranges of the header; ValueError (naming the field) outside them."""
    for name, lo, hi in (("taps", 1, 32), ("delay", 1, 8), ("iterations", 1, 8)):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(name)
    if not 1e-6 <= p["loading"] <= 1.0:
        raise ValueError("loading")
    if not 0.0 < p["power_floor"] <= 1.0:
        raise ValueError("power_floor")


def _max(x, c):
    """max(x, c) of the header: x < c ? c : x -- a NaN x stays NaN."""
    return np.where(x < c, c, x)


def _power(z, dt):
    """fmaf(re, re, im * im) in `dt` (in float32 through float64, as tests/baseline_ref.py does)."""
    if dt is np.float32:
        im2 = (z.imag * z.imag).astype(np.float32)
        return (z.real.astype(np.float64) * z.real.astype(np.float64) + im2.astype(np.float64)).astype(np.float32)
    return z.real * z.real + z.imag * z.imag


def _cholesky_solve(A, P):
    """A (F, K, K) Hermitian, P (F, K) -> g (F, K) in A's dtype: A = L L^H column by column, L y = P, L^H g = y, every inner sum
    over k in the header's order."""
    K = A.shape[1]
    L = np.zeros_like(A)
    real = A.real.dtype.type
    for c in range(K):
        s = A[:, c, c].real.copy()
        for k in range(c):
            s = s - L[:, c, k].real * L[:, c, k].real
            s = s - L[:, c, k].imag * L[:, c, k].imag
        lcc = np.sqrt(s).astype(real)
        L[:, c, c] = lcc
        if c + 1 < K:
            v = A[:, c + 1:, c].copy()
            for k in range(c):
                v = v - L[:, c + 1:, k] * np.conj(L[:, c, k])[:, None]
            L[:, c + 1:, c] = v / lcc[:, None]
    y = np.zeros_like(P)
    for r in range(K):
        v = P[:, r].copy()
        for k in range(r):
            v = v - L[:, r, k] * y[:, k]
        y[:, r] = v / L[:, r, r].real
    g = np.zeros_like(P)
    for r in range(K - 1, -1, -1):
        v = y[:, r].copy()
        for k in range(K - 1, r, -1):
            v = v - np.conj(L[:, k, r]) * g[:, k]
        g[:, r] = v / L[:, r, r].real
    return g


def _sum_t(x, dtype, order):
    """The sum over t (the last axis) in `dtype`: "pairwise" is numpy's sum of a contiguous row; "sequential" adds frame after frame
    from t = 0, the order include/adn.h states for the device (a cumulative sum is sequential in numpy)."""
    if order == "pairwise":
        return x.sum(axis=-1, dtype=dtype)
    if order == "sequential":
        return x.cumsum(axis=-1, dtype=dtype)[..., -1]
    raise ValueError("order")


def wpe(spec, params=None, dtype=np.float64, with_taps=False, order="pairwise"):
    """spec (T, F) complex -> d (T, F) complex in `dtype`'s precision (complex128 / complex64); with_taps: also g (F, K).
    order: how every sum over t is formed, "pairwise" (the reference, and what FLOOR was measured with) or "sequential"."""
    p = dict(DEFAULTS)
    p.update(params or {})
    check_params(p)
    dt = np.dtype(dtype).type
    ct = np.complex64 if dt is np.float32 else np.complex128
    K, D, I = int(p["taps"]), int(p["delay"]), int(p["iterations"])
    delta, rho = dt(np.float32(p["loading"])), dt(np.float32(p["power_floor"]))
    X = np.ascontiguousarray(np.asarray(spec).astype(ct).T)                       # (F, T): a row's frames are contiguous, so
    F, T = X.shape                                                                # every sum over t is numpy's pairwise sum of
    tiny = dt(1e-30)                                                              # one row, whatever the other rows are
    with np.errstate(all="ignore"):
        phi = _max(rho * _sum_t(_power(X, dt), dt, order) / dt(T), tiny)
        # past[j][:, t] = X_{t-D-j}, zero before frame 0
        past = np.zeros((K, F, T), ct)
        for j in range(K):
            if T > D + j:
                past[j, :, D + j:] = X[:, :T - D - j]
        d = X.copy()
        g = np.zeros((F, K), ct)
        for _ in range(I):
            w = (dt(1.0) / _max(_power(d, dt), phi[:, None])).astype(dt)          # (F, T)
            u = (past * w[None]).astype(ct)                                       # w_t X_{t-D-j}: each component rounded
            R = np.zeros((F, K, K), ct)
            P = np.zeros((F, K), ct)
            for j in range(K):
                for k in range(j + 1):
                    R[:, j, k] = _sum_t(u[j] * np.conj(past[k]), ct, order)
                    R[:, k, j] = np.conj(R[:, j, k])
                P[:, j] = _sum_t(u[j] * np.conj(X), ct, order)
            idx = np.arange(K)
            tr = np.zeros(F, dt)
            for j in range(K):
                tr = tr + R[:, j, j].real
            A = R.copy()
            A[:, idx, idx] = (R[:, idx, idx].real + ((delta * tr) / dt(K) + tiny)[:, None]).astype(dt)
            g = _cholesky_solve(A, P)
            d = X.copy()
            for j in range(K):
                d = d - np.conj(g[:, j])[:, None] * past[j]
            d = d.astype(ct)
            d[:, :D] = X[:, :D]                                                   # no tap has a frame there
    d = np.ascontiguousarray(d.T)
    return (d, g) if with_taps else d


def dereverb(x, n_fft=512, hop=128, params=None, gain=False, spec=None):
    """End to end in float64: STFT (or the given (T, F) spectrogram), WPE, optionally the spectral gain of "baseline" on the
    result, the phase of d, inverse STFT of the input's length."""
    if spec is None:
        spec = denoise_ref.stft(x, n_fft, hop)
    d = wpe(spec, params)
    if gain:
        mag, _ = baseline_ref.spectral_gain(d)
        d = denoise_ref.rephase(mag, d)
    return denoise_ref.istft(d, hop, len(x))


si_sdr = baseline_ref.si_sdr
