"""numpy restatement of multichannel WPE as include/adn.h defines it ("dereverb multichannel") -- TEST INFRASTRUCTURE, written
from the header text on top of tests/dereverb_ref.py, whose `_cholesky_solve`, `_power` and `_max` it reuses: with one channel
every line below is that file's `wpe`.  float64 is the reference; dtype=np.float32 carries every statement out in float32, which
is how the float32 host floor FLOOR below was measured (python tests/dereverb_mc_cases.py).  Vectorised over bins; a group is
(C, T, F), frame-major like the device's."""
import numpy as np

import baseline_ref
import denoise_ref
import dereverb_ref as dr

MAX_CHANNELS = 8
MAX_STACKED = 32

# The float32 host floor: the worst max|d32 - d64| / max|d64| per group over the GPU parity cases of tests/dereverb_mc_cases.py,
# measured on the host from this restatement (never from the device) and written here by `python tests/dereverb_mc_cases.py`.
# The one case at loading 1e-6 sets it: two microphones of one source make R nearly singular, and only the loading conditions it.
# FLOOR_DEFAULT_LOADING is the same figure over the cases at the default loading alone, 140 times smaller; the device test holds
# those cases to it, so that the weak-loading case does not loosen every other bound.
FLOOR = 9.6e-03
FLOOR_DEFAULT_LOADING = 6.8e-05


def defaults(channels):
    """The parameters of a NULL `params`: those of "dereverb" with taps = 32 / C."""
    return dict(dr.DEFAULTS, taps=MAX_STACKED // channels)


def check_params(p, channels):
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("channels")
    dr.check_params(p)
    if channels * p["taps"] > MAX_STACKED:
        raise ValueError("channels * taps")


def wpe_mc(specs, params=None, dtype=np.float64, with_taps=False, order="pairwise", slip=None):
    """specs (C, T, F) complex -> d (C, T, F) complex in `dtype`'s precision; with_taps: also G (F, N, C).  order: how every sum
    over t is formed, as in dereverb_ref.wpe.  slip: None, or `slip(R, P) -> (R, P)` applied to every iteration's correlations
    before the solve -- the mutations of tests/test_solver_bounds_host.py, never a reference."""
    specs = np.asarray(specs)
    C = specs.shape[0]
    p = defaults(C) if 1 <= C <= MAX_CHANNELS else dict(dr.DEFAULTS)
    p.update(params or {})
    check_params(p, C)
    dt = np.dtype(dtype).type
    ct = np.complex64 if dt is np.float32 else np.complex128
    K, D, I = int(p["taps"]), int(p["delay"]), int(p["iterations"])
    N = C * K
    delta, rho = dt(np.float32(p["loading"])), dt(np.float32(p["power_floor"]))
    X = np.ascontiguousarray(specs.astype(ct).transpose(0, 2, 1))                 # (C, F, T): a row's frames are contiguous
    _, F, T = X.shape
    tiny = dt(1e-30)
    with np.errstate(all="ignore"):
        total = np.zeros(F, dt)
        for c in range(C):                                                        # channels ascending
            total = total + dr._sum_t(dr._power(X[c], dt), dt, order)
        phi = dr._max(rho * total / dt(T * C), tiny)
        # past[c K + j][:, t] = X_{t-D-j, c}, zero before frame 0: the stacked vector, channel-major, the lag ascending
        past = np.zeros((N, F, T), ct)
        for c in range(C):
            for j in range(K):
                if T > D + j:
                    past[c * K + j, :, D + j:] = X[c, :, :T - D - j]
        d = X.copy()
        G = np.zeros((F, N, C), ct)
        idx = np.arange(N)
        for _ in range(I):
            s = dr._power(d[0], dt)
            for c in range(1, C):
                s = s + dr._power(d[c], dt)
            w = (dt(1.0) / dr._max(s / dt(C), phi[:, None])).astype(dt)          # (F, T), one variance for all channels
            u = (past * w[None]).astype(ct)                                       # w_t x~_t[r]: each component rounded
            R = np.zeros((F, N, N), ct)
            P = np.zeros((F, N, C), ct)
            for r in range(N):
                for q in range(r + 1):
                    R[:, r, q] = dr._sum_t(u[r] * np.conj(past[q]), ct, order)
                    R[:, q, r] = np.conj(R[:, r, q])
                for c in range(C):
                    P[:, r, c] = dr._sum_t(u[r] * np.conj(X[c]), ct, order)
            if slip is not None:
                R, P = slip(R, P)
            tr = np.zeros(F, dt)
            for r in range(N):
                tr = tr + R[:, r, r].real
            A = R.copy()
            A[:, idx, idx] = (R[:, idx, idx].real + ((delta * tr) / dt(N) + tiny)[:, None]).astype(dt)
            for c in range(C):                                                    # one A: the factor is the same for every column
                G[:, :, c] = dr._cholesky_solve(A, np.ascontiguousarray(P[:, :, c]))
            d = X.copy()
            for c in range(C):
                for r in range(N):
                    d[c] = d[c] - np.conj(G[:, r, c])[:, None] * past[r]
            d = d.astype(ct)
            d[:, :, :D] = X[:, :, :D]                                             # no entry has a frame there
    d = np.ascontiguousarray(d.transpose(0, 2, 1))
    return (d, G) if with_taps else d


def dereverb_mc(x, n_fft=512, hop=128, params=None, gain=False, specs=None):
    """End to end in float64: x (C, L) -> (C, L).  The STFT of every channel (or the given (C, T, F) spectrograms), joint WPE,
    optionally the spectral gain of "baseline" per channel on the result, the phase of d, the inverse STFT of the input's length."""
    x = np.asarray(x)
    if specs is None:
        specs = np.stack([denoise_ref.stft(row, n_fft, hop) for row in x])
    d = wpe_mc(specs, params)
    out = []
    for c in range(d.shape[0]):
        dc = d[c]
        if gain:
            mag, _ = baseline_ref.spectral_gain(dc)
            dc = denoise_ref.rephase(mag, dc)
        out.append(denoise_ref.istft(dc, hop, x.shape[1]))
    return np.stack(out)


si_sdr = baseline_ref.si_sdr
