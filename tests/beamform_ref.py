"""numpy restatement of the mask-driven MVDR beamformer as include/adn.h defines it ("beamform") -- TEST INFRASTRUCTURE, written from
the header text on top of tests/dereverb_ref.py, whose `_cholesky_solve`, `_power` and `_max` it reuses.  float64 is the
reference; dtype=np.float32 carries every statement out in float32, which is how the float32 host floor FLOOR below was measured
(python tests/beamform_cases.py).  Vectorised over bins; a group is (C, T, F), frame-major like the device's, its mask magnitudes
(C, F, width) with the frame fastest, like the device's."""
import numpy as np

import baseline_ref
import denoise_ref
import dereverb_mc_ref
import dereverb_ref as dr

MAX_CHANNELS = 8
DEFAULTS = dict(ref_channel=0, loading=1e-3, mask_floor=1e-3)
FIELDS = ("ref_channel", "loading", "mask_floor")

# The float32 host floor: the worst max|Y32 - Y64| / max|Y64| per group over the GPU parity cases of tests/beamform_cases.py,
# measured on the host from this restatement (never from the device) and written here by `python tests/beamform_cases.py`.
# The cases with fewer frames than channels set it: their covariances have rank T < C, and only the loading conditions the solve.
# FLOOR_FULL_RANK is the same figure over the cases with T >= C at the default loading; the device test holds those cases to it, so
# that the rank-deficient cases and the one at loading 1e-6 do not loosen every other bound.
FLOOR = 3.1e-04
FLOOR_FULL_RANK = 4.9e-05


def check_params(p, channels):
    """The legal ranges of the header; ValueError (naming the field) outside them."""
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("channels")
    r = p["ref_channel"]
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r < channels:
        raise ValueError("ref_channel")
    if not 1e-6 <= p["loading"] <= 1.0:
        raise ValueError("loading")
    if not 1e-6 <= p["mask_floor"] <= 0.25:
        raise ValueError("mask_floor")


def _min(x, c):
    """min(x, c) of the header: x > c ? c : x -- a NaN x stays NaN."""
    return np.where(x > c, c, x)


def _weighted(z, w, ct):
    """w z with each component rounded: (w re, w im)."""
    out = np.empty(z.shape, ct)
    out.real = z.real * w
    out.imag = z.imag * w
    return out


def mask(specs, mags, rho, dtype=np.float64):
    """specs (C, T, F) complex, mags (C, F, >= T) -> m (F, T) in `dtype`: s_t / q_t inside [rho, 1 - rho], rho where q_t = 0."""
    dt = np.dtype(dtype).type
    ct = np.complex64 if dt is np.float32 else np.complex128
    X = np.asarray(specs).astype(ct).transpose(0, 2, 1)
    C, F, T = X.shape
    M = np.asarray(mags)[:, :, :T].astype(dt)
    rho = dt(np.float32(rho))
    top = dt(np.float32(1.0) - np.float32(rho))                                   # 1 - rho, rounded once in fp32
    with np.errstate(all="ignore"):
        s, q = np.zeros((F, T), dt), np.zeros((F, T), dt)
        for c in range(C):                                                        # channels ascending
            s = s + (M[c] * M[c]).astype(dt)
            q = q + dr._power(X[c], dt)
        m = np.where(q > 0, _min(dr._max(s / q, rho), top), rho).astype(dt)
    return m


def mvdr(specs, mags, params=None, dtype=np.float64, with_filter=False, order="pairwise", slip=None):
    """specs (C, T, F) complex, mags (C, F, width >= T) real -> Y (T, F) complex in `dtype`'s precision; with_filter: also w (F, C).
    order: how the sums over t of both covariances are formed, as in dereverb_ref.wpe.  slip: None, or
    `slip(phi_s, phi_n) -> (phi_s, phi_n)` applied to the covariances before the solve -- the mutations of
    tests/test_solver_bounds_host.py, never a reference."""
    specs = np.asarray(specs)
    C = specs.shape[0]
    p = dict(DEFAULTS)
    p.update(params or {})
    check_params(p, C)
    dt = np.dtype(dtype).type
    ct = np.complex64 if dt is np.float32 else np.complex128
    ref = int(p["ref_channel"])
    delta = dt(np.float32(p["loading"]))
    X = np.ascontiguousarray(specs.astype(ct).transpose(0, 2, 1))                 # (C, F, T): a row's frames are contiguous
    _, F, T = X.shape
    tiny = dt(1e-30)
    with np.errstate(all="ignore"):
        m = mask(specs, mags, p["mask_floor"], dtype)
        n = (dt(1.0) - m).astype(dt)
        phi = []
        for wgt in (m, n):
            P = np.zeros((F, C, C), ct)
            for r in range(C):
                u = _weighted(X[r], wgt, ct)                                      # m_t X_{t,r}: each component rounded
                for k in range(r + 1):
                    P[:, r, k] = dr._sum_t(u * np.conj(X[k]), ct, order)
                    P[:, k, r] = np.conj(P[:, r, k])
                P[:, r, r] = P[:, r, r].real                                      # the diagonal's imaginary part is dropped
            phi.append(P)
        phi_s, phi_n = phi if slip is None else slip(*phi)
        idx = np.arange(C)
        tr = np.zeros(F, dt)
        for r in range(C):
            tr = tr + phi_n[:, r, r].real
        A = phi_n.copy()
        A[:, idx, idx] = (phi_n[:, idx, idx].real + ((delta * tr) / dt(C) + tiny)[:, None]).astype(dt)
        G = np.zeros((F, C, C), ct)
        for c in range(C):                                                        # one A: the factor is the same for every column
            G[:, :, c] = dr._cholesky_solve(A, np.ascontiguousarray(phi_s[:, :, c]))
        tau = np.zeros(F, dt)
        for c in range(C):
            tau = tau + G[:, c, c].real
        tau = dr._max(tau, tiny).astype(dt)
        w = np.empty((F, C), ct)
        w.real = G[:, :, ref].real / tau[:, None]
        w.imag = G[:, :, ref].imag / tau[:, None]
        Y = np.zeros((F, T), ct)
        for c in range(C):
            Y = (Y + np.conj(w[:, c])[:, None] * X[c]).astype(ct)
    Y = np.ascontiguousarray(Y.T)
    return (Y, w) if with_filter else Y


def gain_magnitudes(specs, dtype=np.float64):
    """The mask magnitudes of `mask="spectral"`: tests/baseline_ref.py's gain of every channel, (C, F, T)."""
    return np.stack([baseline_ref.spectral_gain(s, dtype=dtype)[0] for s in specs])


def beamform(x, n_fft=512, hop=128, params=None, wpe=False, gain=False, specs=None):
    """End to end in float64: x (C, L) -> (L,).  The STFT of every channel (or the given (C, T, F) spectrograms), optionally joint
    WPE at taps = 32 // C, the spectral gain of "baseline" per channel as the mask magnitudes, MVDR, optionally that gain on Y, the
    phase of Y, the inverse STFT of the input's length."""
    x = np.asarray(x)
    if specs is None:
        specs = np.stack([denoise_ref.stft(row, n_fft, hop) for row in x])
    if wpe:
        specs = dereverb_mc_ref.wpe_mc(specs)
    y = mvdr(specs, gain_magnitudes(specs), params)
    if gain:
        y = denoise_ref.rephase(baseline_ref.spectral_gain(y)[0], y)
    return denoise_ref.istft(y, hop, x.shape[1])


si_sdr = baseline_ref.si_sdr
