"""numpy restatement of the streaming MVDR beamformer as include/adn.h defines it ("beamform stream") -- TEST INFRASTRUCTURE, written
from the header text on top of tests/beamform_ref.py (the mask, the weighted products) and tests/dereverb_ref.py (`_cholesky_solve`,
`_max`).  float64 is the reference; dtype=np.float32 carries every statement out in float32, which is what the float32 floor of a
case is measured with.  Vectorised over bins; a group is (C, T, F), frame-major like the device's, its mask magnitudes (C, F, width)
with the frame fastest, columns [0, T) read.

The state is {"phi_s", "phi_n": (F, C, C) -- the lower triangle is carried, the diagonal with its imaginary part; the strict upper
triangle is never read --, "w": (F, C)}: what the device keeps per (slot, bin)."""
import numpy as np

import beamform_ref as bf
import dereverb_ref as dr

MAX_CHANNELS = bf.MAX_CHANNELS
DEFAULTS = dict(ref_channel=0, refresh=1, forget=0.99, loading=1e-3, mask_floor=1e-3)
FIELDS = ("ref_channel", "refresh", "forget", "loading", "mask_floor")
RANGES = dict(refresh=(1, 64), forget=(0.9, 1.0), loading=(1e-6, 1.0), mask_floor=(1e-6, 0.25))


def check_params(p, channels):
    """The legal ranges of the header; ValueError (naming the field) outside them."""
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("channels")
    for name in ("ref_channel", "refresh"):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(name)
    if not 0 <= p["ref_channel"] < channels:
        raise ValueError("ref_channel")
    for name in ("refresh", "forget", "loading", "mask_floor"):
        lo, hi = RANGES[name]
        if not lo <= p[name] <= hi:                                               # a NaN fails the comparison
            raise ValueError(name)


def fresh_state(channels, n_bins, dtype=np.float64):
    ct = np.complex64 if np.dtype(dtype).type is np.float32 else np.complex128
    return dict(phi_s=np.zeros((n_bins, channels, channels), ct), phi_n=np.zeros((n_bins, channels, channels), ct),
                w=np.zeros((n_bins, channels), ct))


def cholesky_solve_columns(A, P):
    """dereverb_ref._cholesky_solve for every column of P (F, K, n) at once: the same statements in the same order per element
    (tests/test_beamform_stream_host.py holds the two bit for bit), one factorisation."""
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
            v = v - L[:, r, k][:, None] * y[:, k]
        y[:, r] = v / L[:, r, r].real[:, None]
    g = np.zeros_like(P)
    for r in range(K - 1, -1, -1):
        v = y[:, r].copy()
        for k in range(K - 1, r, -1):
            v = v - np.conj(L[:, k, r])[:, None] * g[:, k]
        g[:, r] = v / L[:, r, r].real[:, None]
    return g


def solve(phi_s, phi_n, ref, delta, dt):
    """"beamform"'s filter from the carried lower triangles: (F, C, C), (F, C, C) -> w (F, C)."""
    ct = phi_s.dtype.type
    F, C, _ = phi_s.shape
    idx, tiny = np.arange(C), dt(1e-30)
    full = []
    for P in (phi_s, phi_n):                                                      # Hermitian, the diagonal real: dropped at use
        H = np.tril(P, -1)
        H = H + np.conj(H.transpose(0, 2, 1))
        H[:, idx, idx] = P[:, idx, idx].real
        full.append(H.astype(ct))
    hs, hn = full
    tr = np.zeros(F, dt)
    for r in range(C):
        tr = tr + hn[:, r, r].real
    A = hn.copy()
    A[:, idx, idx] = (hn[:, idx, idx].real + ((delta * tr) / dt(C) + tiny)[:, None]).astype(dt)
    G = cholesky_solve_columns(A, hs)                                             # one A: the factor is the same for every column
    tau = np.zeros(F, dt)
    for c in range(C):
        tau = tau + G[:, c, c].real
    tau = dr._max(tau, tiny).astype(dt)
    w = np.empty((F, C), ct)
    w.real = G[:, :, ref].real / tau[:, None]
    w.imag = G[:, :, ref].imag / tau[:, None]
    return w


def mvdr_stream(specs, mags, params=None, dtype=np.float64, state=None, first_frame=0):
    """specs (C, T, F) complex: frames first_frame ... first_frame + T - 1; mags (C, F, width >= T) real -> (Y (T, F) complex in
    `dtype`'s precision, the state after the last frame).  `state`: what an earlier call returned for the frames before (it is not
    modified); with first_frame = 0 the group starts fresh whatever it holds."""
    specs = np.asarray(specs)
    C, T, F = specs.shape
    p = dict(DEFAULTS)
    p.update(params or {})
    check_params(p, C)
    dt = np.dtype(dtype).type
    ct = np.complex64 if dt is np.float32 else np.complex128
    ref, R = int(p["ref_channel"]), int(p["refresh"])
    alpha, delta = dt(np.float32(p["forget"])), dt(np.float32(p["loading"]))
    if first_frame == 0 or state is None:
        if first_frame != 0:
            raise ValueError("first_frame > 0 continues a group: pass its state")
        state = fresh_state(C, F, dtype)
    phi_s, phi_n, w = (np.array(state[k], dtype=ct) for k in ("phi_s", "phi_n", "w"))
    X = specs.astype(ct)                                                          # (C, T, F)
    Y = np.zeros((T, F), ct)
    with np.errstate(all="ignore"):
        m_all = bf.mask(specs, mags, p["mask_floor"], dtype)                      # (F, T): "beamform"'s, frame by frame
        for i in range(T):
            t = first_frame + i
            m = m_all[:, i]
            n = (dt(1.0) - m).astype(dt)
            xt = np.ascontiguousarray(X[:, i].T)                                  # (F, C)
            for P, wgt in ((phi_s, m), (phi_n, n)):
                u = bf._weighted(xt, wgt[:, None], ct)                            # m_t X_{t,r}: each component rounded
                # every (r, k) at once; only r >= k is ever read.  alpha (.) Phi: each component rounded, then the addend
                P[...] = (u[:, :, None] * np.conj(xt)[:, None, :] + bf._weighted(P, alpha, ct)).astype(ct)
            if t % R == 0:
                w = solve(phi_s, phi_n, ref, delta, dt)
            y = np.zeros(F, ct)
            for c in range(C):
                y = (y + np.conj(w[:, c]) * X[c, i]).astype(ct)
            Y[i] = y
    return Y, dict(phi_s=phi_s, phi_n=phi_n, w=w.copy())


def stream_mask_magnitudes(specs, dtype=np.float64):
    """The mask magnitudes of StreamBeamformer: the (causal) spectral gain of every channel, (C, F, T)."""
    return bf.gain_magnitudes(specs, dtype)


def stream_beamform(x, n_fft=512, hop=128, params=None, gain=False, dtype=np.float64):
    """End to end, what StreamBeamformer returns for the finished recording x (C, L) -> (L,): the STFT of every channel, the
    spectral gain of every channel as the mask magnitudes, the recursion, then M = |Y| (with gain=True the spectral gain on it),
    M with the phase of Y and the inverse STFT of the input's length -- the resynthesis of tests/dereverb_mc_stream_ref.py,
    statement for statement.  dtype=np.float32 carries EVERY statement out in float32, the two transforms included."""
    import dereverb_mc_stream_ref as ms
    import dereverb_stream_ref as ds
    import denoise_ref
    f32 = np.dtype(dtype) == np.float32
    x = np.asarray(x)
    specs = np.stack([ds.stft32(row, n_fft, hop) if f32 else denoise_ref.stft(row, n_fft, hop) for row in x])
    y, _ = mvdr_stream(specs, stream_mask_magnitudes(specs, dtype), params, dtype=dtype)
    return ms._resynth(y, hop, x.shape[1], gain, None, dtype)


si_sdr = bf.si_sdr
