"""numpy restatement of the spectral baseline of include/adn.h ("baseline") -- TEST INFRASTRUCTURE, written from the header text.
float64 is the reference; dtype=np.float32 runs the same statements, one rounding each, which is how the float32 host floor
FLOOR below was measured (python tests/baseline_cases.py).  Spectrograms are frame-major (T, F) like the device's; the end-to-end
form is built on tests/denoise_ref.py's stft / rephase / istft."""
import numpy as np

import denoise_ref

DEFAULTS = dict(smooth=0.7, beta=0.96, gamma=0.998, alpha=0.98, gain_floor=0.1, bias=1.0)
FIELDS = ("smooth", "beta", "gamma", "alpha", "gain_floor", "bias")

# The float32 host floor: the worst max|M32 - M64| / max M64 per clip over the GPU parity cases of tests/baseline_cases.py,
# measured on the host from this restatement (never from the device) and written here by `python tests/baseline_cases.py`.
FLOOR = 1.7e-06


def check_params(p):
    """The legal ranges of the header; ValueError outside them."""
    for name in ("smooth", "beta", "alpha"):
        if not 0.0 <= p[name] < 1.0:
            raise ValueError(name)
    if not 0.0 < p["gamma"] < 1.0:
        raise ValueError("gamma")
    if not 0.0 < p["gain_floor"] <= 1.0:
        raise ValueError("gain_floor")
    if not 0.0 < p["bias"] <= 100.0:
        raise ValueError("bias")


def _max(x, c):
    """max(x, c) of the header: x < c ? c : x -- a NaN x stays NaN."""
    return np.where(x < c, c, x)


def spectral_gain(spec, params=None, state=None, dtype=np.float64):
    """spec (T, F) complex -> (M (F, T), state (3, F)) in `dtype`.  `state` (3, F) = rows P, Pmin, S carried from the previous
    call, a bin whose P is negative starts fresh; None: every bin starts fresh.  The parameters are the fp32 values of the struct;
    the derived constants are computed from them in `dtype`."""
    p = dict(DEFAULTS)
    p.update(params or {})
    check_params(p)
    dt = np.dtype(dtype).type
    a_s, b, g, alpha, g_min, bias = (dt(np.float32(p[name])) for name in FIELDS)
    one = dt(1.0)
    c_s, c_g, c_a = one - a_s, (one - g) / (one - b), one - alpha
    spec = np.asarray(spec)
    n_frames, n_bins = spec.shape
    re, im = spec.real.astype(dtype), spec.imag.astype(dtype)
    if state is None:
        P, Pmin, S = np.full(n_bins, -1.0, dtype), np.zeros(n_bins, dtype), np.zeros(n_bins, dtype)
    else:
        P, Pmin, S = (np.array(row, dtype) for row in state)
    fresh = P < 0
    out = np.empty((n_bins, n_frames), dtype)
    tiny, zero = dt(1e-30), dt(0.0)
    if dt is np.float32:
        tiny = np.float32(1e-30)
    with np.errstate(all="ignore"):
        for t in range(n_frames):
            im2 = im[t] * im[t]
            # fmaf(re, re, im * im): the product im * im rounds, re * re + that rounds once -- in float32 through float64, where
            # re * re is exact and the sum's double rounding can differ from the fma in the last bit of rare cases
            if dt is np.float32:
                pw = (re[t].astype(np.float64) * re[t].astype(np.float64) + im2.astype(np.float64)).astype(np.float32)
            else:
                pw = re[t] * re[t] + im2
            Pn = np.where(fresh, pw, a_s * P + c_s * pw)
            grown = g * Pmin + c_g * (Pn - b * P)
            Pm = np.where(~fresh & (Pmin < Pn), grown, Pn)
            N = _max(bias * Pm, tiny)
            Sp = np.where(fresh, zero, S)
            xi = (alpha * Sp) / N + c_a * _max(pw / N - one, zero)
            G = _max(xi / (one + xi), g_min)
            out[:, t] = G * np.sqrt(pw)
            P, Pmin, S = Pn.astype(dtype), Pm.astype(dtype), ((G * G) * pw).astype(dtype)
            fresh = np.zeros(n_bins, bool)
    return out.astype(dtype), np.stack([P, Pmin, S]).astype(dtype)


def denoise(x, n_fft=512, hop=128, params=None, spec=None):
    """End to end in float64: STFT (or the given (T, F) spectrogram), gain, the noisy phase, inverse STFT of the input's length."""
    if spec is None:
        spec = denoise_ref.stft(x, n_fft, hop)
    mag, _ = spectral_gain(spec, params)
    return denoise_ref.istft(denoise_ref.rephase(mag, spec), hop, len(x))


def si_sdr(est, ref):
    """Scale-invariant SDR in dB, float64 (the definition of adn_quality, include/adn.h)."""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    a = np.dot(est, ref) / np.dot(ref, ref)
    return 10.0 * np.log10(np.sum((a * ref) ** 2) / np.sum((est - a * ref) ** 2))
