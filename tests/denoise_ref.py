"""float64 numpy restatement of the long-form denoising definition of include/adn.h ("denoise") -- TEST INFRASTRUCTURE.
Self-contained: own STFT, inverse STFT to the input's length, window plan, cross-fade weights, stitch and phase; the network
is passed in as a callable on (K, F, width) arrays.  Spectrograms are frame-major (T, F) like the device's."""
import numpy as np


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def stft(x, n_fft, hop):
    """(L,) -> (T, F) complex128, T = 1 + L // hop, centred, zero padded (no padding to a multiple of hop)."""
    xp = np.pad(np.asarray(x, np.float64), n_fft // 2)
    idx = hop * np.arange(1 + len(x) // hop)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(hann(n_fft) * xp[idx], axis=1)


def window_sumsquare(n_frames, n_fft, hop):
    wss = np.zeros(n_fft + hop * (n_frames - 1))
    for t in range(n_frames):
        wss[t * hop:t * hop + n_fft] += hann(n_fft) ** 2
    return wss


def istft(spec, hop, length):
    """(T, F) complex -> (length,): overlap-added windowed frames over the window sum-of-squares, n_fft/2 trimmed in front."""
    n_frames, n_fft = spec.shape[0], 2 * (spec.shape[1] - 1)
    frames = np.fft.irfft(spec, n=n_fft, axis=1) * hann(n_fft)
    y = np.zeros(n_fft + hop * (n_frames - 1))
    for t in range(n_frames):
        y[t * hop:t * hop + n_fft] += frames[t]
    wss = window_sumsquare(n_frames, n_fft, hop)
    y = np.where(wss > np.finfo(np.float32).tiny, y / np.where(wss > 0, wss, 1.0), y)
    assert n_fft // 2 + length <= len(y)
    return y[n_fft // 2:n_fft // 2 + length]


def plan(n_frames, window, overlap):
    """-> (K, width)."""
    if n_frames <= window:
        return 1, max(n_frames, 16)
    stride = window - overlap
    return 1 + -(-(n_frames - window) // stride), window


def weights(k, n_windows, width, overlap):
    """Cross-fade weights of window k over its local frames."""
    a = np.ones(width)
    j = np.arange(overlap)
    if k > 0:
        a[:overlap] = (j + 1.0) / (overlap + 1.0)
    if k < n_windows - 1:
        a[width - overlap:] = (width - (width - overlap + j)) / (overlap + 1.0)
    return a


def windows(mag, window, overlap):
    """(T, F) magnitudes -> (K, F, width), frames past the end zero."""
    n_frames = mag.shape[0]
    n_windows, width = plan(n_frames, window, overlap)
    out = np.zeros((n_windows, mag.shape[1], width), dtype=mag.dtype)
    for k in range(n_windows):
        part = mag[k * (window - overlap):k * (window - overlap) + width]
        out[k, :, :part.shape[0]] = part.T
    return out


def stitch(y, n_frames, window, overlap, clamp=False, with_sum_abs=False):
    """(K, F, width) -> (F, T); optionally also sum_k a_k |y| (the scale of the rounding bound)."""
    n_windows, width = plan(n_frames, window, overlap)
    assert y.shape[0] == n_windows and y.shape[2] == width
    out = np.zeros((y.shape[1], n_frames), dtype=np.float64)
    sum_abs = np.zeros_like(out)
    for k in range(n_windows):
        lo = k * (window - overlap)
        n = min(width, n_frames - lo)
        a = weights(k, n_windows, width, overlap)[:n]
        out[:, lo:lo + n] += a * y[k, :, :n]
        sum_abs[:, lo:lo + n] += a * np.abs(y[k, :, :n])
    if clamp:
        out = np.where(np.isnan(out), out, np.maximum(out, 0.0))
    return (out, sum_abs) if with_sum_abs else out


def rephase(m, spec):
    """m (F, T) real, spec (T, F) complex -> (T, F): m with the phase of spec, m itself where |spec| = 0."""
    mag = np.abs(spec)
    return np.where(mag > 0, m.T * spec / np.where(mag > 0, mag, 1.0), m.T + 0j)


def resynth(y, spec, length, hop, window, overlap):
    """Network output (K, F, width) + the input's STFT (T, F) -> audio (length,): stitch, clamp, noisy phase, inverse STFT."""
    return istft(rephase(stitch(y, spec.shape[0], window, overlap, clamp=True), spec), hop, length)


def denoise(x, net, n_fft=512, hop=128, window=256, overlap=32):
    spec = stft(x, n_fft, hop)
    return resynth(net(windows(np.abs(spec), window, overlap)), spec, len(x), hop, window, overlap)
