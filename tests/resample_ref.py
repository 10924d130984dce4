"""Float64 numpy restatement of the resampler and the SNR mixer defined in include/adn.h, plus the dataset rules of the
reference's train-set builder.  Test infrastructure (like oracle/): the package does not import it.

Resampler: g = gcd(src, dst), up = dst / g, down = src / g, q = max(up, down), half = ZEROS * q,
h[j] = up * fc * sinc(fc * j) * kaiser(2 * half + 1, BETA)[j + half] for j = -half .. half with fc = ROLLOFF / q,
M = ceil(L * up / down), y[m] = sum_i x[i] * h[m * down - i * up] over |m * down - i * up| <= half, 0 <= i < L.
With these taps ``scipy.signal.resample_poly(x, up, down, window=h / up)`` is the same operator.
"""
import math

import numpy as np

ZEROS = 32
BETA = 12.0
ROLLOFF = 0.88


def ratio(src_rate, dst_rate):
    g = math.gcd(int(src_rate), int(dst_rate))
    return int(dst_rate) // g, int(src_rate) // g


def design(up, down):
    """Prototype low-pass taps h[-half .. half] (float64), index j + half."""
    q = max(up, down)
    half = ZEROS * q
    fc = ROLLOFF / q
    j = np.arange(-half, half + 1, dtype=np.float64)
    return up * fc * np.sinc(fc * j) * np.kaiser(2 * half + 1, BETA)


def resample_length(length, src_rate, dst_rate):
    up, down = ratio(src_rate, dst_rate)
    return -(-length * up // down)


def resample_ref(x, src_rate, dst_rate):
    """x (L,) or (B, L) -> (y, sum_abs, taps): the float64 result; per output sum_i |h| |x| over the terms of its sum; and the
    number of those terms.  Vectorised per residue p = m mod up: the outputs m = p + up * k read x[k * down + a + d] for a fixed
    window of d with fixed coefficients, i.e. a strided view of the zero-extended input times that residue's taps."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        y, s, t = resample_ref(x[None], src_rate, dst_rate)
        return y[0], s[0], t[0]
    up, down = ratio(src_rate, dst_rate)
    B, L = x.shape
    if up == down:
        return x.copy(), np.abs(x), np.ones((B, L), dtype=np.int64)
    h = design(up, down)
    half = (len(h) - 1) // 2
    M = -(-L * up // down)
    y = np.zeros((B, M))
    sum_abs = np.zeros((B, M))
    taps = np.zeros((B, M), dtype=np.int64)
    K = half // up
    pad = K + 2
    ncyc = -(-M // up)
    width = pad + (ncyc - 1) * down + down + K + 2 + 1
    xp = np.zeros((B, max(width, pad + L) + 1))
    xp[:, pad:pad + L] = x
    valid = np.zeros(xp.shape[1])
    valid[pad:pad + L] = 1.0
    for p in range(min(up, M)):
        a, ph = divmod(p * down, up)
        dmin, dmax = -((half - ph) // up), (half + ph) // up
        d = np.arange(dmin, dmax + 1)
        c = h[ph - d * up + half]                              # coefficient of x[k * down + a + d]
        nk = len(range(p, M, up))
        start = pad + a + dmin
        idx = start + down * np.arange(nk)
        win = np.lib.stride_tricks.sliding_window_view(xp, len(d), axis=1)[:, idx, :]        # (B, nk, taps)
        y[:, p::up] = win @ c
        sum_abs[:, p::up] = np.abs(win) @ np.abs(c)
        taps[:, p::up] = np.lib.stride_tricks.sliding_window_view(valid, len(d))[idx].sum(axis=1).astype(np.int64)[None]
    return y, sum_abs, taps


def mix_snr_ref(clean, noise, snr_db):
    """add_noise for "white" / "urban" (create_train_dataset.py:147-157) in float64 -> (out, s, s * noise), s per clip."""
    c = np.asarray(clean, dtype=np.float64)
    n = np.asarray(noise, dtype=np.float64)
    c2, n2 = np.atleast_2d(c), np.atleast_2d(n)
    c_rms = np.sqrt(np.mean(c2 ** 2, axis=1) + 1e-12)
    n_rms = np.sqrt(np.mean(n2 ** 2, axis=1) + 1e-12)
    s = c_rms / (10.0 ** (snr_db / 20.0)) / n_rms
    scaled = s[:, None] * n2
    out = np.clip(c2 + scaled, -1.0, 1.0)
    return out.reshape(c.shape), s, scaled.reshape(c.shape)


def frame_audio(audio, chunk_samples):
    """Non-overlapping chunks, a shorter tail is dropped (create_train_dataset.py:71-84)."""
    return [audio[i:i + chunk_samples] for i in range(0, len(audio) - chunk_samples + 1, chunk_samples)]


def match_audio_length(noise, target_len, start):
    """create_train_dataset.py:52-68 with the random snippet position handed in."""
    if len(noise) == target_len:
        return noise.copy()
    if len(noise) < target_len:
        return np.tile(noise, int(np.ceil(target_len / len(noise))))[:target_len]
    return noise[start:start + target_len]


def noise_cancellation_ref(clean32, coins):
    """create_train_dataset.py:124-135 in float32 with the 0.8 coins handed in (one per 16000-sample block)."""
    clean32 = np.asarray(clean32, dtype=np.float32)
    noise = np.zeros_like(clean32)
    for b, coin in enumerate(coins):
        if coin:
            lo, hi = b * 16000, min(b * 16000 + 8000, len(clean32))
            noise[lo:hi] = np.float32(-0.8) * clean32[lo:hi]
    return np.clip(clean32 + noise, -1.0, 1.0)
