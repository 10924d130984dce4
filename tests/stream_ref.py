"""float64 numpy restatement of the streaming definition of include/adn.h ("stream") -- TEST INFRASTRUCTURE.
The whole-signal formulation, built on denoise_ref's stft / istft / rephase: step k sees frames [k B + B + A - W, k B + B + A) of
the finished signal's spectrogram and keeps local frames [W - B - A, W - A) of the network's answer.  The network is passed in as
a callable on (K, F, W) arrays.  Spectrograms are frame-major (T, F) like the device's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as ref  # noqa: E402


def steps_done(received, n_fft, hop, block, lookahead):
    r = received - n_fft // 2 - (block + lookahead - 1) * hop
    return 0 if r < 0 else r // (block * hop) + 1


def emitted(received, n_fft, hop, block, lookahead):
    return max(0, steps_done(received, n_fft, hop, block, lookahead) * block * hop - n_fft // 2)


def latency(n_fft, hop, block, lookahead):
    return (block + lookahead - 1) * hop + n_fft


def n_steps(n_frames, block):
    """K = ceil(T / B): the steps of a stream of T frames."""
    return -(-n_frames // block)


def windows(mag, window, block, lookahead):
    """(T, F) magnitudes -> (K, F, W): window k holds frames [k B + B + A - W, k B + B + A), zero before 0 and from T on."""
    n_frames, n_bins = mag.shape
    out = np.zeros((n_steps(n_frames, block), n_bins, window), dtype=mag.dtype)
    for k in range(out.shape[0]):
        first = k * block + block + lookahead - window
        lo, hi = max(first, 0), min(first + window, n_frames)
        if hi > lo:
            out[k, :, lo - first:hi - first] = mag[lo:hi].T
    return out


def join(y, n_frames, window, block, lookahead, clamp=True):
    """(K, F, W) -> (F, T): frame k B + i is local frame W - B - A + i of window k, nothing is blended."""
    assert y.shape[0] == n_steps(n_frames, block) and y.shape[2] == window
    out = np.zeros((y.shape[1], n_frames), dtype=np.float64)
    j0 = window - block - lookahead
    for k in range(y.shape[0]):
        n = min(block, n_frames - k * block)
        out[:, k * block:k * block + n] = y[k, :, j0:j0 + n]
    if clamp:
        out = np.where(np.isnan(out), out, np.maximum(out, 0.0))
    return out


def resynth(y, spec, length, hop, window, block, lookahead):
    """Network output (K, F, W) + the input's STFT (T, F) -> audio (length,): join, clamp, noisy phase, inverse STFT."""
    return ref.istft(ref.rephase(join(y, spec.shape[0], window, block, lookahead), spec), hop, length)


def denoise(x, net, n_fft=512, hop=128, window=192, block=16, lookahead=0):
    spec = ref.stft(x, n_fft, hop)
    return resynth(net(windows(np.abs(spec), window, block, lookahead)), spec, len(x), hop, window, block, lookahead)
