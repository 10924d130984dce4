"""The cases of the streaming spectral-baseline tests (tests/test_baseline_stream_host.py, tests/test_gpu_baseline_stream.py) --
TEST INFRASTRUCTURE.  Everything is seeded; the signals are tests/baseline_cases.py's.

    python tests/baseline_stream_cases.py     measures, on the host from the restatement, the float32 floor of the magnitude form
                                              over the end-to-end cases and writes FLOOR_WINDOWS into this file

If a case exceeds 10 x baseline_ref.FLOOR, a `Pmin < P` comparison flipped in float32 on that input: change E2E_SEED, not a bound.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_cases as bc  # noqa: E402
import baseline_ref as br  # noqa: E402
import denoise_ref  # noqa: E402

N_FFT, HOP = 512, 128
F = N_FFT // 2 + 1

# The float32 host floor of the magnitude form: the worst max|M32 - M64| / max M64 over the end-to-end cases below, measured on the
# host from tests/baseline_ref.py called with m.astype(complex) (never from the device), written here by this file's main().
FLOOR_WINDOWS = 1.4e-07

# ---- the kernel alone: F = 33 (less than a wave), 257 (four waves + 1 lane), 513 (eight waves + 1 lane) ------------------------------
KERNEL_BINS = (33, 257, 513)
KERNEL_ROWS = (1, 3)
# (W, col0, n_cols, n_steps): a step of the default plan; whole windows over three steps (48 frames: a tile and a half);
# single-column steps across a tile boundary; the U-Net stream's plan; a tile of 32 frames that spans steps of 5
KERNEL_PLANS = ((16, 12, 4, 1), (16, 0, 16, 3), (16, 15, 1, 40), (192, 176, 16, 5), (20, 7, 5, 7))
TILE = bc.TILE

# ---- float64 equivalence of the stream of steps with the offline form, and the end-to-end cases -------------------------------------
LENGTHS = (100, 2047, 24000)
BLOCKS = (1, 4, 5, 16)
E2E_SEED = 50


def magnitudes(n_rows, n_frames, n_bins, seed):
    """(n_rows, n_frames, n_bins) float32 >= 0: squared normal draws under a slow per-row envelope, every 17th frame of bin 0
    exactly zero -- nothing a spectrogram could not hold, and no two rows alike."""
    rng = np.random.default_rng([seed, n_rows, n_frames, n_bins])
    m = rng.standard_normal((n_rows, n_frames, n_bins)) ** 2
    env = 0.05 + np.abs(np.sin(np.arange(n_frames)[None, :, None] * 0.21 + np.arange(n_rows)[:, None, None]))
    m = (m * env).astype(np.float32)
    m[:, ::17, 0] = 0.0
    return m


def e2e_audio(length, seed=E2E_SEED):
    """float32 (length,): the last `length` samples of a white mix at 8 dB that is one second longer (speech and noise from sample 0)."""
    return bc.white_mix(8000 + length, 8.0, seed)[0][8000:]


def window_of(block):
    return max(16, block)


def gain_net(block, dtype=np.float64, params=None):
    """The magnitude form as tests/stream_ref.py's network callable: (K, F, W) -> (K, F, W), the recurrence run over the kept
    columns [W - B, W) of the windows in step order, the other columns zero."""
    def net(win):
        out = np.zeros(win.shape, dtype)
        state = None
        w = win.shape[2]
        for k in range(win.shape[0]):
            m = win[k, :, w - block:].T.astype(dtype)                  # (B, F): frame-major, as the restatement takes it
            out[k, :, w - block:], state = br.spectral_gain(m.astype(np.complex128 if dtype == np.float64 else np.complex64),
                                                            params, state, dtype)
        return out
    return net


def floor_of_windows(m):
    """max|M32 - M64| / max M64 of one stream's (T, F) float32 magnitudes."""
    m64, _ = br.spectral_gain(m.astype(np.complex128), dtype=np.float64)
    m32, _ = br.spectral_gain(m.astype(np.complex64), dtype=np.float32)
    return float(np.abs(m32.astype(np.float64) - m64).max() / m64.max())


def measure_floor(verbose=False):
    worst = 0.0
    for length in LENGTHS:
        m = np.abs(denoise_ref.stft(e2e_audio(length), N_FFT, HOP)).astype(np.float32)
        f = floor_of_windows(m)
        if verbose:
            print(f"L {length}: {f:.3g} ({f / br.FLOOR:.2f} of baseline_ref.FLOOR)")
        assert f <= 10.0 * br.FLOOR, "a Pmin < P comparison flipped in float32 on this input: change E2E_SEED"
        worst = max(worst, f)
    return worst


def main():
    floor = measure_floor(verbose=True)
    text = f"{floor:.1e}"
    path = os.path.abspath(__file__)
    src = open(path).read()
    src, n = re.subn(r"^FLOOR_WINDOWS = .*$", f"FLOOR_WINDOWS = {text}", src, flags=re.M)
    assert n == 1
    open(path, "w").write(src)
    print(f"FLOOR_WINDOWS = {text} (unrounded {floor:.4g})")


if __name__ == "__main__":
    main()
