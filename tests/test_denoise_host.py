"""Host side of the long-form denoiser: the window plan, the float64 restatement (tests/denoise_ref.py) and the argument
checks of the four adn_denoise_* entry points.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as ref  # noqa: E402

PARAMS = ((512, 128, 256, 32), (512, 128, 64, 0), (256, 64, 48, 24), (1024, 256, 32, 16))     # n_fft, hop, W, V


def lengths(hop):
    return (24000, 24001, 100000, 37, 1, hop - 1, 2 * hop - 1)


def _lib():
    from audiodenoiser_amd import _lib as m
    return m, m.load()


def _plan_brute(n_frames, window, overlap):
    if n_frames <= window:
        return 1, max(n_frames, 16)
    k = 1
    while (k - 1) * (window - overlap) + window < n_frames:
        k += 1
    return k, window


@pytest.mark.parametrize("window,overlap", ((256, 32), (64, 0), (48, 24), (32, 16), (16, 8), (17, 3)))
def test_plan_rule_coverage_and_weights(window, overlap):
    m, L = _lib()
    k_out, w_out = ctypes.c_int(), ctypes.c_int()
    stride = window - overlap
    for n_frames in range(1, 3 * window + 1):
        k, width = ref.plan(n_frames, window, overlap)
        assert (k, width) == _plan_brute(n_frames, window, overlap), n_frames
        assert L.adn_denoise_plan(n_frames, window, overlap, ctypes.byref(k_out), ctypes.byref(w_out)) == 0
        assert (k_out.value, w_out.value) == (k, width), n_frames
        cover = np.zeros(n_frames, dtype=int)
        total = np.zeros(n_frames)
        for i in range(k):
            lo = i * stride
            n = min(width, n_frames - lo)
            assert n >= 1, (n_frames, i)                     # no window starts past the end
            cover[lo:lo + n] += 1
            total[lo:lo + n] += ref.weights(i, k, width, overlap)[:n]
        assert cover.min() >= 1 and cover.max() <= 2, n_frames
        assert np.abs(total - 1.0).max() <= 1e-15, n_frames


@pytest.mark.parametrize("n_fft,hop,window,overlap", PARAMS)
def test_identity_network_reconstructs_the_input(n_fft, hop, window, overlap):
    """With y = in the definition is STFT -> |X| -> |X| * X / |X| -> iSTFT of length L: perfect reconstruction for the Hann
    window at hop <= n_fft / 4 (measured with this restatement: worst 6.7e-16; the bound leaves room for another FFT)."""
    worst = 0.0
    for length in lengths(hop):
        x = np.random.default_rng([n_fft, window, length]).uniform(-1.0, 1.0, length)
        out = ref.denoise(x, lambda w: w, n_fft, hop, window, overlap)
        assert out.shape == x.shape
        worst = max(worst, float(np.abs(out - x).max()))
        n_frames = 1 + length // hop
        wss = ref.window_sumsquare(n_frames, n_fft, hop)[n_fft // 2:n_fft // 2 + length]
        assert wss.min() >= 0.25, (length, float(wss.min()))
    print(f"n_fft {n_fft} hop {hop} W {window} V {overlap}: worst |x^ - x| = {worst:.3g}")
    assert worst <= 1e-12


def test_window_sumsquare_collapses_at_half_overlap():
    """Why hop <= n_fft / 4: at hop = n_fft / 2 the divisor of the last tail sample is ~2e-8."""
    n_fft, hop = 512, 256
    for length in (hop - 1, 2 * hop - 1):
        wss = ref.window_sumsquare(1 + length // hop, n_fft, hop)[n_fft // 2:n_fft // 2 + length]
        assert wss.min() < 1e-4


def test_restatement_is_anchored_to_the_oracle():
    """The restatement's float64 STFT / iSTFT against oracle/griffin_lim_numpy.py (complex64 / float32 storage) on 24 000 samples:
    1e-6 of the maximum (measured: STFT 3.5e-8, iSTFT 1.7e-7)."""
    from oracle import griffin_lim_numpy as gl
    x = np.random.default_rng(3).uniform(-1.0, 1.0, 24000).astype(np.float32)
    mine = ref.stft(x, 512, 128)
    theirs = gl.stft_complex(x, 512, 128).T
    assert mine.shape == theirs.shape == (188, 257)
    e_stft = float(np.abs(mine - theirs).max() / np.abs(mine).max())
    back = ref.istft(mine, 128, 128 * 187)
    theirs_back = gl.istft(mine.T, 128)
    e_istft = float(np.abs(back - theirs_back).max() / np.abs(back).max())
    print(f"stft {e_stft:.3g}, istft {e_istft:.3g}")
    assert e_stft <= 1e-6 and e_istft <= 1e-6


def test_stitch_restatement_passes_non_finite_values():
    y = np.random.default_rng(4).standard_normal((4, 5, 64))
    y[1, 2, 3] = np.nan
    y[2, 0, 60] = np.inf
    out = ref.stitch(y, 200, 64, 16, clamp=True)
    assert np.isnan(out[2, 48 + 3]) and np.isinf(out[0, 96 + 60])
    assert np.isfinite(np.delete(out.ravel(), [2 * 200 + 51, 156])).all() and out[np.isfinite(out)].min() >= 0.0


def test_entry_point_argument_errors():
    m, L = _lib()
    k, w = ctypes.c_int(), ctypes.c_int()
    good = 1 << 12                                            # an aligned, never dereferenced address: every call below is refused first

    def refused(rc, text):
        assert rc == 1, rc                                    # ADN_ERR_INVALID
        assert text.encode() in L.adn_last_error(), L.adn_last_error()

    refused(L.adn_denoise_plan(0, 256, 32, ctypes.byref(k), ctypes.byref(w)), "adn_denoise_plan: need n_frames >= 1")
    refused(L.adn_denoise_plan(100, 15, 0, ctypes.byref(k), ctypes.byref(w)), "window >= 16")
    refused(L.adn_denoise_plan(100, 64, 33, ctypes.byref(k), ctypes.byref(w)), "overlap <= window / 2")
    refused(L.adn_denoise_plan(100, 64, -1, ctypes.byref(k), ctypes.byref(w)), "0 <= overlap")
    refused(L.adn_denoise_plan(100, 64, 8, None, ctypes.byref(w)), "adn_denoise_plan: null pointer")
    refused(L.adn_denoise_windows(None, 1, 100, 257, 64, 8, good, None), "adn_denoise_windows: null pointer")
    refused(L.adn_denoise_windows(good, 0, 100, 257, 64, 8, good, None), "adn_denoise_windows: n_clips and n_bins")
    refused(L.adn_denoise_windows(good, 1, 100, 257, 64, 40, good, None), "adn_denoise_windows: need n_frames >= 1")
    refused(L.adn_denoise_windows(good + 4, 1, 100, 257, 64, 8, good, None), "spec must be 8-byte aligned")
    refused(L.adn_denoise_stitch(good, 1, 100, 257, 64, 8, 0, None, None), "adn_denoise_stitch: null pointer")
    refused(L.adn_denoise_stitch(good, 1, 100, 257, 64, 8, 0, good, None), "out may not alias y")
    refused(L.adn_denoise_stitch(good, 1, 100, 257, 64, 8, 2, 2 * good, None), "clamp must be 0 or 1")
    refused(L.adn_denoise_stitch(good, 1, 100, 0, 64, 8, 1, 2 * good, None), "adn_denoise_stitch: n_clips and n_bins")
    refused(L.adn_denoise_stitch(good, 1, 0, 257, 64, 8, 1, 2 * good, None), "adn_denoise_stitch: need n_frames >= 1")
    refused(L.adn_denoise_stitch(good + 4, 1, 128, 257, 64, 8, 1, 2 * good, None), "16-byte")
    refused(L.adn_denoise_resynth(good, None, 1, 1000, 512, 128, 256, 32, good, None), "adn_denoise_resynth: null pointer")
    refused(L.adn_denoise_resynth(good, good, 1, 1000, 500, 125, 256, 32, good, None), "n_fft must be a power of two")
    refused(L.adn_denoise_resynth(good, good, 1, 1000, 512, 256, 256, 32, good, None), "hop <= n_fft / 4")
    refused(L.adn_denoise_resynth(good, good, 1, 1000, 512, 0, 256, 32, good, None), "hop <= n_fft / 4")
    refused(L.adn_denoise_resynth(good, good, 1, 0, 512, 128, 256, 32, good, None), "1 <= length < 2^30")
    refused(L.adn_denoise_resynth(good, good, 1, 1 << 30, 512, 128, 256, 32, good, None), "1 <= length < 2^30")
    refused(L.adn_denoise_resynth(good, good, 0, 1000, 512, 128, 256, 32, good, None), "n_clips >= 1")
    refused(L.adn_denoise_resynth(good, good, 1, 1000, 512, 128, 8, 0, good, None), "window >= 16")
    refused(L.adn_denoise_resynth(good, good + 4, 1, 1000, 512, 128, 256, 32, good, None), "spec must be 8-byte aligned")


def test_denoiser_constructor_refusals():
    import torch
    from audiodenoiser_amd import Denoiser
    from audiodenoiser_amd.denoise import denoise_plan
    from audiodenoiser_amd.model import UNet
    assert denoise_plan(782) == (4, 256) and denoise_plan(188) == (1, 188) and denoise_plan(1) == (1, 16)
    net = UNet(1, 1).eval()
    for kwargs in (dict(n_fft=500), dict(n_fft=32), dict(hop_length=256), dict(hop_length=0), dict(window_frames=8),
                   dict(overlap_frames=129), dict(overlap_frames=-1), dict(phase="random"), dict(batch_windows=0),
                   dict(sample_rate=0), dict(gl_iterations=-1)):
        with pytest.raises(ValueError, match="Denoiser"):
            Denoiser(net, **kwargs)
    with pytest.raises(ValueError, match=r"UNet\(1, 1\)"):
        Denoiser(torch.nn.Conv2d(1, 1, 3))
    with pytest.raises(ValueError, match=r"UNet\(1, 1\)"):
        Denoiser(UNet(2, 1).eval())
    with pytest.raises(RuntimeError, match="train mode"):
        Denoiser(UNet(1, 1))
    if not next(net.parameters()).is_cuda:
        with pytest.raises(RuntimeError, match="ROCm device"):
            Denoiser(net)
