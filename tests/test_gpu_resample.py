"""Device resampler (adn_resample), SNR mixer (adn_mix_snr) and the datasets built on them against the float64 restatement
in tests/resample_ref.py.

Bounds (derived, not tuned):
* resample, per element: |y - y_ref| <= 1.01 * (taps + 2) * 2^-24 * sum_i |h||x| -- an fp32 sum of `taps` fp32 products in any
  order plus one rounding of each coefficient; where sum |h||x| is 0 the output is exactly 0.
* mix_snr, per sample: |out - ref| <= 1e-5 * |s noise| + 3 * 2^-24 * (|clean| + |s noise|) -- a relative error of 1e-5 in the
  scale (blocked pairwise fp32 sums of non-negative terms err by < 2e-6) plus the roundings of one multiply and one add.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref  # noqa: E402
from conftest import load_real_audio_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
RATE_PAIRS = ((44100, 8000), (8000, 44100), (48000, 8000), (22050, 8000), (16000, 8000), (8000, 16000), (44100, 48000))
SHAPES = ((1, 1), (3, 100), (64, 4001), (2, 176400))
RESAMPLE_CASES = [(src, dst, n, length) for (src, dst) in RATE_PAIRS for (n, length) in SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _resample_bound(sum_abs, taps):
    return 1.01 * (taps + 2) * EPS * sum_abs


def _check_resample(x, src, dst, what):
    from audiodenoiser_amd.resample import resample
    y = resample(x, src, dst)
    y_ref, sum_abs, taps = ref.resample_ref(x, src, dst)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == y_ref.shape, what
    err = np.abs(y.astype(np.float64) - y_ref)
    bound = _resample_bound(sum_abs, taps)
    share = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
    print(f"{what}: {y.size} outputs, taps <= {int(taps.max())}, max err {err.max():.3g}, largest share of the bound {share:.3f}")
    assert np.all(y[sum_abs == 0] == 0), what
    assert np.all(err <= bound), (what, float(err.max()), share)
    return y


@pytest.mark.parametrize("src,dst,n_clips,length", RESAMPLE_CASES)
def test_resample_against_reference(dev, src, dst, n_clips, length):
    rng = np.random.default_rng([src, dst, n_clips, length])
    x = rng.uniform(-1.0, 1.0, (n_clips, length)).astype(np.float32)
    _check_resample(x, src, dst, f"{src}->{dst} ({n_clips}, {length})")


@pytest.mark.parametrize("src,dst", ((44100, 8000), (8000, 44100)))
@pytest.mark.parametrize("where", ("first", "last"))
def test_resample_impulse_at_the_edges(dev, src, dst, where):
    x = np.zeros((1, 4001), dtype=np.float32)
    x[0, 0 if where == "first" else -1] = 1.0
    y = _check_resample(x, src, dst, f"impulse {where} {src}->{dst}")
    assert np.abs(y).max() > 0          # the filter's main lobe peaks at up * fc = 0.16 (44100 -> 8000): the edge is not dropped


@pytest.mark.parametrize("src,dst,n_clips,length", ((48000, 50, 2, 100000), (1000, 4001, 3, 300), (4096, 1, 1, 300000)))
def test_resample_ratios_beyond_the_staged_path(dev, src, dst, n_clips, length):
    """Rate pairs whose 64-cycle input span does not fit the LDS (down > ~550) take the kernel's global-memory path: same
    definition, same bound."""
    rng = np.random.default_rng([src, dst, n_clips, length])
    x = rng.uniform(-1.0, 1.0, (n_clips, length)).astype(np.float32)
    _check_resample(x, src, dst, f"{src}->{dst} ({n_clips}, {length})")


def test_resample_equal_rates_is_a_copy(dev):
    from audiodenoiser_amd.resample import resample
    x = np.random.default_rng(5).uniform(-1, 1, (3, 1001)).astype(np.float32)
    assert np.array_equal(resample(x, 8000, 8000), x)
    xt = torch.from_numpy(x).to(dev)
    y = resample(xt, 8000, 8000)
    assert y.data_ptr() != xt.data_ptr() and torch.equal(y, xt)


def test_resample_real_clip(dev, golden_dir):
    fx = load_real_audio_fixture(golden_dir)
    clip = fx["lr_sum_int16"].astype(np.float32) / np.float32(65536.0)
    y = _check_resample(clip, int(fx["sample_rate"]), 8000, "real clip 44100->8000")
    assert y.shape == (24000,)


def test_resample_determinism_batch_invariance_and_surface(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.resample import resample
    L = _lib.load()
    assert L.adn_resample_prepare(0, 44100, 8000) == 0
    assert L.adn_resample_prepare(0, 44100, 8000) == 0
    assert L.adn_resample_prepare(0, 44100, 44101) == 1
    assert L.adn_resample_prepare(99, 44100, 8000) == 1
    x = torch.from_numpy(np.random.default_rng(11).uniform(-1, 1, (64, 30011)).astype(np.float32)).to(dev)
    for src, dst in ((44100, 8000), (8000, 44100), (48000, 8000)):
        a, b = resample(x, src, dst), resample(x, src, dst)
        assert a.is_cuda and a.device == x.device and a.dtype == torch.float32
        assert torch.equal(a, b), (src, dst)
        for k in (0, 17, 63):
            alone = resample(x[k], src, dst)
            assert alone.dim() == 1 and torch.equal(alone, a[k]), (src, dst, k)
    # a rate pair this process has not seen: the call that builds the table gives the same bits as the next one
    first = resample(x[:2], 11025, 8000)
    assert torch.equal(first, resample(x[:2], 11025, 8000))
    xn = x[:2].cpu().numpy()
    yn = resample(xn, 44100, 8000)
    assert isinstance(yn, np.ndarray) and np.array_equal(yn, resample(x[:2], 44100, 8000).cpu().numpy())
    with pytest.raises(RuntimeError, match="ROCm device"):
        resample(x[:2].cpu(), 44100, 8000)
    with pytest.raises(TypeError):
        resample(x[:2].double(), 44100, 8000)
    with pytest.raises(_lib.AdnError):
        resample(x[:2], 44100, 44101)


def test_resample_cold_call_inside_a_capture_is_refused(dev):
    """adn.h: a cold adn_resample on a capturing stream enqueues nothing, returns ADN_ERR_INVALID and names
    adn_resample_prepare; after the prepare the same call is captured and replays."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.resample import prepare_resample, resample
    x = torch.from_numpy(np.random.default_rng(12).uniform(-1, 1, (4, 5000)).astype(np.float32)).to(dev)
    out = torch.empty((4, ref.resample_length(5000, 32000, 8000)), dtype=torch.float32, device=dev)
    L = _lib.load()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            rc_cold = L.adn_resample(x.data_ptr(), 4, 5000, 32000, 8000, out.data_ptr(), side.cuda_stream)
            msg = L.adn_last_error()
        finally:
            graph.capture_end()
    assert rc_cold == 1 and b"adn_resample_prepare" in msg
    prepare_resample(32000, 8000, dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            rc = L.adn_resample(x.data_ptr(), 4, 5000, 32000, 8000, out.data_ptr(), side.cuda_stream)
        finally:
            graph.capture_end()
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, resample(x, 32000, 8000))


# ---- mix_snr ------------------------------------------------------------------------------------------------------------------
def _check_mix(clean, noise, snr_db, what):
    from audiodenoiser_amd.resample import mix_snr
    out = mix_snr(clean, noise, snr_db)
    out_ref, s, scaled = ref.mix_snr_ref(clean, noise, snr_db)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == out_ref.shape
    err = np.abs(out.astype(np.float64) - out_ref)
    bound = 1e-5 * np.abs(scaled) + 3 * EPS * (np.abs(np.asarray(clean, np.float64)) + np.abs(scaled))
    share = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
    print(f"{what}: scale {np.ravel(s)[:3]}, max err {err.max():.3g}, largest share of the bound {share:.3f}")
    assert np.all(err <= bound), (what, float(err.max()), share)
    assert np.abs(out).max() <= 1.0
    return out, out_ref


@pytest.mark.parametrize("shape", ((16, 16000), (1, 1 << 22), (3, 24001)))
@pytest.mark.parametrize("snr_db", (8.0, 0.0, -5.0, 30.0))
def test_mix_snr_against_reference(dev, shape, snr_db):
    rng = np.random.default_rng([shape[0], shape[1], int(snr_db) + 100])
    t = np.arange(shape[1]) / 8000.0
    clean = (0.3 * np.sin(2 * np.pi * 220.0 * t)[None] * rng.uniform(0.2, 1.0, (shape[0], 1))).astype(np.float32)
    noise = rng.standard_normal(shape).astype(np.float32)
    _check_mix(clean, noise, snr_db, f"mix {shape} {snr_db} dB")


def test_mix_snr_silence_clipping_and_determinism(dev):
    from audiodenoiser_amd.resample import mix_snr
    rng = np.random.default_rng(21)
    clean = rng.uniform(-0.5, 0.5, (3, 24001)).astype(np.float32)
    noise = rng.standard_normal((3, 24001)).astype(np.float32)
    out, _ = _check_mix(clean * 3, np.zeros_like(noise), 8.0, "silent noise")          # out = clip(clean), some samples clip
    assert np.array_equal(out, np.clip(clean * 3, -1, 1))
    out, out_ref = _check_mix(np.zeros_like(clean), noise, 8.0, "silent clean")
    assert np.abs(out_ref).max() < 1e-5
    loud = (clean * 2.5).astype(np.float32)
    out, out_ref = _check_mix(loud, noise, 0.0, "loud clean")
    assert (np.abs(out_ref) == 1.0).sum() > 100 and (np.abs(out) == 1.0).sum() > 100
    c, n = torch.from_numpy(loud).to(dev), torch.from_numpy(noise).to(dev)
    a, b = mix_snr(c, n, 8.0), mix_snr(c, n, 8.0)
    assert a.is_cuda and torch.equal(a, b)
    assert torch.equal(mix_snr(c[1], n[1], 8.0), a[1])                                 # a clip alone = the clip in its batch
    with pytest.raises(RuntimeError, match="ROCm device"):
        mix_snr(c.cpu(), n.cpu(), 8.0)
    with pytest.raises(ValueError):
        mix_snr(c, n[:2], 8.0)


# ---- load_audio and the datasets -----------------------------------------------------------------------------------------------
def _speechlike(n, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(100, 3000, 3), rng.uniform(0, 6, 3)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 1.5 * t))).astype(np.float32)


def test_load_audio(dev, tmp_path):
    from audiodenoiser_amd.resample import load_audio, resample
    from audiodenoiser_amd.wav import read_wav, write_wav
    path = str(tmp_path / "stereo.wav")
    write_wav(path, np.stack([_speechlike(30000, 44100, 1), _speechlike(30000, 44100, 2)], axis=1), 44100, "PCM_16")
    audio, rate = load_audio(path, sr=8000)
    assert isinstance(audio, np.ndarray) and audio.dtype == np.float32 and rate == 8000
    assert audio.shape == (ref.resample_length(30000, 44100, 8000),)
    assert np.array_equal(audio, resample(read_wav(path)[0], 44100, 8000))
    raw, rate = load_audio(path, sr=None)
    assert rate == 44100 and np.array_equal(raw, read_wav(path)[0])
    same, rate = load_audio(path, sr=44100)
    assert rate == 44100 and np.array_equal(same, raw)
    both, rate = load_audio(path, sr=8000, mono=False)
    assert both.shape == (2, audio.shape[0]) and rate == 8000


def test_wav_dataset_with_resample(dev, tmp_path):
    from audiodenoiser_amd.data_loader import WavToSpecDataset
    from audiodenoiser_amd.resample import resample
    from audiodenoiser_amd.wav import read_wav, write_wav
    d44, d8 = tmp_path / "d44", tmp_path / "d8"
    d44.mkdir()
    d8.mkdir()
    for k in range(3):
        for side in ("clean", "noisy"):
            name = f"{side}_{k}.wav"
            write_wav(str(d44 / name), _speechlike(66150, 44100, 10 * k + (side == "noisy")), 44100, "PCM_16")
            write_wav(str(d8 / name), resample(read_wav(str(d44 / name))[0], 44100, 8000), 8000, "FLOAT")
    a = WavToSpecDataset(str(d44), sample_rate=8000, resample=True, device=dev)
    b = WavToSpecDataset(str(d8), sample_rate=8000, device=dev)
    assert len(a) == len(b) == 3
    for i in range(3):
        (an, ac), (bn, bc) = a[i], b[i]
        assert an.shape == (1, 256, 64) and not an.is_cuda and float(an.max()) > 0
        assert torch.equal(an, bn) and torch.equal(ac, bc)
    (an, ac), (bn, bc) = a.load_batch_to_device([2, 0, 1]), b.load_batch_to_device([2, 0, 1])
    assert an.is_cuda and an.shape == (3, 1, 256, 64)
    assert torch.equal(an, bn) and torch.equal(ac, bc)
    with pytest.raises(ValueError, match="no resampler in this build"):
        WavToSpecDataset(str(d44), sample_rate=8000, device=dev)[0]


def test_noise_mix_dataset(dev, tmp_path):
    from audiodenoiser_amd.data_loader import NoiseMixDataset
    from audiodenoiser_amd.stft import stft_magnitude_fit
    from audiodenoiser_amd.wav import read_wav, write_wav
    clean_dir, noise_dir = tmp_path / "clean", tmp_path / "noise"
    clean_dir.mkdir()
    noise_dir.mkdir()
    write_wav(str(clean_dir / "a.wav"), _speechlike(40000, 8000, 1), 8000, "FLOAT")          # 2 chunks of 16000 at 8 kHz
    write_wav(str(clean_dir / "b.wav"), _speechlike(200000, 44100, 2), 44100, "PCM_16")      # 36282 samples: 2 chunks
    write_wav(str(clean_dir / "c.wav"), _speechlike(100000, 44100, 3), 44100, "PCM_16")      # 18141 samples: 1 chunk
    write_wav(str(noise_dir / "n0.wav"), 0.2 * _speechlike(6000, 8000, 4), 8000, "FLOAT")    # shorter than a chunk: tiled
    write_wav(str(noise_dir / "n1.wav"), 0.2 * _speechlike(120000, 44100, 5), 44100, "PCM_16")   # longer: a random snippet
    types = ("white", "urban", "noise_cancellation")
    ds = NoiseMixDataset(str(clean_dir), str(noise_dir), noise_types=types, seed=7, device=dev)
    assert len(ds) == 5 * 3 and ds.chunk_samples == 16000
    n = ds.chunk_samples
    idx = list(range(len(ds)))
    noisy, clean = ds.audio_batch(idx)
    assert noisy.shape == clean.shape == (15, n) and noisy.is_cuda and clean.is_cuda
    noisy_h, clean_h = noisy.cpu().numpy().astype(np.float64), clean.cpu().numpy()

    def file_ref(path):
        audio, rate = read_wav(path)
        y, sum_abs, taps = ref.resample_ref(audio, rate, 8000)
        return y, (_resample_bound(sum_abs, taps) if rate != 8000 else np.zeros_like(y))
    clean_ref = [file_ref(p) for p in ds.clean_files]
    noise_ref = [file_ref(p) for p in ds.noise_files]
    used_files, used_snippet = set(), False
    for i in idx:
        plan = ds.item_plan(i)
        c_all, ec_all = clean_ref[plan["clean_file"]]
        c, ec = ref.frame_audio(c_all, n)[plan["chunk"]], ref.frame_audio(ec_all, n)[plan["chunk"]]
        assert np.all(np.abs(clean_h[i] - c) <= ec), ("clean chunk", i)
        if plan["noise_type"] == "noise_cancellation":
            assert np.array_equal(noisy[i].cpu().numpy(), ref.noise_cancellation_ref(clean_h[i], plan["coins"])), i
            continue
        if plan["noise_type"] == "white":
            nz = ds.white_noise(i).cpu().numpy().astype(np.float64)
            en = np.zeros(n)
            assert abs(nz.std() - 1.0) < 0.05 and abs(nz.mean()) < 0.05
        else:
            nz_all, en_all = noise_ref[plan["noise_file"]]
            nz = ref.match_audio_length(nz_all, n, plan["noise_start"])
            en = ref.match_audio_length(en_all, n, plan["noise_start"])
            used_files.add(plan["noise_file"])
            used_snippet |= plan["noise_start"] is not None
        out_ref, s, scaled = ref.mix_snr_ref(c, nz, 8.0)
        s = float(s[0])
        c_rms, n_rms = np.sqrt(np.mean(c ** 2) + 1e-12), np.sqrt(np.mean(nz ** 2) + 1e-12)
        # the mixer's own bound, plus what the resampler's error in its inputs can move: the samples themselves and, through
        # the two RMS values, the scale (an RMS moves by at most the RMS of the error)
        rel_scale = 1.01 * (np.sqrt(np.mean(ec ** 2)) / c_rms + np.sqrt(np.mean(en ** 2)) / n_rms)
        bound = (1e-5 * np.abs(scaled) + 3 * EPS * (np.abs(c) + np.abs(scaled))) + ec + s * en + np.abs(scaled) * rel_scale
        err = np.abs(noisy_h[i] - out_ref)
        print(f"item {i} {plan['noise_type']}: max err {err.max():.3g}, largest share of the bound {(err / bound).max():.3f}")
        assert np.all(err <= bound), (i, plan, float(err.max()))
    assert used_files == {0, 1} and used_snippet, "the seed must exercise both the tiled and the snippet noise file"
    spec_noisy, spec_clean = ds.load_batch_to_device(idx)
    assert spec_noisy.shape == (15, 1, 256, 64) and spec_noisy.is_cuda
    assert torch.equal(spec_noisy, stft_magnitude_fit(noisy, (256, 64), 512, 128, False))
    assert torch.equal(spec_clean, stft_magnitude_fit(clean, (256, 64), 512, 128, False))
    again_noisy, again_clean = ds.audio_batch(idx)
    assert torch.equal(again_noisy, noisy) and torch.equal(again_clean, clean)
    for i in (0, 4, 8, 14):
        item_noisy, item_clean = ds[i]
        assert item_noisy.shape == (1, 256, 64) and not item_noisy.is_cuda
        assert torch.equal(item_noisy, spec_noisy[i].cpu()) and torch.equal(item_clean, spec_clean[i].cpu())
    ds.set_epoch(1)
    other_noisy, other_clean = ds.audio_batch(idx)
    assert torch.equal(other_clean, clean) and not torch.equal(other_noisy, noisy)
