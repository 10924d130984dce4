"""Device reverb (adn_reverb) and the dataset opt-in built on it against the per-sample restatement tests/reverb_ref.py.

The tolerance is measured per case, not chosen: e32 = max|ref_fp32 - ref_fp64| / max|ref_fp64| is the rounding floor of the
plain sequential fp32 loop on that very input, and the kernel must stay within max(4 * e32, 2^-22) of ref_fp64 on the same scale.
The factor 4 covers the re-association inside the kernel's scan; 2^-22 is four fp32 roundings of the output for cases where e32
happens to come out tiny.  Every sample is compared (clipping is 1-Lipschitz).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref  # noqa: E402
import reverb_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _gated_tone(length, rate, seed, amp=0.4, noise=0.05):
    """A 220 Hz tone gated on and off every quarter second plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(length) / rate
    return (amp * np.sin(2 * np.pi * 220.0 * t) * ((t % 0.5) < 0.25) + noise * rng.standard_normal(length)).astype(np.float32)


def _check(x, rate, what, clip=True, **params):
    """Run the device reverb on ``x`` ((L,) or (B, L) float32), compare every clip with the float64 reference under the
    measured bound of the module docstring.  -> (device result as numpy, worst e32, worst kernel error)."""
    from audiodenoiser_amd.reverb import reverb
    y = reverb(x, rate, clip=clip, **params)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == x.shape, what
    worst32 = worst = 0.0
    for k, (row, out) in enumerate(zip(np.atleast_2d(x), np.atleast_2d(y))):
        r64 = ref.reverb_ref(row, rate, clip=clip, dtype=np.float64, **params)
        r32 = ref.reverb_ref(row, rate, clip=clip, dtype=np.float32, **params)
        scale = np.abs(r64).max()
        if scale == 0:
            assert np.all(out == 0), (what, k)
            continue
        e32 = float(np.abs(r32.astype(np.float64) - r64).max() / scale)
        err = float(np.abs(out.astype(np.float64) - r64).max() / scale)
        bound = max(4 * e32, 2.0 ** -22)
        print(f"{what} clip {k}: {len(row)} samples, scale {scale:.3g}, e32 {e32:.3g}, kernel {err:.3g}, bound {bound:.3g}")
        worst32, worst = max(worst32, e32), max(worst, err)
        assert err <= bound, (what, k, err, e32, bound)
    return y, worst32, worst


@pytest.mark.parametrize("rate,length", ((8000, 16000), (16000, 8000), (44100, 20000), (48000, 12000)))
def test_reverb_against_reference(dev, rate, length):
    y, _, _ = _check(_gated_tone(length, rate, rate + length), rate, f"{rate} Hz x {length}")
    assert np.abs(y - 0.8 * _gated_tone(length, rate, rate + length)).max() > 1e-3          # the wet path is audible in it


@pytest.mark.parametrize("rate", (2000, 4000, 12739, 12740, 96000, 128000))
def test_reverb_rate_range(dev, rate):
    """The ends of the supported range, the documented least range, and the two rates either side of the kernel's switch from
    one wave per clip to eight (shortest delay 64 / 65)."""
    length = 3 * min(sum(ref.delay_lengths(rate), [])) + 2 * max(sum(ref.delay_lengths(rate), [])) + 17
    _check(_gated_tone(length, rate, rate), rate, f"{rate} Hz x {length}")


@pytest.mark.parametrize("rate,length", ((8000, 1), (8000, 39), (8000, 40), (8000, 41), (44100, 224), (44100, 1)))
def test_reverb_short_clips(dev, rate, length):
    """Shorter than the shortest delay (one partial chunk), exactly one chunk, one sample more, a single sample."""
    x = np.random.default_rng(length).uniform(-0.9, 0.9, length).astype(np.float32)
    y, _, _ = _check(x, rate, f"{rate} Hz x {length}")
    assert np.array_equal(y, (x * (np.float32(0.4) * np.float32(2.0))).astype(np.float32))   # nothing has come back yet: dry only


def test_reverb_tail_after_a_burst(dev):
    x = np.zeros(2000 + 8000, dtype=np.float32)
    x[:2000] = _gated_tone(2000, 8000, 5, amp=0.8)
    y, _, _ = _check(x, 8000, "burst + 1 s of silence")
    assert np.abs(y[-800:]).max() > 1e-4                      # room_size 0.9: the tail is still there after a second


@pytest.mark.parametrize("params", (
    dict(dry_level=0.0, wet_level=1.0),
    dict(room_size=0.0, damping=0.0), dict(room_size=1.0, damping=1.0), dict(room_size=0.0, damping=1.0),
    dict(room_size=1.0, damping=0.0), dict(width=0.0), dict(wet_level=0.0), dict(room_size=0.5, damping=0.25, wet_level=0.7,
                                                                               dry_level=0.9, width=0.3)))
def test_reverb_parameters(dev, params):
    x = _gated_tone(6000, 8000, 9)
    y, _, _ = _check(x, 8000, f"8000 Hz {params}", **params)
    if params.get("dry_level") == 0.0:
        assert np.all(y[:202] == 0) and np.abs(y[202:]).max() > 0.01        # the wet path alone, first echo at the first comb delay
    if params.get("wet_level") == 0.0:
        assert np.array_equal(y, (x * np.float32(0.8)).astype(np.float32))


def test_reverb_clip_on_and_off(dev):
    x = _gated_tone(6000, 8000, 13, amp=0.95)
    on, _, _ = _check(x, 8000, "clip on", clip=True, dry_level=1.0, wet_level=1.0)
    off, _, _ = _check(x, 8000, "clip off", clip=False, dry_level=1.0, wet_level=1.0)
    assert np.abs(off).max() > 1.5 and np.abs(on).max() == 1.0 and (np.abs(on) == 1.0).sum() > 100
    assert np.array_equal(on, np.clip(off, -1.0, 1.0))


def test_reverb_batch_of_mixed_clips(dev):
    rng = np.random.default_rng(37)
    rows = []
    for k in range(37):
        kind = k % 4
        if kind == 0:
            row = _gated_tone(4000, 8000, 100 + k, amp=rng.uniform(0.1, 0.9))
        elif kind == 1:
            row = rng.uniform(-1.0, 1.0, 4000).astype(np.float32)
        elif kind == 2:
            row = np.zeros(4000, dtype=np.float32)
            row[rng.integers(0, 4000, 5)] = rng.uniform(-1, 1, 5)
        else:
            row = np.zeros(4000, dtype=np.float32) if k == 3 else (1e-3 * rng.standard_normal(4000)).astype(np.float32)
        rows.append(row)
    _check(np.stack(rows), 8000, "37 mixed clips")


def test_reverb_determinism_batch_invariance_in_place_and_surface(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.reverb import reverb
    L = _lib.load()
    for rate, n in ((8000, 16000), (44100, 9001)):
        x = torch.from_numpy(np.stack([_gated_tone(n, rate, 200 + k, amp=0.1 + 0.02 * k) for k in range(37)])).to(dev)
        a, b = reverb(x, rate), reverb(x, rate)
        assert a.is_cuda and a.device == x.device and a.dtype == torch.float32 and a.shape == x.shape
        assert a.data_ptr() != x.data_ptr() and torch.equal(a, b), rate
        for k in (0, 17, 36):
            alone = reverb(x[k], rate)
            assert alone.dim() == 1 and torch.equal(alone, a[k]), (rate, k)
        assert torch.equal(reverb(x[5:9], rate), a[5:9]), rate
        # in place through the C ABI: out == audio
        y = x.clone()
        stream = torch.cuda.current_stream(dev).cuda_stream
        assert L.adn_reverb(y.data_ptr(), 37, n, rate, 0.9, 0.9, 0.33, 0.4, 1.0, 1, y.data_ptr(), stream) == 0
        assert torch.equal(y, a), rate
        yn = reverb(x[:2].cpu().numpy(), rate)
        assert isinstance(yn, np.ndarray) and np.array_equal(yn, a[:2].cpu().numpy())
    with pytest.raises(RuntimeError, match="ROCm device"):
        reverb(x[:2].cpu(), 8000)
    with pytest.raises(TypeError):
        reverb(x[:2].double(), 8000)
    with pytest.raises(ValueError):
        reverb(x[None], 8000)


def test_reverb_invalid_arguments_launch_nothing(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.reverb import reverb
    L = _lib.load()
    x = torch.from_numpy(_gated_tone(4000, 8000, 1)).to(dev)[None].contiguous()
    out = torch.full_like(x, 7.0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(n_clips=1, length=4000, rate=8000, par=(0.9, 0.9, 0.33, 0.4, 1.0), audio=x.data_ptr(), dst=out.data_ptr()):
        return L.adn_reverb(audio, n_clips, length, rate, *par, 1, dst, stream)
    assert call(audio=None) == 1 and call(dst=None) == 1 and call(n_clips=0) == 1 and call(length=0) == 1
    assert call(rate=1999) == 1 and call(rate=128001) == 1 and call(rate=0) == 1
    for k in range(5):
        for bad in (-0.5, 1.5, float("nan")):
            par = [0.9, 0.9, 0.33, 0.4, 1.0]
            par[k] = bad
            assert call(par=tuple(par)) == 1, (k, bad)
    torch.cuda.synchronize(dev)
    assert torch.all(out == 7.0)                               # nothing was written
    with pytest.raises(_lib.AdnError):
        reverb(x, 1000)
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert not torch.any(out == 7.0)


# ---- the dataset opt-in ------------------------------------------------------------------------------------------------------
def _speechlike(n, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(100, 3000, 3), rng.uniform(0, 6, 3)))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 1.5 * t))).astype(np.float32)


def _resample_bound(sum_abs, taps):
    return 1.01 * (taps + 2) * EPS * sum_abs


def test_noise_mix_dataset_with_reverb(dev, tmp_path):
    """All four noise types of the reference in one dataset.  The reverb items are the clipped reference of their own clean
    chunk under the measured bound; white / urban / noise_cancellation items are checked as tests/test_gpu_resample.py checks
    them (same bounds); the spectrogram batch is the STFT of exactly the audio batch."""
    from audiodenoiser_amd.data_loader import NoiseMixDataset
    from audiodenoiser_amd.reverb import ReverbSettings
    from audiodenoiser_amd.stft import stft_magnitude_fit
    from audiodenoiser_amd.wav import read_wav, write_wav
    clean_dir, noise_dir = tmp_path / "clean", tmp_path / "noise"
    clean_dir.mkdir()
    noise_dir.mkdir()
    write_wav(str(clean_dir / "a.wav"), _speechlike(40000, 8000, 1), 8000, "FLOAT")          # 2 chunks of 16000 at 8 kHz
    write_wav(str(clean_dir / "b.wav"), _speechlike(100000, 44100, 3), 44100, "PCM_16")      # 18141 samples: 1 chunk
    write_wav(str(noise_dir / "n0.wav"), 0.2 * _speechlike(6000, 8000, 4), 8000, "FLOAT")    # shorter than a chunk: tiled
    write_wav(str(noise_dir / "n1.wav"), 0.2 * _speechlike(120000, 44100, 5), 44100, "PCM_16")   # longer: a random snippet
    types = ("white", "urban", "noise_cancellation", "reverb")
    ds = NoiseMixDataset(str(clean_dir), str(noise_dir), noise_types=types, seed=7, device=dev, reverb=True)
    assert len(ds) == 3 * 4 and ds.chunk_samples == 16000
    n = ds.chunk_samples
    idx = list(range(len(ds)))
    noisy, clean = ds.audio_batch(idx)
    assert noisy.shape == clean.shape == (12, n) and noisy.is_cuda and clean.is_cuda
    noisy_h, clean_h = noisy.cpu().numpy().astype(np.float64), clean.cpu().numpy()
    # the clean halves: what a dataset without the type hands out for the same chunks, bit for bit
    plain = NoiseMixDataset(str(clean_dir), str(noise_dir), noise_types=types[:3], seed=7, device=dev)
    _, plain_clean = plain.audio_batch(list(range(len(plain))))
    for i in idx:
        assert torch.equal(clean[i], plain_clean[(i // 4) * 3]), i

    def file_ref(path):
        audio, rate = read_wav(path)
        y, sum_abs, taps = resample_ref.resample_ref(audio, rate, 8000)
        return y, (_resample_bound(sum_abs, taps) if rate != 8000 else np.zeros_like(y))
    clean_ref = [file_ref(p) for p in ds.clean_files]
    noise_ref = [file_ref(p) for p in ds.noise_files]
    seen = set()
    for i in idx:
        plan = ds.item_plan(i)
        seen.add(plan["noise_type"])
        c_all, ec_all = clean_ref[plan["clean_file"]]
        c, ec = resample_ref.frame_audio(c_all, n)[plan["chunk"]], resample_ref.frame_audio(ec_all, n)[plan["chunk"]]
        assert np.all(np.abs(clean_h[i] - c) <= ec), ("clean chunk", i)
        if plan["noise_type"] == "reverb":
            r64 = ref.reverb_ref(clean_h[i], 8000, clip=True, dtype=np.float64)
            r32 = ref.reverb_ref(clean_h[i], 8000, clip=True, dtype=np.float32)
            scale = np.abs(r64).max()
            e32 = float(np.abs(r32 - r64).max() / scale)
            err = float(np.abs(noisy_h[i] - r64).max() / scale)
            print(f"item {i} reverb: e32 {e32:.3g}, kernel {err:.3g}, bound {max(4 * e32, 2.0 ** -22):.3g}")
            assert err <= max(4 * e32, 2.0 ** -22), (i, err, e32)
            assert np.abs(noisy_h[i]).max() <= 1.0 and np.abs(noisy_h[i] - clean_h[i]).max() > 1e-2
            continue
        if plan["noise_type"] == "noise_cancellation":
            assert np.array_equal(noisy[i].cpu().numpy(), resample_ref.noise_cancellation_ref(clean_h[i], plan["coins"])), i
            continue
        if plan["noise_type"] == "white":
            nz = ds.white_noise(i).cpu().numpy().astype(np.float64)
            en = np.zeros(n)
            assert abs(nz.std() - 1.0) < 0.05 and abs(nz.mean()) < 0.05
        else:
            nz_all, en_all = noise_ref[plan["noise_file"]]
            nz = resample_ref.match_audio_length(nz_all, n, plan["noise_start"])
            en = resample_ref.match_audio_length(en_all, n, plan["noise_start"])
        out_ref, s, scaled = resample_ref.mix_snr_ref(c, nz, 8.0)
        s = float(s[0])
        c_rms, n_rms = np.sqrt(np.mean(c ** 2) + 1e-12), np.sqrt(np.mean(nz ** 2) + 1e-12)
        rel_scale = 1.01 * (np.sqrt(np.mean(ec ** 2)) / c_rms + np.sqrt(np.mean(en ** 2)) / n_rms)
        bound = (1e-5 * np.abs(scaled) + 3 * EPS * (np.abs(c) + np.abs(scaled))) + ec + s * en + np.abs(scaled) * rel_scale
        err = np.abs(noisy_h[i] - out_ref)
        print(f"item {i} {plan['noise_type']}: max err {err.max():.3g}, largest share of the bound {(err / bound).max():.3f}")
        assert np.all(err <= bound), (i, plan, float(err.max()))
    assert seen == set(types)
    spec_noisy, spec_clean = ds.load_batch_to_device(idx)
    assert spec_noisy.shape == (12, 1, 256, 64) and spec_noisy.is_cuda
    assert torch.equal(spec_noisy, stft_magnitude_fit(noisy, (256, 64), 512, 128, False))
    assert torch.equal(spec_clean, stft_magnitude_fit(clean, (256, 64), 512, 128, False))
    again_noisy, again_clean = ds.audio_batch(idx)
    assert torch.equal(again_noisy, noisy) and torch.equal(again_clean, clean)
    for i in (3, 7, 11):
        item_noisy, item_clean = ds[i]
        assert torch.equal(item_noisy, spec_noisy[i].cpu()) and torch.equal(item_clean, spec_clean[i].cpu())
    # reverb items use no draw: another epoch moves the other types' items and leaves these alone; other settings move them
    ds.set_epoch(1)
    other_noisy, _ = ds.audio_batch(idx)
    assert torch.equal(other_noisy[3::4], noisy[3::4]) and not torch.equal(other_noisy[0::4], noisy[0::4])
    small = NoiseMixDataset(str(clean_dir), str(noise_dir), noise_types=types, seed=7, device=dev,
                            reverb=ReverbSettings(room_size=0.2, wet_level=0.1))
    small_noisy, small_clean = small.audio_batch(idx)
    assert torch.equal(small_clean, clean) and torch.equal(small_noisy[0::4], noisy[0::4])
    assert not torch.equal(small_noisy[3::4], noisy[3::4])
    only = NoiseMixDataset(str(clean_dir), str(noise_dir), noise_types=("reverb",), seed=1, device=dev, reverb=True)
    only_noisy, _ = only.audio_batch([0, 1, 2])
    assert torch.equal(only_noisy, noisy[3::4])
