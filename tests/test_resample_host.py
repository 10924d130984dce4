"""Host-side checks of the resampler / SNR mixer feature: the filter the definition in include/adn.h yields (through its
float64 restatement tests/resample_ref.py), that restatement against scipy, the host-only C entry points, and the
dataset logic of NoiseMixDataset that needs no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref  # noqa: E402

RATE_PAIRS = ((44100, 8000), (8000, 44100), (48000, 8000), (22050, 8000), (16000, 8000), (8000, 16000))
IN_BAND_HZ = (50, 100, 500, 1000, 1500, 2000, 2500, 3000)
STOP_BAND_HZ = (4000, 4010, 4050, 4100, 4300, 5000, 7000, 7900, 8100, 11000, 15000, 19000, 21000)


@pytest.mark.parametrize("src", (44100, 48000))
def test_filter_pass_band_and_stop_band(src):
    """0.5 s unit cosines -> 8 kHz, RMS of the middle half of the output against sqrt(1/2)."""
    n = src // 2
    t = np.arange(n) / src
    worst_pass, worst_stop = 0.0, -np.inf
    for f in IN_BAND_HZ + STOP_BAND_HZ:
        y, _, _ = ref.resample_ref(np.cos(2 * np.pi * f * t), src, 8000)
        mid = y[len(y) // 4: len(y) - len(y) // 4]
        gain = np.sqrt(np.mean(mid ** 2)) / np.sqrt(0.5)
        if f in IN_BAND_HZ:
            worst_pass = max(worst_pass, abs(gain - 1.0))
        else:
            worst_stop = max(worst_stop, 20 * np.log10(max(gain, 1e-300)))
    print(f"{src} -> 8000: worst |gain - 1| in band {worst_pass:.3g}, worst stop-band gain {worst_stop:.1f} dB")
    assert worst_pass <= 1e-5
    assert worst_stop <= -110.0


@pytest.mark.parametrize("src,dst", RATE_PAIRS)
def test_reference_equals_scipy_resample_poly(src, dst):
    signal = pytest.importorskip("scipy.signal")
    up, down = ref.ratio(src, dst)
    x = np.random.default_rng(src + dst).uniform(-1, 1, (3, 4001))
    y, _, _ = ref.resample_ref(x, src, dst)
    ys = signal.resample_poly(x, up, down, axis=1, window=ref.design(up, down) / up)
    assert ys.shape == y.shape
    err = np.abs(ys - y).max()
    print(f"{src} -> {dst}: max |resample_ref - resample_poly| = {err:.3g}")
    assert err <= 1e-12


def test_resample_length_and_argument_errors():
    from audiodenoiser_amd import _lib
    L = _lib.load()
    out = ctypes.c_long()
    for src, dst in RATE_PAIRS:
        up, down = ref.ratio(src, dst)
        for length in (1, 441, 442, 132300):
            assert L.adn_resample_length(length, src, dst, ctypes.byref(out)) == 0
            assert out.value == -(-length * up // down) == ref.resample_length(length, src, dst)
    assert L.adn_resample_length(100, 8000, 8000, ctypes.byref(out)) == 0 and out.value == 100
    assert L.adn_resample_length(100, 0, 8000, ctypes.byref(out)) == 1             # ADN_ERR_INVALID
    assert L.adn_resample_length(100, 8000, 0, ctypes.byref(out)) == 1
    assert L.adn_resample_length(100, 44100, 44101, ctypes.byref(out)) == 1        # max(up, down) > 4096
    assert b"4096" in L.adn_last_error()
    assert L.adn_resample_length(0, 44100, 8000, ctypes.byref(out)) == 1
    assert L.adn_resample_length(100, 44100, 8000, None) == 1
    assert L.adn_resample_length(1 << 40, 8000, 44100, ctypes.byref(out)) == 1     # M >= 2^31
    assert L.adn_resample(None, 1, 100, 44100, 8000, None, None) == 1
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.adn_resample(p, 1, 16, 44100, 8000, p, None) == 1                     # out aliases audio
    assert L.adn_resample(p, 0, 16, 44100, 8000, None, None) == 1
    assert L.adn_resample_prepare(0, 44100, 44101) == 1
    need = ctypes.c_size_t()
    assert L.adn_mix_snr_workspace_bytes(0, 16000, ctypes.byref(need)) == 1
    assert L.adn_mix_snr_workspace_bytes(4, 0, ctypes.byref(need)) == 1
    assert L.adn_mix_snr_workspace_bytes(4, 16000, None) == 1
    assert L.adn_mix_snr_workspace_bytes(4, 16000, ctypes.byref(need)) == 0 and need.value % 4 == 0
    assert L.adn_mix_snr(None, None, 1, 16, 8.0, None, 0, None, None) == 1
    assert L.adn_mix_snr(p, p, 1, 16, 8.0, p, 64, p, None) == 1                    # out aliases clean


def _tone(n, f, rate, amp=0.5):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / rate)).astype(np.float32)


@pytest.fixture()
def mix_dirs(tmp_path):
    from audiodenoiser_amd.wav import write_wav
    clean, noise = tmp_path / "clean", tmp_path / "noise"
    clean.mkdir()
    noise.mkdir()
    # at 8 kHz with 0.25 s chunks (2000 samples): a -> 5000 samples (2 chunks), b -> 44100 -> 8000 samples (4), c -> 1999 (0)
    write_wav(str(clean / "a.wav"), _tone(5000, 440, 8000), 8000, "FLOAT")
    write_wav(str(clean / "b.WAV"), np.stack([_tone(44100, 300, 44100), _tone(44100, 500, 44100)], axis=1), 44100)
    write_wav(str(clean / "c.wav"), _tone(1999, 200, 8000), 8000)
    (clean / "notes.txt").write_text("not audio")
    write_wav(str(noise / "n0.wav"), _tone(1200, 1000, 8000, 0.1), 8000, "FLOAT")          # shorter than a chunk: tiled
    write_wav(str(noise / "n1.wav"), _tone(22050, 700, 22050, 0.1), 22050)                 # 8000 samples: random snippet
    return str(clean), str(noise)


def test_noise_mix_dataset_host_logic(mix_dirs):
    from audiodenoiser_amd.data_loader import NoiseMixDataset
    from audiodenoiser_amd.wav import wav_info
    clean_dir, noise_dir = mix_dirs
    assert wav_info(os.path.join(clean_dir, "b.WAV")) == (44100, 2, 44100)
    types = ("white", "urban", "noise_cancellation")
    ds = NoiseMixDataset(clean_dir, noise_dir, noise_types=types, sample_rate=8000, chunk_seconds=0.25, seed=3)
    assert [os.path.basename(p) for p in ds.clean_files] == ["a.wav", "b.WAV", "c.wav"]
    assert [os.path.basename(p) for p in ds.noise_files] == ["n0.wav", "n1.wav"]
    assert ds.chunk_samples == 2000
    assert ds.clean_lengths == [5000, 8000, 1999] and ds.noise_lengths == [1200, 8000]
    assert ds.chunks == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 3)]           # tails (1000, 0, 1999 samples) dropped
    assert len(ds) == 6 * 3
    for i in range(len(ds)):
        plan = ds.item_plan(i)
        assert (plan["clean_file"], plan["chunk"]) == ds.chunks[i // 3] and plan["noise_type"] == types[i % 3]
        assert plan["noise_file"] in (0, 1) and len(plan["coins"]) == 1
        if plan["noise_file"] == 1:
            assert 0 <= plan["noise_start"] < 8000 - 2000
        else:
            assert plan["noise_start"] is None
    with pytest.raises(IndexError):
        ds.item_plan(len(ds))
    again = NoiseMixDataset(clean_dir, noise_dir, noise_types=types, sample_rate=8000, chunk_seconds=0.25, seed=3)
    plans = [ds.item_plan(i) for i in range(len(ds))]
    assert plans == [again.item_plan(i) for i in range(len(ds))]
    assert len({(p["noise_file"], p["noise_start"], p["white_seed"]) for p in plans}) > len(ds) // 2       # items differ
    again.set_epoch(1)
    other = [again.item_plan(i) for i in range(len(ds))]
    assert all(a["white_seed"] != b["white_seed"] for a, b in zip(plans, other))
    assert [(p["clean_file"], p["chunk"], p["noise_type"]) for p in other] == [(p["clean_file"], p["chunk"], p["noise_type"]) for p in plans]
    other_seed = NoiseMixDataset(clean_dir, noise_dir, noise_types=types, sample_rate=8000, chunk_seconds=0.25, seed=4)
    assert all(a["white_seed"] != other_seed.item_plan(i)["white_seed"] for i, a in enumerate(plans))
    with pytest.raises(ValueError, match="Pedalboard"):
        NoiseMixDataset(clean_dir, noise_dir, noise_types=("white", "reverb"))
    with pytest.raises(ValueError, match="noise_types"):
        NoiseMixDataset(clean_dir, noise_dir, noise_types=("pink",))
    # the reference's defaults: 2 s chunks at 8 kHz -> only b.WAV (8000 samples) is too short as well: nothing left
    assert len(NoiseMixDataset(clean_dir, noise_dir)) == 0


def test_wav_dataset_rate_mismatch_still_raises(tmp_path):
    from audiodenoiser_amd.data_loader import WavToSpecDataset
    from audiodenoiser_amd.wav import write_wav
    for name in ("clean_0.wav", "noisy_0.wav"):
        write_wav(str(tmp_path / name), _tone(44100, 440, 44100), 44100)
    ds = WavToSpecDataset(str(tmp_path), sample_rate=8000)
    assert ds.resample is False
    with pytest.raises(ValueError, match=r"sample rate 44100 != expected 8000 \(no resampler in this build\)"):
        ds._audio(ds.pairs[0][0])
    with pytest.raises(ValueError, match="no resampler in this build"):
        ds.audio_view(16000)[0]
    with pytest.raises(ValueError, match="sample_rate"):
        WavToSpecDataset(str(tmp_path), resample=True)
    rs = WavToSpecDataset(str(tmp_path), sample_rate=8000, resample=True)
    for call in (lambda: rs.audio_view(16000), lambda: rs.loader(16000, batch_size=1), lambda: rs.to_device_batch((None, None))):
        with pytest.raises(ValueError, match="resample=True"):
            call()


def test_resample_surface_refuses_cpu_tensors():
    import torch
    from audiodenoiser_amd import resample as rs
    with pytest.raises(RuntimeError, match="ROCm device"):
        rs.resample(torch.zeros(100), 44100, 8000)
    with pytest.raises(RuntimeError, match="ROCm device"):
        rs.mix_snr(torch.zeros(100), torch.zeros(100))
    assert rs.resample_length(176400, 44100, 8000) == 32000
    if not torch.cuda.is_available():                      # no CPU arithmetic path: numpy input has nowhere to go either
        from audiodenoiser_amd._lib import AdnError
        with pytest.raises(AdnError, match="no ROCm device"):
            rs.resample(np.zeros(100, np.float32), 44100, 8000)
