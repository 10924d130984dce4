"""The cases of the spectral-baseline tests (tests/test_baseline_host.py, tests/test_gpu_baseline.py) -- TEST INFRASTRUCTURE.
The test signal is written down as code so that it is the same everywhere; everything is seeded.

    python tests/baseline_cases.py          measures the float32 host floor over the GPU parity cases and the SI-SDR figures of the
                                            restatement, writes FLOOR into tests/baseline_ref.py and both into the marked block of
                                            profiles/bench_baseline.md
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_ref as br  # noqa: E402
import denoise_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000

# GPU parity cases: F = 33 (less than a wave), 257 (four waves + 1 lane), 513 (eight waves + 1 lane); hop = n_fft / 4; the frame
# counts sit around the kernel's tile of 32 frames, 97 is past three tiles; 1 clip and 3 clips
PARITY_N_FFT = (64, 512, 1024)
PARITY_FRAMES = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 97, 188)
PARITY_CLIPS = (1, 3)
TILE = 32                                   # frames per LDS tile of csrc/baseline_kernels.hip (BL_TF)


def speech_like(n_samples, seed, sr=SR):
    """Speech-like bursts, float64: bursts of 0.15-0.5 s separated by gaps of 0.05-0.3 s; a burst is a Hann-enveloped sum of the
    harmonics k = 1..13 of an f0 in [100, 250] Hz with amplitudes k^-1.2 and a 3 Hz vibrato of +-10 %; peak 0.3."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n_samples)
    pos = int(rng.uniform(0.0, 0.1) * sr)
    while pos < n_samples:
        n = int(rng.uniform(0.15, 0.5) * sr)
        f0 = rng.uniform(100.0, 250.0)
        t = np.arange(n) / sr
        # phase of a tone whose frequency is f0 (1 + 0.1 sin(2 pi 3 t)): the integral of the frequency
        phase = 2.0 * np.pi * f0 * (t - 0.1 * (np.cos(2.0 * np.pi * 3.0 * t) - 1.0) / (2.0 * np.pi * 3.0))
        burst = sum(k ** -1.2 * np.sin(k * phase + rng.uniform(0.0, 2.0 * np.pi)) for k in range(1, 14))
        burst = burst * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / max(n - 1, 1)))
        m = min(n, n_samples - pos)
        x[pos:pos + m] = burst[:m]
        pos += n + int(rng.uniform(0.05, 0.3) * sr)
    peak = np.abs(x).max()
    return x * (0.3 / peak) if peak > 0 else x


def mix(clean, noise, snr_db):
    """The reference's rule for its "white" and "urban" mixes: the noise scaled so that rms(clean) / rms(noise) = 10^(snr / 20),
    each rms as sqrt(mean square + 1e-12), the sum clipped to [-1, 1]."""
    clean_rms = np.sqrt(np.mean(clean ** 2) + 1e-12)
    noise_rms = np.sqrt(np.mean(noise ** 2) + 1e-12)
    scaled = noise * (clean_rms / 10.0 ** (snr_db / 20.0) / noise_rms) if noise_rms > 1e-9 else np.zeros_like(clean)
    return np.clip(clean + scaled, -1.0, 1.0)


def white_mix(n_samples, snr_db, seed):
    """-> (noisy float32, clean float32): the burst signal and its seeded white mix."""
    clean = speech_like(n_samples, seed)
    noise = np.random.default_rng([seed, 1]).standard_normal(n_samples)
    return mix(clean, noise, snr_db).astype(np.float32), clean.astype(np.float32)


def parity_length(n_fft, n_frames):
    hop = n_fft // 4
    return hop * (n_frames - 1) + hop // 2          # T = 1 + L // hop


def parity_audio(n_fft, n_frames, n_clips):
    """(n_clips, L) float32: white mixes at 8, 0 and 15 dB of three different burst signals."""
    length = parity_length(n_fft, n_frames)
    return np.stack([white_mix(length, (8.0, 0.0, 15.0)[c], 1000 * n_fft + 10 * n_frames + c)[0] for c in range(n_clips)])


def floor_of(spec):
    """max|M32 - M64| / max M64 of one clip's (T, F) spectrogram (complex64 values)."""
    m64, _ = br.spectral_gain(spec, dtype=np.float64)
    m32, _ = br.spectral_gain(spec, dtype=np.float32)
    return float(np.abs(m32.astype(np.float64) - m64).max() / m64.max())


def measure_floor(verbose=False):
    worst = 0.0
    for n_fft in PARITY_N_FFT:
        for n_frames in PARITY_FRAMES:
            x = parity_audio(n_fft, n_frames, 3)
            for c in range(3):
                spec = denoise_ref.stft(x[c], n_fft, n_fft // 4).astype(np.complex64)
                f = floor_of(spec)
                worst = max(worst, f)
                if verbose:
                    print(f"n_fft {n_fft} T {n_frames} clip {c}: {f:.3g}")
    return worst


def quality_case(snr_db=8.0, seconds=6.0, seed=7):
    """The quality mix: 6 s of the burst signal with white noise at `snr_db`."""
    return white_mix(int(seconds * SR), snr_db, seed)


def restatement_si_sdr(snr_db):
    noisy, clean = quality_case(snr_db)
    out = br.denoise(noisy.astype(np.float64), 512, 128)
    return br.si_sdr(noisy, clean), br.si_sdr(out, clean)


def main():
    floor = measure_floor(verbose=True)
    text = f"{floor:.1e}"
    path = os.path.join(ROOT, "tests", "baseline_ref.py")
    src = open(path).read()
    src, n = re.subn(r"^FLOOR = .*$", f"FLOOR = {text}", src, flags=re.M)
    assert n == 1
    open(path, "w").write(src)
    rows = [f"| {snr:g} dB | {a:.1f} dB | {b:.1f} dB | {b - a:+.1f} dB |" for snr in (0.0, 8.0, 15.0) for a, b in (restatement_si_sdr(snr),)]
    block = (f"Float32 host floor (worst max|M32 - M64| / max M64 per clip over the {len(PARITY_N_FFT) * len(PARITY_FRAMES) * 3} "
             f"parity clips): **{text}** (unrounded {floor:.4g}).\n\n"
             "SI-SDR of the float64 restatement, 6 s burst signal + white noise, n_fft 512 / hop 128:\n\n"
             "| mix | noisy | restatement | gain |\n|---|---|---|---|\n" + "\n".join(rows) + "\n")
    md = os.path.join(ROOT, "profiles", "bench_baseline.md")
    doc = open(md).read()
    doc, n = re.subn(r"(<!-- host:begin -->\n).*?(<!-- host:end -->)", lambda m: m.group(1) + block + m.group(2), doc, flags=re.S)
    assert n == 1
    open(md, "w").write(doc)
    print(f"FLOOR = {text}")
    print(block)


if __name__ == "__main__":
    main()
