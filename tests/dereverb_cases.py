"""The cases of the dereverberation tests (tests/test_dereverb_host.py, tests/test_gpu_dereverb.py) -- TEST INFRASTRUCTURE.
Everything is seeded; the signals are tests/baseline_cases.py's, the reverberation tests/reverb_ref.py's Freeverb at 8 kHz.

    python tests/dereverb_cases.py          measures the float32 host floor over the GPU parity cases and the SI-SDR figures of the
                                            restatement, writes FLOOR into tests/dereverb_ref.py and both into the marked block of
                                            profiles/bench_dereverb.md
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_cases as bc  # noqa: E402
import baseline_ref as br  # noqa: E402
import denoise_ref  # noqa: E402
import dereverb_ref as dr  # noqa: E402
import reverb_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000

# GPU parity cases: F = 33 (less than a wave) and 257 (four waves + 1 lane); hop = n_fft / 4; the frame counts sit around D, D + 1,
# D + K and the kernel's staging chunk of 64 frames; 1 clip and 3 clips
PARITY_N_FFT = (64, 512)
PARITY_FRAMES = (1, 3, 4, 5, 22, 23, 24, 64, 65, 188)
PARITY_CLIPS = (1, 3)
CHUNK = 64                                  # frames per staged chunk of csrc/dereverb_kernels.hip (WPE_TC)
# ... and three more parameter sets at T = 97: the smallest, the largest, and the weakest loading
EXTRA_FRAMES = 97
EXTRA_PARAMS = (dict(taps=1, delay=1, iterations=1), dict(taps=32, delay=8, iterations=2), dict(loading=1e-6))
# The kernel layouts the cases above do not reach (tests/variant_cover.py): K = 19 is 16 lanes per bin with a partial fifth block
# row, 21 the first K of 32 lanes (partial), 28 the last (all 28 blocks), 29 the first of 64 lanes (partial).  n_fft 64, judged per
# bin only (tests/solver_bounds.py): FLOOR above is measured over parity_cases() and does not see these.
VARIANT_TAPS = (19, 21, 28, 29)
VARIANT_FRAMES = (23, 97)


@functools.lru_cache(maxsize=None)
def parity_audio(n_fft, n_frames, n_clips):
    """(n_clips, L) float32: baseline_cases.parity_audio through the Freeverb restatement at 8 kHz (read-only: cached)."""
    x = bc.parity_audio(n_fft, n_frames, n_clips)
    out = reverb_ref.reverb_ref(x.astype(np.float64), SR).astype(np.float32)
    out.setflags(write=False)
    return out


def parity_cases():
    """(n_fft, n_frames, params or None) of every parity case."""
    for n_fft in PARITY_N_FFT:
        for n_frames in PARITY_FRAMES:
            yield n_fft, n_frames, None
        for params in EXTRA_PARAMS:
            yield n_fft, EXTRA_FRAMES, params


def variant_cases():
    """(n_fft, n_frames, params) of every variant case."""
    for taps in VARIANT_TAPS:
        for n_frames in VARIANT_FRAMES:
            yield 64, n_frames, dict(taps=taps)


def floor_of(spec, params=None):
    """max|d32 - d64| / max|d64| of one clip's (T, F) spectrogram (complex64 values)."""
    d64 = dr.wpe(spec, params, dtype=np.float64)
    d32 = dr.wpe(spec, params, dtype=np.float32)
    return float(np.abs(d32.astype(np.complex128) - d64).max() / np.abs(d64).max())


def measure_floor(verbose=False):
    worst = 0.0
    for n_fft, n_frames, params in parity_cases():
        x = parity_audio(n_fft, n_frames, 3)
        for c in range(3):
            spec = denoise_ref.stft(x[c], n_fft, n_fft // 4).astype(np.complex64)
            f = floor_of(spec, params)
            worst = max(worst, f)
            if verbose:
                print(f"n_fft {n_fft} T {n_frames} {params or 'defaults'} clip {c}: {f:.3g}", flush=True)
    return worst


@functools.lru_cache(maxsize=None)
def reverberant(n_samples, seed):
    """-> (reverberant float32, dry float32): the burst signal through Freeverb at 8 kHz (read-only: cached)."""
    dry = bc.speech_like(n_samples, seed)
    wet = reverb_ref.reverb_ref(dry, SR).astype(np.float32)
    dry = dry.astype(np.float32)
    wet.setflags(write=False)
    dry.setflags(write=False)
    return wet, dry


def quality_case(seconds=4.0, seed=7):
    """The quality clip: 4 s of the burst signal, reverberant and dry."""
    return reverberant(int(seconds * SR), seed)


@functools.lru_cache(maxsize=None)
def restatement_si_sdr(seconds=4.0, seed=7):
    """SI-SDR against the dry signal of: the reverberant input, WPE, the spectral baseline alone, WPE then the spectral baseline --
    all from the float64 restatements, n_fft 512 / hop 128, the defaults."""
    wet, dry = quality_case(seconds, seed)
    x = wet.astype(np.float64)
    spec = denoise_ref.stft(x, 512, 128)
    return (dr.si_sdr(wet, dry), dr.si_sdr(dr.dereverb(x, spec=spec), dry), dr.si_sdr(br.denoise(x, spec=spec), dry),
            dr.si_sdr(dr.dereverb(x, gain=True, spec=spec), dry))


def main():
    floor = measure_floor(verbose=True)
    text = f"{floor:.1e}"
    path = os.path.join(ROOT, "tests", "dereverb_ref.py")
    src = open(path).read()
    src, n = re.subn(r"^FLOOR = .*$", f"FLOOR = {text}", src, flags=re.M)
    assert n == 1
    open(path, "w").write(src)
    a, b, c, d = restatement_si_sdr()
    n_clips = 3 * sum(1 for _ in parity_cases())
    block = (f"Float32 host floor (worst max|d32 - d64| / max|d64| per clip over the {n_clips} parity clips, the maximum-parameter "
             f"and the loading 1e-6 cases included): **{text}** (unrounded {floor:.4g}).\n\n"
             "SI-SDR against the dry signal, float64 restatements on the host, `speech_like(32000, 7)` through the Freeverb "
             "restatement at 8 kHz, n_fft 512 / hop 128, K 20, D 3, I 3:\n\n"
             "| path | SI-SDR |\n|---|---|\n"
             f"| reverberant input | {a:.2f} dB |\n| WPE | {b:.2f} dB |\n| spectral baseline alone | {c:.2f} dB |\n"
             f"| WPE, then spectral baseline | {d:.2f} dB |\n")
    md = os.path.join(ROOT, "profiles", "bench_dereverb.md")
    doc = open(md).read()
    doc, n = re.subn(r"(<!-- host:begin -->\n).*?(<!-- host:end -->)", lambda m: m.group(1) + block + m.group(2), doc, flags=re.S)
    assert n == 1
    open(md, "w").write(doc)
    print(f"FLOOR = {text}")
    print(block)


if __name__ == "__main__":
    main()
