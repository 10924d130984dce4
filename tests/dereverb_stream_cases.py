"""The cases of the streaming dereverberation tests (tests/test_dereverb_stream_host.py, tests/test_gpu_dereverb_stream.py) -- TEST
INFRASTRUCTURE.  Everything is seeded; the signals are tests/dereverb_cases.py's (tests/baseline_cases.py's through the Freeverb
restatement at 8 kHz).

    python tests/dereverb_stream_cases.py   measures, on the host from the restatement, the float32 floors over the GPU parity cases,
                                            the long-run stability figures and the SI-SDR figures, writes FLOOR and FLOOR_AUDIO
                                            into tests/dereverb_stream_ref.py and all of it into the marked block of
                                            profiles/bench_dereverb_stream.md
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref  # noqa: E402
import dereverb_cases as dc  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = dc.SR

# GPU parity cases: F = 33 (less than a wave: four whole workgroups of 8 bins and one bin) and 257 (32 workgroups and one bin);
# hop = n_fft / 4; the frame counts sit around D, D + 1, D + K, a wrap of the history ring (D + K = 23 frames) and several steps
PARITY_N_FFT = (64, 512)
PARITY_FRAMES = (1, 3, 4, 5, 23, 24, 40, 97)
PARITY_ROWS = (1, 3)
PARITY_PARAMS = (None, dict(taps=1, delay=1), dict(taps=32, delay=8, forget=0.95))
PARAM_IDS = ("defaults", "smallest", "largest")
# end to end: the longest rows, a block that divides the frames (1), one that does not (4: 97 = 24 x 4 + 1), with and without gain
E2E_FRAMES = 97
E2E_BLOCKS = (1, 4)

# long runs of the float32 restatement (3750 frames: 60 s at 8 kHz) at the defaults and at the corners of the legal ranges
LONG_FRAMES = 3750
LONG_PARAMS = (None, dict(forget=0.95, taps=32, delay=1), dict(forget=1.0))
LONG_IDS = ("defaults", "forget 0.95, K 32, D 1", "forget 1.0")
LONG_BINS = tuple(range(2, 257, 17))                 # 15 of the 257 bins: the run is a Python loop over frames


def parity_audio(n_fft, n_frames, n_rows=3):
    return dc.parity_audio(n_fft, n_frames, 3)[:n_rows]


def parity_cases():
    """(n_fft, n_frames, params or None) of every parity case."""
    for n_fft in PARITY_N_FFT:
        for n_frames in PARITY_FRAMES:
            for params in PARITY_PARAMS:
                yield n_fft, n_frames, params


def floor_of(spec, params=None):
    """max|d32 - d64| / max|d64| of one row's (T, F) spectrogram (complex64 values)."""
    d64 = ds.wpe_online(spec, params, dtype=np.float64)
    d32 = ds.wpe_online(spec, params, dtype=np.float32)
    return float(np.abs(d32.astype(np.complex128) - d64).max() / np.abs(d64).max())


def measure_floor(verbose=False):
    worst = 0.0
    for n_fft, n_frames, params in parity_cases():
        x = parity_audio(n_fft, n_frames)
        for c in range(3):
            spec = denoise_ref.stft(x[c], n_fft, n_fft // 4).astype(np.complex64)
            f = floor_of(spec, params)
            worst = max(worst, f)
            if verbose:
                print(f"n_fft {n_fft} T {n_frames} {params or 'defaults'} row {c}: {f:.3g}", flush=True)
    return worst


def e2e_cases():
    """(n_fft, gain) of every end-to-end case; the audio is parity_audio(n_fft, E2E_FRAMES)."""
    for n_fft in PARITY_N_FFT:
        for gain in (False, True):
            yield n_fft, gain


@functools.lru_cache(maxsize=None)
def e2e_want(n_fft, gain, row):
    """The float64 end-to-end form of one row (read-only: cached)."""
    x = parity_audio(n_fft, E2E_FRAMES)[row]
    out = ds.stream_dereverb(x.astype(np.float64), n_fft, n_fft // 4, gain=gain)
    out.setflags(write=False)
    return out


def measure_floor_audio(verbose=False):
    worst = 0.0
    for n_fft, gain in e2e_cases():
        for c in range(3):
            x = parity_audio(n_fft, E2E_FRAMES)[c]
            a64 = e2e_want(n_fft, gain, c)
            a32 = ds.stream_dereverb(x, n_fft, n_fft // 4, gain=gain, dtype=np.float32)
            f = float(np.abs(a32.astype(np.float64) - a64).max() / np.abs(a64).max())
            worst = max(worst, f)
            if verbose:
                print(f"end to end n_fft {n_fft} gain {gain} row {c}: {f:.3g}", flush=True)
    return worst


@functools.lru_cache(maxsize=None)
def long_spec():
    """(LONG_FRAMES, len(LONG_BINS)) complex64: 60 s of the burst signal through Freeverb, n_fft 512 / hop 128, a comb of bins."""
    wet, _ = dc.reverberant((LONG_FRAMES - 1) * 128 + 64, 11)
    spec = denoise_ref.stft(wet.astype(np.float64), 512, 128)[:, list(LONG_BINS)].astype(np.complex64)
    assert spec.shape[0] == LONG_FRAMES
    spec.setflags(write=False)
    return spec


@functools.lru_cache(maxsize=None)
def long_run(index):
    """-> (finite, the four per-quarter figures max|d32 - d64| / max|d64| over the whole clip) of LONG_PARAMS[index]."""
    spec = long_spec()
    d64 = ds.wpe_online(spec, LONG_PARAMS[index], dtype=np.float64)
    d32 = ds.wpe_online(spec, LONG_PARAMS[index], dtype=np.float32)
    scale = np.abs(d64).max()
    q = LONG_FRAMES // 4
    err = np.abs(d32.astype(np.complex128) - d64)
    quarters = tuple(float(err[i * q:(i + 1) * q if i < 3 else None].max() / scale) for i in range(4))
    return bool(np.isfinite(d32).all() and np.isfinite(d64).all()), quarters


@functools.lru_cache(maxsize=None)
def restatement_si_sdr(seconds=4.0, seed=7):
    """SI-SDR against the dry signal of: the reverberant input, the stream form at the defaults, the stream form with the gain,
    offline WPE -- all from the float64 restatements, n_fft 512 / hop 128."""
    wet, dry = dc.quality_case(seconds, seed)
    x = wet.astype(np.float64)
    return (ds.si_sdr(wet, dry), ds.si_sdr(ds.stream_dereverb(x), dry), ds.si_sdr(ds.stream_dereverb(x, gain=True), dry),
            dc.restatement_si_sdr(seconds, seed)[1])


def main():
    floor, floor_audio = measure_floor(verbose=True), measure_floor_audio(verbose=True)
    text, text_audio = f"{floor:.1e}", f"{floor_audio:.1e}"
    path = os.path.join(ROOT, "tests", "dereverb_stream_ref.py")
    src = open(path).read()
    src, n = re.subn(r"^FLOOR = .*$", f"FLOOR = {text}", src, flags=re.M)
    src, m = re.subn(r"^FLOOR_AUDIO = .*$", f"FLOOR_AUDIO = {text_audio}", src, flags=re.M)
    assert n == 1 and m == 1
    open(path, "w").write(src)
    a, b, c, d = restatement_si_sdr()
    n_rows = 3 * sum(1 for _ in parity_cases())
    rows = ""
    for i, name in enumerate(LONG_IDS):
        finite, q = long_run(i)
        rows += f"| {name} | {'yes' if finite else 'NO'} | " + " | ".join(f"{v:.2g}" for v in q) + f" | {q[3] / q[1]:.2f} |\n"
    block = (f"Float32 host floor of the spectrum (worst max|d32 - d64| / max|d64| per row over the {n_rows} parity rows, the three "
             f"parameter sets included): **{text}** (unrounded {floor:.4g}).\n\n"
             f"Float32 host floor of the audio (the end-to-end stream form with every statement in float32, the transforms included, "
             f"over the {3 * sum(1 for _ in e2e_cases())} end-to-end rows, with and without the gain): **{text_audio}** (unrounded "
             f"{floor_audio:.4g}).\n\n"
             f"Long runs of the float32 restatement, {LONG_FRAMES} frames (60 s at 8 kHz) of `speech_like` through the Freeverb "
             f"restatement, {len(LONG_BINS)} bins of n_fft 512: max|d32 - d64| / max|d64| per quarter of the clip, and the growth "
             "from the second quarter to the fourth (the host test allows 4):\n\n"
             "| parameters | finite | Q1 | Q2 | Q3 | Q4 | Q4 / Q2 |\n|---|---|---|---|---|---|---|\n" + rows + "\n"
             "SI-SDR against the dry signal, float64 restatements on the host, `speech_like(32000, 7)` through the Freeverb "
             "restatement at 8 kHz, n_fft 512 / hop 128, the defaults:\n\n"
             "| path | SI-SDR |\n|---|---|\n"
             f"| reverberant input | {a:.2f} dB |\n| stream form (recursive WPE) | {b:.2f} dB |\n"
             f"| stream form, then the spectral gain | {c:.2f} dB |\n| offline WPE | {d:.2f} dB |\n")
    md = os.path.join(ROOT, "profiles", "bench_dereverb_stream.md")
    doc = open(md).read()
    doc, n = re.subn(r"(<!-- host:begin -->\n).*?(<!-- host:end -->)", lambda m: m.group(1) + block + m.group(2), doc, flags=re.S)
    assert n == 1
    open(md, "w").write(doc)
    print(f"FLOOR = {text}\nFLOOR_AUDIO = {text_audio}")
    print(block)


if __name__ == "__main__":
    main()
