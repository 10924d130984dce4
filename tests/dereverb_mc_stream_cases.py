"""The cases of the streaming multichannel dereverberation tests (tests/test_dereverb_mc_stream_host.py,
tests/test_gpu_dereverb_mc_stream.py) -- TEST INFRASTRUCTURE.  Everything is seeded; the recordings are tests/dereverb_mc_cases.py's
(one dry signal heard by C microphones through the Freeverb restatement).

    python tests/dereverb_mc_stream_cases.py   measures, on the host from the restatement, the float32 floors over the GPU parity
                                               cases, the long-run figures and the SI-SDR table, writes FLOOR and FLOOR_AUDIO into
                                               tests/dereverb_mc_stream_ref.py and all of it into the marked host block of
                                               profiles/bench_dereverb_mc_stream.md
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_cases as bc  # noqa: E402
import denoise_ref  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_stream_ref as ms  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402
import reverb_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = mc.SR

# GPU parity cases.  F = 33 (n_fft 64) is a multiple of no 8-bin tile: four whole workgroups and one bin.  T sits at 1, at D, at
# D + 1, around a wrap of the longest ring (D + K = 19 frames at K = 16) and at several steps; (C, K) gives N = 10, 21 and 32 three
# ways (the C lanes that form errors: 2, 3, 4, 8; lanes idle: 22, 11, 0); 1 group and 3 groups.
PARITY_N_FFT = 64
PARITY_FRAMES = (1, 3, 4, 23, 97)
PARITY_CK = ((2, 5), (3, 7), (2, 16), (4, 8), (8, 4))
PARITY_GROUPS = (1, 3)
# ... n_fft 512 (F = 257) once, the lowest legal forget at N = 32 once, the longest delay once (at (8, 4): the longest rings, 96 cells)
WIDE_CASE = (512, 97, (2, 10), None)
FORGET_CASE = (64, 97, (2, 16), dict(forget=ms.lowest_forget(32)))
DELAY_CASE = (64, 97, (8, 4), dict(delay=8))
# The channel counts PARITY_CK does not reach (tests/variant_cover.py): C is a run-time value of the kernel, and at 5, 6 and 7 the
# defaults taps = 32 // C give N = 30, 30, 28 (rows of P idle), record sizes that are multiples of nothing and rings at c H with
# odd H; (5, 2) and (7, 1) are short rings.  At T = 4 only frame 3 is filtered.  Judged per bin only (tests/recursive_bounds.py):
# FLOOR below is measured over parity_cases() and does not see these.
VARIANT_CK = ((5, 6), (6, 5), (7, 4), (5, 2), (7, 1))
VARIANT_FRAMES = (4, 23, 97)
# end to end: C = 2 at the defaults (taps 16), three recordings, with and without the gain
E2E_FRAMES = 97
E2E_CHANNELS = 2
E2E_N_FFT = (64, 512)

# long runs of the float32 restatement (3750 frames: 60 s at 8 kHz) at N = 32
LONG_FRAMES = 3750
LONG_RUNS = (((2, 16), 0.99), ((8, 4), 0.99), ((2, 16), ms.lowest_forget(32)), ((8, 4), ms.lowest_forget(32)))
LONG_BINS = tuple(range(2, 257, 51))                 # 5 of the 257 bins: the run is a Python loop over frames


def parity_cases():
    """(n_fft, n_frames, (C, K), extra parameters or None) of every parity case."""
    for n_frames in PARITY_FRAMES:
        for ck in PARITY_CK:
            yield PARITY_N_FFT, n_frames, ck, None
    yield WIDE_CASE
    yield FORGET_CASE
    yield DELAY_CASE


def variant_cases():
    """(n_fft, n_frames, (C, K), None) of every variant case."""
    for ck in VARIANT_CK:
        for n_frames in VARIANT_FRAMES:
            yield PARITY_N_FFT, n_frames, ck, None


def case_id(case):
    n_fft, n_frames, ck, extra = case
    return f"{n_fft}-T{n_frames}-C{ck[0]}K{ck[1]}" + ("".join(f"-{k}{v:g}" for k, v in extra.items()) if extra else "")


def params_of(ck, extra=None):
    return dict(extra or {}, taps=ck[1])


parity_audio = mc.parity_audio                         # (n_fft, n_frames, channels, n_groups=3) -> (n_groups * channels, L)


def floor_of(specs, params):
    """max|d32 - d64| / max|d64| of one group's (C, T, F) spectrograms (complex64 values)."""
    d64 = ms.wpe_mc_online(specs, params, dtype=np.float64)
    d32 = ms.wpe_mc_online(specs, params, dtype=np.float32)
    return float(np.abs(d32.astype(np.complex128) - d64).max() / np.abs(d64).max())


def measure_floor(verbose=False):
    worst = 0.0
    for n_fft, n_frames, ck, extra in parity_cases():
        for g in range(3):
            f = floor_of(mc.group_specs(n_fft, n_frames, ck[0], g), params_of(ck, extra))
            worst = max(worst, f)
            if verbose:
                print(f"n_fft {n_fft} T {n_frames} (C, K) {ck} {extra or ''} group {g}: {f:.3g}", flush=True)
    return worst


def e2e_cases():
    """(n_fft, gain) of every end-to-end case; the audio is parity_audio(n_fft, E2E_FRAMES, E2E_CHANNELS)."""
    for n_fft in E2E_N_FFT:
        for gain in (False, True):
            yield n_fft, gain


@functools.lru_cache(maxsize=None)
def e2e_want(n_fft, gain, g):
    """The float64 end-to-end form of recording g, (C, L) (read-only: cached)."""
    x = parity_audio(n_fft, E2E_FRAMES, E2E_CHANNELS)[g * E2E_CHANNELS:(g + 1) * E2E_CHANNELS]
    out = ms.stream_dereverb_mc(x.astype(np.float64), n_fft, n_fft // 4, gain=gain)
    out.setflags(write=False)
    return out


def measure_floor_audio(verbose=False):
    """The worst max|a32 - a64| / max|a64| per channel over the end-to-end cases."""
    worst = 0.0
    for n_fft, gain in e2e_cases():
        for g in range(3):
            x = parity_audio(n_fft, E2E_FRAMES, E2E_CHANNELS)[g * E2E_CHANNELS:(g + 1) * E2E_CHANNELS]
            a64 = e2e_want(n_fft, gain, g)
            a32 = ms.stream_dereverb_mc(x, n_fft, n_fft // 4, gain=gain, dtype=np.float32)
            for c in range(E2E_CHANNELS):
                f = float(np.abs(a32[c].astype(np.float64) - a64[c]).max() / np.abs(a64[c]).max())
                worst = max(worst, f)
                if verbose:
                    print(f"end to end n_fft {n_fft} gain {gain} recording {g} channel {c}: {f:.3g}", flush=True)
    return worst


@functools.lru_cache(maxsize=None)
def _long_channel(c):
    """(LONG_FRAMES, len(LONG_BINS)) complex64: 60 s of the burst signal at microphone c, n_fft 512 / hop 128, a comb of bins."""
    n = (LONG_FRAMES - 1) * 128 + 64
    wet = reverb_ref.reverb_ref(bc.speech_like(n, 11).astype(np.float64), mc.MIC_RATES[c])
    spec = denoise_ref.stft(wet, 512, 128)[:, list(LONG_BINS)].astype(np.complex64)
    assert spec.shape[0] == LONG_FRAMES
    spec.setflags(write=False)
    return spec


def long_specs(channels):
    return np.stack([_long_channel(c) for c in range(channels)])


@functools.lru_cache(maxsize=None)
def long_run(index, with_float64=False):
    """-> (finite, the four per-quarter figures max|d32 - d64| / max|d64| or None) of LONG_RUNS[index] in float32."""
    (channels, taps), forget = LONG_RUNS[index]
    specs = long_specs(channels)
    params = dict(taps=taps, forget=forget)
    d32 = ms.wpe_mc_online(specs, params, dtype=np.float32)
    finite = bool(np.isfinite(d32).all())
    if not with_float64:
        return finite, None
    d64 = ms.wpe_mc_online(specs, params, dtype=np.float64)
    scale = np.abs(d64).max()
    q = LONG_FRAMES // 4
    err = np.abs(d32.astype(np.complex128) - d64)
    return finite, tuple(float(err[:, i * q:(i + 1) * q if i < 3 else None].max() / scale) for i in range(4))


# The SI-SDR table: (label, C, K, gain); C = None is the single-channel stream form on microphone 0
TABLE = (("single-channel stream, K = 20", None, 20, False), ("joint stream, C = 2, K = 10", 2, 10, False),
         ("joint stream, C = 2, K = 16", 2, 16, False), ("joint stream, C = 4, K = 8", 4, 8, False),
         ("joint stream, C = 2, K = 16, then the spectral gain", 2, 16, True))


@functools.lru_cache(maxsize=None)
def restatement_si_sdr(label):
    """SI-SDR against the dry signal, per channel, of one row of TABLE ("input": the reverberant microphones 0 and 1) -- float64
    restatements on dereverb_mc_cases.recording, n_fft 512 / hop 128, D 3, forget 0.99, loading 300."""
    if label == "input":
        wet, dry = mc.recording(2)
        return tuple(float(ms.si_sdr(w, dry)) for w in wet)
    _, channels, taps, gain = next(row for row in TABLE if row[0] == label)
    wet, dry = mc.recording(channels or 1)
    x = wet.astype(np.float64)
    if channels is None:
        out = [ds.stream_dereverb(x[0], params=dict(taps=taps), gain=gain)]
    else:
        out = ms.stream_dereverb_mc(x, params=dict(taps=taps), gain=gain)
    return tuple(float(ms.si_sdr(o, dry)) for o in out)


def main():
    floor, floor_audio = measure_floor(verbose=True), measure_floor_audio(verbose=True)
    text, text_audio = f"{floor:.1e}", f"{floor_audio:.1e}"
    path = os.path.join(ROOT, "tests", "dereverb_mc_stream_ref.py")
    src = open(path).read()
    src, n = re.subn(r"^FLOOR = .*$", f"FLOOR = {text}", src, flags=re.M)
    src, m = re.subn(r"^FLOOR_AUDIO = .*$", f"FLOOR_AUDIO = {text_audio}", src, flags=re.M)
    assert n == 1 and m == 1
    open(path, "w").write(src)
    n_groups = 3 * sum(1 for _ in parity_cases())
    fmt = lambda v: " / ".join(f"{s:.2f}" for s in v)  # noqa: E731
    rows = ""
    for i, ((channels, taps), forget) in enumerate(LONG_RUNS):
        finite, q = long_run(i, True)
        rows += (f"| ({channels}, {taps}) | {forget:.6f} | {'yes' if finite else 'NO'} | " + " | ".join(f"{v:.2g}" for v in q) + " |\n")
    block = (f"Float32 host floor of the spectrum (worst max|d32 - d64| / max|d64| per group over the {n_groups} parity groups, the "
             f"n_fft 512, lowest-forget and delay-8 cases included): **{text}** (unrounded {floor:.4g}).\n\n"
             f"Float32 host floor of the audio (the end-to-end form with every statement in float32, the transforms included, per "
             f"channel over the {3 * E2E_CHANNELS * sum(1 for _ in e2e_cases())} end-to-end channels, with and without the gain): "
             f"**{text_audio}** (unrounded {floor_audio:.4g}).\n\n"
             f"Long runs of the float32 restatement at N = 32, {LONG_FRAMES} frames (60 s at 8 kHz) of `speech_like` heard by the "
             f"microphones of `dereverb_mc_cases.MIC_RATES`, {len(LONG_BINS)} bins of n_fft 512: max|d32 - d64| / max|d64| per "
             "quarter of the clip:\n\n"
             "| (C, K) | forget | finite | Q1 | Q2 | Q3 | Q4 |\n|---|---|---|---|---|---|---|\n" + rows + "\n"
             "SI-SDR against the dry signal per channel, float64 restatements on the host: `speech_like(32000, 7)` heard by "
             f"microphones `reverb_ref(dry, rate)` at rate {', '.join(str(r) for r in mc.MIC_RATES[:4])}; n_fft 512 / hop 128, D 3, "
             "forget 0.99, loading 300, after the inverse STFT:\n\n"
             "| form | stacked size C K | SI-SDR per channel (dB) |\n|---|---|---|\n"
             f"| input | - | {fmt(restatement_si_sdr('input'))} |\n"
             + "".join(f"| {label} | {(c or 1) * k} | {fmt(restatement_si_sdr(label))} |\n" for label, c, k, _ in TABLE))
    md = os.path.join(ROOT, "profiles", "bench_dereverb_mc_stream.md")
    doc = open(md).read()
    doc, n = re.subn(r"(<!-- host:begin -->\n).*?(<!-- host:end -->)", lambda m: m.group(1) + block + m.group(2), doc, flags=re.S)
    assert n == 1
    open(md, "w").write(doc)
    print(f"FLOOR = {text}\nFLOOR_AUDIO = {text_audio}")
    print(block)


if __name__ == "__main__":
    main()
