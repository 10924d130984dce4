"""The cases of the multichannel dereverberation tests (tests/test_dereverb_mc_host.py, tests/test_gpu_dereverb_mc.py) -- TEST
INFRASTRUCTURE.  Everything is seeded.  A recording of C microphones is one dry signal of tests/baseline_cases.py through the
Freeverb restatement of tests/reverb_ref.py at C different `rate` arguments: the rate only scales Freeverb's delay lengths, so
every microphone hears the same source in a different room.

    python tests/dereverb_mc_cases.py       measures the float32 host floor over exactly the GPU parity cases and the SI-SDR
                                            table of the restatement, writes FLOOR and FLOOR_DEFAULT_LOADING into
                                            tests/dereverb_mc_ref.py and all of it into the marked host block of
                                            profiles/bench_dereverb_mc.md
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_cases as bc  # noqa: E402
import denoise_ref  # noqa: E402
import dereverb_mc_ref as mr  # noqa: E402
import dereverb_ref as dr  # noqa: E402
import reverb_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000
MIC_RATES = (8000, 8600, 7500, 9100, 8300, 7800, 8900, 7200)     # microphone m: reverb_ref(dry, MIC_RATES[m])

# GPU parity cases.  F = 33 (n_fft 64) is a multiple of no tile width (16, 8, 4 bins); T sits around D, D + K and the kernel's
# staging chunk of 64 frames; (C, K) covers the three lane groupings (N = 10: 16 lanes; 20, 21, 24: 32; 32: 64), K not divisible
# by 4 (5, 10, 7) and divisible (8, 16, 4), and N = 32 three ways; 1 group and 3 groups.
PARITY_N_FFT = 64
PARITY_FRAMES = (1, 3, 4, 23, 65, 97)
PARITY_CK = ((2, 5), (2, 10), (3, 7), (3, 8), (2, 16), (4, 8), (8, 4))
PARITY_GROUPS = (1, 3)
# ... n_fft 512 (F = 257) once, and the weakest loading once
WIDE_CASE = (512, 97, (2, 10), None)
LOADING_CASE = (64, 97, (2, 16), dict(loading=1e-6))
# The kernel layouts PARITY_CK does not reach (tests/variant_cover.py): one pair per key (lanes per bin, WINDOW, P block columns,
# partial last row block, partial last P block, lanes doubled), the defaults taps = 32 // C where a key holds one -- (3, 10),
# (5, 6), (7, 4) --, and beside them (6, 5), the remaining default, and (7, 1), the smallest N at the largest pitch of 28 cells.
# n_fft 64, judged per bin only (tests/solver_bounds.py): the FLOOR constants are measured over parity_cases() and do not see these.
VARIANT_CK = ((2, 6), (2, 8), (4, 5), (4, 2), (3, 2), (4, 4), (3, 4), (4, 7), (2, 14), (3, 10), (8, 3), (8, 1), (6, 2), (5, 6),
              (5, 2), (7, 4), (5, 4), (6, 5), (7, 1))
VARIANT_FRAMES = (23, 97)


def parity_cases():
    """(n_fft, n_frames, (C, K), extra parameters or None) of every parity case."""
    for n_frames in PARITY_FRAMES:
        for ck in PARITY_CK:
            yield PARITY_N_FFT, n_frames, ck, None
    yield WIDE_CASE
    yield LOADING_CASE


def variant_cases():
    """(n_fft, n_frames, (C, K), None) of every variant case."""
    for ck in VARIANT_CK:
        for n_frames in VARIANT_FRAMES:
            yield PARITY_N_FFT, n_frames, ck, None


def params_of(ck, extra=None):
    return dict(extra or {}, taps=ck[1])


@functools.lru_cache(maxsize=None)
def _mic(kind, a, b, c, rate):
    dry = bc.parity_audio(a, b, 3)[c] if kind == "parity" else bc.speech_like(a, b)
    out = reverb_ref.reverb_ref(np.asarray(dry, np.float64), rate).astype(np.float32)
    out.setflags(write=False)
    return out


def parity_audio(n_fft, n_frames, channels, n_groups=3):
    """(n_groups * channels, L) float32, the channels of a group consecutive: group g is baseline_cases.parity_audio's clip g heard
    by `channels` microphones."""
    return np.stack([_mic("parity", n_fft, n_frames, g, MIC_RATES[c]) for g in range(n_groups) for c in range(channels)])


def recording(channels, seconds=4.0, seed=7):
    """-> (wet (channels, L) float32, dry (L,) float32): the burst signal heard by `channels` microphones."""
    n = int(seconds * SR)
    wet = np.stack([_mic("speech", n, seed, 0, MIC_RATES[c]) for c in range(channels)])
    return wet, bc.speech_like(n, seed).astype(np.float32)


def floor_of(specs, params):
    """max|d32 - d64| / max|d64| of one group's (C, T, F) spectrograms (complex64 values)."""
    d64 = mr.wpe_mc(specs, params, dtype=np.float64)
    d32 = mr.wpe_mc(specs, params, dtype=np.float32)
    return float(np.abs(d32.astype(np.complex128) - d64).max() / np.abs(d64).max())


def group_specs(n_fft, n_frames, channels, g):
    x = parity_audio(n_fft, n_frames, channels)[g * channels:(g + 1) * channels]
    return np.stack([denoise_ref.stft(row, n_fft, n_fft // 4).astype(np.complex64) for row in x])


def floor_for(extra):
    """The floor a parity case is held to: FLOOR_DEFAULT_LOADING unless the case changes the loading."""
    return mr.FLOOR if extra and "loading" in extra else mr.FLOOR_DEFAULT_LOADING


def measure_floor(verbose=False):
    """-> (worst over all parity cases, worst over those at the default loading)."""
    worst, worst_default = 0.0, 0.0
    for n_fft, n_frames, ck, extra in parity_cases():
        for g in range(3):
            f = floor_of(group_specs(n_fft, n_frames, ck[0], g), params_of(ck, extra))
            worst = max(worst, f)
            if not (extra and "loading" in extra):
                worst_default = max(worst_default, f)
            if verbose:
                print(f"n_fft {n_fft} T {n_frames} (C, K) {ck} {extra or ''} group {g}: {f:.3g}", flush=True)
    return worst, worst_default


# The SI-SDR table: (label, C, K); C = None is today's path, adn_wpe on every channel alone
TABLE = (("per channel, K = 20", None, 20), ("joint, C = 2, K = 10", 2, 10), ("joint, C = 2, K = 16", 2, 16),
         ("joint, C = 4, K = 8", 4, 8))


@functools.lru_cache(maxsize=None)
def restatement_si_sdr(label):
    """SI-SDR against the dry signal, per channel, of one row of TABLE ("input": the reverberant microphones 0 and 1) -- float64
    restatements, n_fft 512 / hop 128, D 3, I 3, after the inverse STFT."""
    if label == "input":
        wet, dry = recording(2)
        return tuple(float(mr.si_sdr(w, dry)) for w in wet)
    _, channels, taps = next(row for row in TABLE if row[0] == label)
    wet, dry = recording(channels or 2)
    x = wet.astype(np.float64)
    if channels is None:
        out = [dr.dereverb(row, params=dict(taps=taps)) for row in x]
    else:
        out = mr.dereverb_mc(x, params=dict(taps=taps))
    return tuple(float(mr.si_sdr(o, dry)) for o in out)


def main():
    floor, floor_default = measure_floor(verbose=True)
    text, text_default = f"{floor:.1e}", f"{floor_default:.1e}"
    path = os.path.join(ROOT, "tests", "dereverb_mc_ref.py")
    src = open(path).read()
    for name, value in (("FLOOR", text), ("FLOOR_DEFAULT_LOADING", text_default)):
        src, n = re.subn(rf"^{name} = .*$", f"{name} = {value}", src, flags=re.M)
        assert n == 1
    open(path, "w").write(src)
    n_groups = 3 * sum(1 for _ in parity_cases())
    fmt = lambda v: " / ".join(f"{s:.2f}" for s in v)  # noqa: E731
    block = (f"Float32 host floor (worst max|d32 - d64| / max|d64| per group over the {n_groups} parity groups, the n_fft 512 and the "
             f"loading 1e-6 cases included): **{text}** (unrounded {floor:.4g}), set by the loading 1e-6 case; over the cases at the "
             f"default loading alone: **{text_default}** (unrounded {floor_default:.4g}).\n\n"
             "SI-SDR against the dry signal per channel, float64 restatements on the host: `speech_like(32000, 7)` heard by "
             f"microphones `reverb_ref(dry, rate)` at rate {', '.join(str(r) for r in MIC_RATES[:4])}; n_fft 512 / hop 128, D 3, I 3, "
             "the default loading and floor, after the inverse STFT:\n\n"
             "| form | stacked size C K | SI-SDR per channel (dB) |\n|---|---|---|\n"
             f"| input | - | {fmt(restatement_si_sdr('input'))} |\n"
             + "".join(f"| {label} | {(c or 1) * k} | {fmt(restatement_si_sdr(label))} |\n" for label, c, k in TABLE))
    md = os.path.join(ROOT, "profiles", "bench_dereverb_mc.md")
    doc = open(md).read()
    doc, n = re.subn(r"(<!-- host:begin -->\n).*?(<!-- host:end -->)", lambda m: m.group(1) + block + m.group(2), doc, flags=re.S)
    assert n == 1
    open(md, "w").write(doc)
    print(f"FLOOR = {text}, FLOOR_DEFAULT_LOADING = {text_default}")
    print(block)


if __name__ == "__main__":
    main()
