"""The cases of the beamformer tests (tests/test_beamform_host.py, tests/test_gpu_beamform.py) -- TEST INFRASTRUCTURE.  Everything
is seeded.  The recordings are those of tests/dereverb_mc_cases.py (one dry signal heard by C microphones in different rooms) plus
independent white noise per microphone, which is what a spatial filter can remove and a per-channel gain cannot.

    python tests/beamform_cases.py          measures the float32 host floor over exactly the GPU parity cases and the SI-SDR table
                                            of the restatement, writes FLOOR and FLOOR_FULL_RANK into tests/beamform_ref.py
                                            and all of it into the marked host block of profiles/bench_beamform.md
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_ref  # noqa: E402
import beamform_ref as bf  # noqa: E402
import denoise_ref  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNR_DB = 8.0

# GPU parity cases.  F = 33 (n_fft 64) is a multiple of no tile width (16, 8 bins); T sits around the kernel's staging chunk of 32
# frames (1, 2, 23: less than one; 65, 97: a multiple plus one); C covers both lane groupings (4 lanes per bin up to
# C = 4, 8 beyond) and 1, 1, 2, 2 and 5 triangle entries per lane; both ends of the reference channel; 1 group and 3 groups.
PARITY_N_FFT = 64
PARITY_FRAMES = (1, 2, 23, 65, 97)
PARITY_CHANNELS = (1, 2, 3, 5, 8)
PARITY_GROUPS = (1, 3)
# ... n_fft 512 (F = 257) once, the weakest loading once, a mag_width wider than T once, a mask that is not the gain's once
WIDE_CASE = (512, 97, 4, dict())
LOADING_CASE = (64, 97, 4, dict(loading=1e-6))
PITCH_CASE = (64, 23, 3, dict(mag_extra=9))
UNIFORM_CASE = (64, 65, 5, dict(uniform_mask=True))
# The instantiations the grid above does not reach (tests/variant_cover.py): C = 4 is the edge of the 4-lane layout (C == LPB, all 64
# lanes stage a cell, 10 entries over 4 lanes), 6 and 7 are 21 and 28 entries over 8 lanes (3 and 4 per lane, a partial last
# round).  Over PARITY_FRAMES at both ends of the reference channel, and C = 6 once at an interior column of G.  Judged per bin
# only (tests/solver_bounds.py): the FLOOR constants are measured over parity_cases() and do not see these.
VARIANT_CHANNELS = (4, 6, 7)
VARIANT_REF_CASE = (64, 65, 6, (3,))


def parity_cases():
    """(n_fft, n_frames, C, extra) of every parity case; every case runs at ref_channel 0 and C - 1."""
    for n_frames in PARITY_FRAMES:
        for channels in PARITY_CHANNELS:
            yield PARITY_N_FFT, n_frames, channels, dict()
    yield WIDE_CASE
    yield LOADING_CASE
    yield PITCH_CASE
    yield UNIFORM_CASE


def refs_of(channels):
    return (0,) if channels == 1 else (0, channels - 1)


def variant_cases():
    """(n_fft, n_frames, C, reference channels) of every variant case."""
    for n_frames in PARITY_FRAMES:
        for channels in VARIANT_CHANNELS:
            yield PARITY_N_FFT, n_frames, channels, refs_of(channels)
    yield VARIANT_REF_CASE


def params_of(extra, ref):
    p = dict(ref_channel=ref)
    if "loading" in extra:
        p["loading"] = extra["loading"]
    return p


def add_noise(wet, seed, snr_db=SNR_DB):
    """wet (rows, L) float32 -> float32: independent white noise per row, drawn row after row from one generator, each draw scaled
    to `snr_db` below that row's power."""
    rng = np.random.default_rng(seed)
    out = np.empty_like(wet)
    for i, row in enumerate(wet):
        noise = rng.standard_normal(row.shape[0])
        power = float(np.mean(row.astype(np.float64) ** 2))
        noise *= np.sqrt(power / np.mean(noise ** 2)) * 10.0 ** (-snr_db / 20.0)
        out[i] = (row.astype(np.float64) + noise).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def parity_audio(n_fft, n_frames, channels):
    """(3 * channels, L) float32, the channels of a group consecutive: dereverb_mc_cases.parity_audio plus seeded noise."""
    out = add_noise(mc.parity_audio(n_fft, n_frames, channels), 1000 * n_fft + 10 * n_frames + channels)
    out.setflags(write=False)
    return out


def uniform_magnitudes(specs, seed):
    """M = seeded uniform [0, 1) x |X|, (C, F, T) float32: a mask that is not the gain's."""
    rng = np.random.default_rng(seed)
    a = np.abs(np.asarray(specs)).transpose(0, 2, 1)
    return (rng.random(a.shape) * a).astype(np.float32)


def magnitudes_of(specs, extra, seed=5):
    """The float32 mask magnitudes (C, F, T) a parity case runs on, from (C, T, F) spectrograms: the spectral gain's, or the
    seeded uniform ones."""
    if extra.get("uniform_mask"):
        return uniform_magnitudes(specs, seed)
    return bf.gain_magnitudes(specs).astype(np.float32)


@functools.lru_cache(maxsize=None)
def recording(channels, seconds=4.0):
    """-> (noisy (channels, L) float32, dry (L,) float32): dereverb_mc_cases.recording with independent white noise at 8 dB per
    microphone, np.random.default_rng(3), drawn microphone after microphone."""
    wet, dry = mc.recording(channels, seconds)
    noisy = add_noise(wet, 3)
    noisy.setflags(write=False)
    return noisy, dry


def floor_of(specs, mags, params):
    """max|Y32 - Y64| / max|Y64| of one group's (C, T, F) spectrograms (complex64 values) and float32 magnitudes."""
    y64 = bf.mvdr(specs, mags, params, dtype=np.float64)
    y32 = bf.mvdr(specs, mags, params, dtype=np.float32)
    return float(np.abs(y32.astype(np.complex128) - y64).max() / np.abs(y64).max())


def group_specs(n_fft, n_frames, channels, g):
    x = parity_audio(n_fft, n_frames, channels)[g * channels:(g + 1) * channels]
    return np.stack([denoise_ref.stft(row, n_fft, n_fft // 4).astype(np.complex64) for row in x])


def ill_conditioned(n_frames, channels, extra):
    """A case whose Phi_n only the loading conditions: fewer frames than channels (the covariances have rank T < C), or the weakest
    loading."""
    return n_frames < channels or "loading" in extra


def floor_for(n_frames, channels, extra):
    """The floor a parity case is held to: FLOOR_FULL_RANK unless only the loading conditions it."""
    return bf.FLOOR if ill_conditioned(n_frames, channels, extra) else bf.FLOOR_FULL_RANK


def measure_floor(verbose=False):
    """-> (worst over all parity cases, worst over those with T >= C at the default loading)."""
    worst, worst_default = 0.0, 0.0
    for n_fft, n_frames, channels, extra in parity_cases():
        for g in range(3):
            specs = group_specs(n_fft, n_frames, channels, g)
            mags = magnitudes_of(specs, extra)
            for ref in refs_of(channels):
                f = floor_of(specs, mags, params_of(extra, ref))
                worst = max(worst, f)
                if not ill_conditioned(n_frames, channels, extra):
                    worst_default = max(worst_default, f)
                if verbose:
                    print(f"n_fft {n_fft} T {n_frames} C {channels} ref {ref} {extra or ''} group {g}: {f:.3g}", flush=True)
    return worst, worst_default


# The SI-SDR table: label -> (wpe, mvdr, gain); "input" and the forms on microphone 0 alone are today's
TABLE = (("microphone 0 as recorded", None), ("spectral gain on microphone 0", None), ("MVDR, mask from the spectral gain", (False, False)),
         ("MVDR, then the spectral gain", (False, True)), ("joint WPE, then gain on channel 0", None),
         ("joint WPE, then MVDR", (True, False)), ("joint WPE, then MVDR, then gain", (True, True)))
TABLE_CHANNELS = (2, 4, 8)


@functools.lru_cache(maxsize=None)
def restatement_si_sdr(label, channels):
    """SI-SDR in dB against the dry signal of one row of TABLE at `channels` microphones -- float64 restatements, n_fft 512 /
    hop 128, defaults, after the inverse STFT.  None where the form does not exist (joint WPE at 8 channels has 4 taps: left out
    as in the issue's table)."""
    noisy, dry = recording(channels)
    x = noisy.astype(np.float64)
    if "WPE" in label and channels > 4:
        return None
    if label == "microphone 0 as recorded":
        out = x[0]
    elif label == "spectral gain on microphone 0":
        out = baseline_ref.denoise(x[0], 512, 128)
    elif label == "joint WPE, then gain on channel 0":
        out = mr.dereverb_mc(x, gain=True)[0]
    else:
        wpe, gain = dict(TABLE)[label]
        out = bf.beamform(x, wpe=wpe, gain=gain)
    return float(bf.si_sdr(out, dry))


def table_text():
    cell = lambda v: "–" if v is None else f"{v:.2f}"  # noqa: E731
    rows = "".join(f"| {label} | " + " | ".join(cell(restatement_si_sdr(label, c)) for c in TABLE_CHANNELS) + " |\n" for label, _ in TABLE)
    return "| form | " + " | ".join(f"C = {c}" for c in TABLE_CHANNELS) + " |\n|---|" + "---|" * len(TABLE_CHANNELS) + "\n" + rows


def main():
    floor, floor_default = measure_floor(verbose=True)
    text, text_default = f"{floor:.1e}", f"{floor_default:.1e}"
    path = os.path.join(ROOT, "tests", "beamform_ref.py")
    src = open(path).read()
    for name, value in (("FLOOR", text), ("FLOOR_FULL_RANK", text_default)):
        src, n = re.subn(rf"^{name} = .*$", f"{name} = {value}", src, flags=re.M)
        assert n == 1
    open(path, "w").write(src)
    n_cmp = sum(3 * len(refs_of(c)) for _, _, c, _ in parity_cases())
    block = (f"Float32 host floor (worst max|Y32 - Y64| / max|Y64| per group over the {n_cmp} parity comparisons -- every case, three "
             f"groups, both reference channels; the n_fft 512, loading 1e-6, wide mag_width and uniform-mask cases included): "
             f"**{text}** (unrounded {floor:.4g}), set by the cases with fewer frames than channels, whose covariances have "
             f"rank T < C and are conditioned by the loading alone; over the cases with T >= C at the default loading: "
             f"**{text_default}** (unrounded {floor_default:.4g}).\n\n"
             "SI-SDR (dB) against the dry signal, float64 restatements on the host: `dereverb_mc_cases.recording(C)` (4 s of "
             f"`speech_like(32000, 7)` heard by C microphones) with independent white noise at {SNR_DB:g} dB per microphone "
             "(`np.random.default_rng(3)`, drawn microphone after microphone, each draw scaled to that microphone's wet power); "
             "n_fft 512 / hop 128, every parameter at its default (joint WPE at taps = 32 // C), after the inverse STFT:\n\n"
             + table_text())
    md = os.path.join(ROOT, "profiles", "bench_beamform.md")
    doc = open(md).read()
    doc, n = re.subn(r"(<!-- host:begin -->\n).*?(<!-- host:end -->)", lambda m: m.group(1) + block + m.group(2), doc, flags=re.S)
    assert n == 1
    open(md, "w").write(doc)
    print(f"FLOOR = {text}, FLOOR_FULL_RANK = {text_default}")
    print(block)


if __name__ == "__main__":
    main()
