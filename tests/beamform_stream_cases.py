"""The cases of the streaming beamformer tests (tests/test_beamform_stream_host.py, tests/test_gpu_beamform_stream.py) -- TEST
INFRASTRUCTURE.  The inputs are those of tests/beamform_cases.py (`parity_audio`, `magnitudes_of`), imported and not edited.

A case is (n_frames, channels, params, extra) at n_fft 64 (F = 33: both tile widths, 16 and 8 bins, end in a partial tile) and runs
on 1 and on 3 groups.  The float32 floor of a case is measured when a test runs, from the restatements alone
(tests/beamform_stream_ref.py), on the very inputs the compared result was computed from: the largest per-bin E
(tests/solver_bounds.py, `per_bin`) of the float32 restatement against the float64 one over every bin of the three groups, never
below 2^-23.  The recursion has one order of summation (frame after frame), so the two floor columns of `solver_bounds.check`'s line
hold the same figure.

    python tests/beamform_stream_cases.py          prints the floor of every parity case on the host's own inputs and the SI-SDR
                                                   table of the restatement (both are copied into profiles/bench_beamform_stream.md)
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_stream_ref as bs  # noqa: E402
import solver_bounds as sb  # noqa: E402

N_FFT = 64
N_BINS = N_FFT // 2 + 1
PARITY_FRAMES = (1, 2, 23, 65)
PARITY_CHANNELS = (1, 2, 3, 5, 8)
PARITY_GROUPS = (1, 3)
# added to the grid: a reference channel other than 0, both ends of forget, refresh 4, the weakest loading, a magnitude buffer wider
# than T read from a column > 0
ADDED = ((23, 3, dict(ref_channel=2), dict()),
         (65, 8, dict(ref_channel=7), dict()),
         (65, 5, dict(forget=0.9), dict()),
         (65, 2, dict(forget=1.0), dict()),
         (23, 8, dict(forget=1.0), dict()),
         (65, 3, dict(refresh=4), dict()),
         (23, 5, dict(refresh=4, forget=0.9, ref_channel=4), dict()),
         (65, 5, dict(loading=1e-6), dict()),
         (23, 3, dict(), dict(mag_extra=9, mag_col0=4)))
# The instantiations the grid above does not reach (tests/variant_cover.py): mvdr_stream_kernel<4>, <6> and <7>, over PARITY_FRAMES,
# C = 4 once at refresh 4 and forget 0.9, C = 7 once at its last reference channel.  A floor above VARIANT_CAP bounds nothing: such
# a case may not be here (tests/test_variant_cover_host.py).
VARIANT_CHANNELS = (4, 6, 7)
VARIANT_ADDED = ((65, 4, dict(refresh=4, forget=0.9), dict()),
                 (23, 7, dict(ref_channel=6), dict()))
VARIANT_CAP = 5e-4


def parity_cases():
    for n_frames in PARITY_FRAMES:
        for channels in PARITY_CHANNELS:
            yield n_frames, channels, dict(), dict()
    yield from ADDED


def variant_cases():
    for n_frames in PARITY_FRAMES:
        for channels in VARIANT_CHANNELS:
            yield n_frames, channels, dict(), dict()
    yield from VARIANT_ADDED


def label(n_frames, channels, params, extra, kind="parity"):
    return f"mvdr_stream {kind} n_fft {N_FFT} T {n_frames} C {channels} {dict(params, **extra) or 'defaults'}"


class Bounds:
    """ref: the float64 restatement (groups, T, F); f32: the float32 one; floor: the case's floor.  `floors` is shaped for
    solver_bounds.check, whose line names two orders: the recursion has one."""

    def __init__(self, ref, f32):
        self.ref, self.f32 = ref, f32
        f = float(sb.per_bin(f32, ref).max())
        self.floors = dict(pairwise=f, sequential=f)
        self.floor = max(f, sb.EPS)


@functools.lru_cache(maxsize=None)
def _bounds(spec, mags, channels, params):
    kw = dict(params)
    sg = spec.a.reshape((-1, channels) + spec.a.shape[1:])
    mg = mags.a.reshape((-1, channels) + mags.a.shape[1:])
    run = lambda dtype: np.stack([bs.mvdr_stream(s, m, kw, dtype=dtype)[0] for s, m in zip(sg, mg)])  # noqa: E731
    return Bounds(run(np.float64), run(np.float32))


def bounds(spec, mags, channels, params=None):
    """spec (groups * C, T, F) complex64, mags (groups * C, F, T) float32 -> Bounds of adn_mvdr_online on them from frame 0."""
    return _bounds(sb.Frozen(np.asarray(spec, np.complex64)), sb.Frozen(np.asarray(mags, np.float32)), channels,
                   tuple(sorted((params or {}).items())))


@functools.lru_cache(maxsize=None)
def host_inputs(n_frames, channels):
    """-> spec (3 * C, T, F) complex64, mags (3 * C, F, T) float32 (read-only): the host's own STFT and gain of the parity audio."""
    return sb.mvdr_inputs(N_FFT, n_frames, channels)


QUALITY_CHANNELS = (2, 4, 8)
QUALITY_SKIP = 8000                                  # "after the first second", at 8 kHz


@functools.lru_cache(maxsize=None)
def quality(channels):
    """SI-SDR (dB) against the dry signal of `beamform_cases.recording(channels)`, float64 restatements, n_fft 512 / hop 128, every
    parameter at its default, the mask the restated streaming one (the causal spectral gain of tests/baseline_ref.py per channel),
    after the inverse STFT: {"mic0" | "offline" | "stream": (whole, after the first second)}."""
    import denoise_ref
    noisy, dry = bc.recording(channels)
    x = noisy.astype(np.float64)
    specs = np.stack([denoise_ref.stft(row, 512, 128) for row in x])
    mags = bs.stream_mask_magnitudes(specs)
    outs = dict(mic0=x[0], offline=denoise_ref.istft(bc.bf.mvdr(specs, mags), 128, x.shape[1]),
                stream=denoise_ref.istft(bs.mvdr_stream(specs, mags)[0], 128, x.shape[1]))
    k = QUALITY_SKIP
    return {name: (float(bs.si_sdr(o, dry)), float(bs.si_sdr(o[k:], dry[k:]))) for name, o in outs.items()}


def quality_table():
    rows = ["| C | microphone 0, whole | after 1 s | offline MVDR, whole | after 1 s | streaming MVDR, whole | after 1 s |",
            "|---|---|---|---|---|---|---|"]
    for c in QUALITY_CHANNELS:
        q = quality(c)
        rows.append(f"| {c} | " + " | ".join(f"{v:.2f}" for name in ("mic0", "offline", "stream") for v in q[name]) + " |")
    return "\n".join(rows)


def main():
    print(quality_table(), flush=True)
    for case in parity_cases():
        n_frames, channels, params, extra = case
        b = bounds(*host_inputs(n_frames, channels), channels, params)
        print(f"{label(*case)}: float32 floor {b.floors['sequential']:.3g}", flush=True)
    for case in variant_cases():
        n_frames, channels, params, extra = case
        b = bounds(*host_inputs(n_frames, channels), channels, params)
        print(f"{label(*case, kind='variant')}: float32 floor {b.floors['sequential']:.3g}", flush=True)


if __name__ == "__main__":
    main()
