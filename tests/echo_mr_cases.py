"""The cases of the multi-reference echo canceller tests (tests/test_echo_mr_host.py, tests/test_gpu_echo_mr.py) -- TEST
INFRASTRUCTURE.  tests/echo_cases.py's recipes, extended to Q loudspeakers.

Parity audio, per row and Q: L = n_fft + (T - 1) n_fft / 4 samples; src_q = speech_like(L, seed + 200 q) at peak 0.5, far_q = src_q +
0.3 sum_{a != q} src_a at peak 0.5 (the channels of a stereo programme are correlated; a row too short to hold a burst stays zero and
every frame is gated); near = speech_like(L, seed + 100) at peak 0.5 with near[: L // 3] = 0; Q rooms of 5 hop taps of standard_normal
* exp(-n / hop), each scaled to energy 0.49 / Q, drawn in channel order; mic = sum_q conv(far_q, room_q)[:L] + near + 1e-3
standard_normal.  The spectra are denoise_ref.stft's, rounded to complex64, the first T frames.  Three rows per case.

One parameter set per lane layout and edge (PARAMS): G = 8 full (8 x 1, 2 x 4) and partial (2 x 3), G = 16 partial (3 x 5) and full (2
x 8, the default of refs = 2, and 4 x 4, the default of refs = 4), G = 32 at its first size (2 x 9), partial (5 x 6) and full (2 x 16
with the largest ring, D = 8, and 8 x 4).  Every `forget` satisfies 2 N (1 - forget) <= 1; the two full G = 32 sets sit at the rule's
edge (0.984375) and at the default.

The grid's rows of 1, 4 and 5 frames at n_fft 64 are 64 ... 128 samples long: the far end's first burst has not begun and every frame
is gated.  The SHORT cases cut the same frame counts out of the 97-frame case where the far end is active (frames 80 ...) and run
them as frames 0 ... T - 1 of a fresh row, one parameter set per lane layout, all at delay 0.

    python tests/echo_mr_cases.py   prints the fp32 floor of every parity case on the host's own inputs and the quality table of
                                    the restatement (both are copied into profiles/bench_echo_mr.md)
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_bounds as sb  # noqa: E402  (first: it completes dereverb_cases -> baseline_cases)
import baseline_cases as bc  # noqa: E402
import denoise_ref  # noqa: E402
import echo_cases as ec  # noqa: E402
import echo_mr_ref as mr  # noqa: E402
import echo_ref as er  # noqa: E402
import recursive_bounds as rb  # noqa: E402

PARITY_N_FFT = (64, 512)
PARITY_FRAMES = {64: (1, 4, 5, 24, 40, 97), 512: (40,)}
PARITY_ROWS = (1, 3)
# (Q, params): taps per channel.  None: the header's default for that Q
PARAMS = ((8, dict(taps=1, forget=0.95)), (2, dict(taps=4)), (2, dict(taps=3, delay=1, forget=0.95)),
          (3, dict(taps=5, delay=2, forget=0.97)), (2, None), (4, None), (2, dict(taps=9, forget=0.98)),
          (5, dict(taps=6, delay=1, forget=0.99)), (2, dict(taps=16, delay=8, forget=0.984375)), (8, dict(taps=4)))
PARAM_IDS = ("8x1", "2x4", "2x3-D1", "3x5-D2", "2x8-default", "4x4-default", "2x9", "5x6-D1", "2x16-D8", "8x4")
WIDE_PARAMS = (PARAMS[4], PARAMS[8])                   # the sets that also run at n_fft 512 (F = 257)
WIDE_IDS = ("2x8-default", "2x16-D8")
LAYOUTS = (PARAMS[1], PARAMS[4], PARAMS[9])            # G = 8, 16, 32, all full, all at delay 0
LAYOUT_IDS = ("G8-2x4", "G16-2x8", "G32-8x4")
SHORT_FRAMES, SHORT_FROM = (1, 4, 5), 80
TILTED_FRAMES = 97
TILTED_PARAMS = (PARAMS[4],)
E2E_FRAMES = 97
LONG_FRAMES, LONG_SILENCE, LONG_BINS = ec.LONG_FRAMES, ec.LONG_SILENCE, ec.LONG_BINS


def taps_delay(refs, kw):
    p = dict(mr.defaults(refs), **(kw or {}))
    return p["taps"], p["delay"]


def record_floats(refs, kw):
    """2 N^2 + 4 N + 2 Q D: the floats of a (slot, bin) record."""
    k, d = taps_delay(refs, kw)
    n = refs * k
    return 2 * n * n + 4 * n + 2 * refs * d


def lanes(refs, kw):
    n = refs * taps_delay(refs, kw)[0]
    return 8 if n <= 8 else 16 if n <= 16 else 32


def cases():
    """(n_fft, n_frames, refs, params or None) of every parity case."""
    for n_frames in PARITY_FRAMES[64]:
        for refs, kw in PARAMS:
            yield 64, n_frames, refs, kw
    for n_frames in PARITY_FRAMES[512]:
        for refs, kw in WIDE_PARAMS:
            yield 512, n_frames, refs, kw


def label(n_fft, n_frames, refs, kw, kind="parity"):
    return f"aec_mr_online {kind} n_fft {n_fft} T {n_frames} refs {refs} {kw or 'defaults'}"


def far_mix(sources):
    """src (Q, L) -> far (Q, L): far_q = src_q + 0.3 sum_{a != q} src_a, each at peak 0.5."""
    total = sources.sum(axis=0)
    return np.stack([ec._peak(s + 0.3 * (total - s)) for s in sources])


@functools.lru_cache(maxsize=None)
def parity_audio(n_fft, n_frames, refs):
    """-> mic (3, L), far (3, Q, L), near (3, L) float64 (read-only)."""
    L, hop = ec.parity_length(n_fft, n_frames), n_fft // 4
    mics, fars, nears = [], [], []
    for c in range(3):
        seed = 1000 * n_fft + 10 * n_frames + c
        rng = np.random.default_rng(seed + 50000)
        far = far_mix(np.stack([ec._peak(bc.speech_like(L, seed + 200 * q)) for q in range(refs)]))
        near = ec._peak(bc.speech_like(L, seed + 100))
        near[: L // 3] = 0.0
        rooms = [ec._room(rng, 5 * hop, hop) / np.sqrt(refs) for _ in range(refs)]
        mics.append(sum(np.convolve(f, room)[:L] for f, room in zip(far, rooms)) + near + 1e-3 * rng.standard_normal(L))
        fars.append(far)
        nears.append(near)
    arrays = (np.stack(mics), np.stack(fars), np.stack(nears))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _spec(x, n_fft, n_frames):
    return denoise_ref.stft(x, n_fft, n_fft // 4)[:n_frames].astype(np.complex64)


@functools.lru_cache(maxsize=None)
def parity_spec(n_fft, n_frames, refs):
    """-> mic (3, T, F), far (3, Q, T, F) complex64 (read-only)."""
    mic, far, _ = parity_audio(n_fft, n_frames, refs)
    out = (np.stack([_spec(row, n_fft, n_frames) for row in mic]),
           np.stack([np.stack([_spec(ch, n_fft, n_frames) for ch in row]) for row in far]))
    for a in out:
        a.setflags(write=False)
    return out


def short_spec(n_frames, refs):
    """-> mic (3, n_frames, 33), far (3, Q, n_frames, 33) complex64 (read-only): the short cases whose far end is NOT silent."""
    mic, far = parity_spec(64, 97, refs)
    out = (np.ascontiguousarray(mic[:, SHORT_FROM:SHORT_FROM + n_frames]), np.ascontiguousarray(far[:, :, SHORT_FROM:SHORT_FROM + n_frames]))
    assert all((np.abs(out[1][c]) ** 2 > 1e-8).mean() > 0.5 for c in range(3))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _bounds(mic, far, params):
    kw = None if params is None else dict(params)
    n = mic.a.shape[0]
    wide_m, wide_f = np.concatenate(list(mic.a), axis=-1), np.concatenate(list(far.a), axis=-1)   # the rows as more bins of one call
    f32 = {a: np.stack(np.split(mr.aec_mr_online(wide_m, wide_f, kw, dtype=np.float32, arithmetic=a), n, axis=-1)) for a in rb.ARITHMETICS}
    ref = np.stack([mr.aec_mr_online(m.astype(np.complex128), f.astype(np.complex128), kw) for m, f in zip(mic.a, far.a)])
    return rb.Bounds(ref, f32)


def aec_mr_bounds(mic, far, params=None):
    """mic (rows, T, F), far (rows, Q, T, F) complex64 -> recursive_bounds.Bounds of adn_aec_mr_online on them from frame 0."""
    return _bounds(sb.Frozen(np.asarray(mic, np.complex64)), sb.Frozen(np.asarray(far, np.complex64)), rb._items(params))


def tilted(spec):
    return sb.scale_spec(spec, sb.tilt(spec.shape[-1]))


# ---- quality: the prototype's recipe, Q loudspeakers ----------------------------------------------------------------------------------
QUALITY = ((2, None), (4, None))                       # asserted: the defaults, 2 x 8 and 4 x 4
QUALITY_TABLE = ((2, dict(taps=8)), (2, dict(taps=4)), (2, dict(taps=16)), (4, dict(taps=4)), (4, dict(taps=8)))


@functools.lru_cache(maxsize=None)
def quality_audio(refs):
    """-> mic (L,), far (Q, L), near (L,) float64 at 8 kHz (read-only): echo_cases.quality_audio's recipe with Q loudspeakers and Q
    rooms; with Q = 1 it is that recipe's arrays."""
    L = 512 + (ec.QUALITY_FRAMES - 1) * 128
    far = far_mix(np.stack([ec._peak(bc.speech_like(L, 7 + 31 * q)) for q in range(refs)]))
    near = ec._peak(bc.speech_like(L, 11))
    near[:16000] = 0.0
    rng = np.random.default_rng(0)
    rooms = [ec._room(rng, 640, 120.0, lead=16) for _ in range(refs)]
    mic = sum(np.convolve(f, room)[:L] for f, room in zip(far, rooms)) + near + 1e-3 * rng.standard_normal(L)
    for a in (mic, far, near):
        a.setflags(write=False)
    return mic, far, near


@functools.lru_cache(maxsize=None)
def quality_spec(refs):
    """-> mic (372, 257), far (Q, 372, 257) complex64, and mic, near in float64 for the figures."""
    mic, far, near = quality_audio(refs)
    m, n = ec.spec_of(mic), ec.spec_of(near)
    return m.astype(np.complex64), np.stack([ec.spec_of(ch) for ch in far]).astype(np.complex64), m, n


def quality_of(e_spec, refs):
    """-> (ERLE in dB over the single-talk frames 40 ... 119, SI-SDR in dB of the microphone and of e_spec against the near-end
    spectrum over frames 130 ... end) of a (372, 257) output spectrogram of the recipe with Q loudspeakers."""
    _, _, mic, near = quality_spec(refs)
    erle = 10.0 * np.log10(np.sum(np.abs(mic[ec.ERLE_FRAMES]) ** 2) / np.sum(np.abs(e_spec[ec.ERLE_FRAMES]) ** 2))
    return float(erle), ec.si_sdr_spec(mic[ec.SDR_FIRST:], near[ec.SDR_FIRST:]), ec.si_sdr_spec(e_spec[ec.SDR_FIRST:], near[ec.SDR_FIRST:])


def quality_of_audio(out, refs):
    return quality_of(ec.spec_of(np.asarray(out, np.float64)), refs)


@functools.lru_cache(maxsize=None)
def quality_restatement(refs, params=None):
    """quality_of the float64 restatement with all Q references, on the complex64 spectra."""
    mic, far, _, _ = quality_spec(refs)
    return quality_of(mr.aec_mr_online(mic, far, None if params is None else dict(params)), refs)


@functools.lru_cache(maxsize=None)
def quality_single(refs, which):
    """quality_of tests/echo_ref.py's single-reference restatement at its defaults (K = 8), fed channel 0 ("first") or the mean of
    the channels ("mean")."""
    mic, far, _, _ = quality_spec(refs)
    one = far[0] if which == "first" else far.astype(np.complex128).mean(axis=0).astype(np.complex64)
    return quality_of(er.aec_online(mic, one), refs)


# ---- the long run with silence ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_spec(refs=2):
    """-> mic (LONG_FRAMES, 15), far (Q, LONG_FRAMES, 15) complex64 (read-only): echo_cases.long_spec's recipe with Q loudspeakers,
    every far-end channel digital silence for frames 1000 ... 3000."""
    L = 128 * (LONG_FRAMES - 1) + 64
    rng = np.random.default_rng(3)
    far = far_mix(np.stack([ec._peak(bc.speech_like(L, 21 + 31 * q)) for q in range(refs)]))
    near = ec._peak(bc.speech_like(L, 121))
    far[:, 128 * LONG_SILENCE[0] - 256:128 * LONG_SILENCE[1] + 256] = 0.0
    rooms = [ec._room(rng, 640, 128.0) / np.sqrt(refs) for _ in range(refs)]
    mic = sum(np.convolve(f, room)[:L] for f, room in zip(far, rooms)) + near + 1e-3 * rng.standard_normal(L)
    fs = np.stack([denoise_ref.stft(ch, 512, 128)[:, list(LONG_BINS)].astype(np.complex64) for ch in far])
    ms = denoise_ref.stft(mic, 512, 128)[:, list(LONG_BINS)].astype(np.complex64)
    assert fs.shape[1] == LONG_FRAMES and not fs[:, LONG_SILENCE[0]:LONG_SILENCE[1]].any()
    ms.setflags(write=False)
    fs.setflags(write=False)
    return ms, fs


def main():
    worst = 0.0

    def row(name, b):
        nonlocal worst
        worst = max(worst, b.floor)
        print(f"| {name} | {b.by_arithmetic['plain']:.2e} | {b.by_arithmetic['fma']:.2e} |", flush=True)

    for n_fft, n_frames, refs, kw in cases():
        row(label(n_fft, n_frames, refs, kw), aec_mr_bounds(*parity_spec(n_fft, n_frames, refs), kw))
    for n_frames in SHORT_FRAMES:
        for refs, kw in LAYOUTS:
            row(label(64, n_frames, refs, kw, "short"), aec_mr_bounds(*short_spec(n_frames, refs), kw))
    for refs, kw in TILTED_PARAMS:
        mic, far = parity_spec(64, TILTED_FRAMES, refs)
        row(label(64, TILTED_FRAMES, refs, kw, "tilted"), aec_mr_bounds(tilted(mic), tilted(far), kw))
    print(f"largest floor {worst:.2e} (cap {rb.CAP:g})")
    print("| far end | canceller | ERLE dB | SI-SDR dB in -> out |")
    for refs in (2, 4):
        for which in ("first", "mean"):
            erle, sdr_in, sdr_out = quality_single(refs, which)
            print(f"| Q = {refs} | one reference ({'channel 0' if which == 'first' else 'mean'}), K = 8 | {erle:.2f} | {sdr_in:.2f} -> {sdr_out:.2f} |", flush=True)
        for q, kw in QUALITY_TABLE:
            if q == refs:
                erle, sdr_in, sdr_out = quality_restatement(q, rb._items(kw))
                print(f"| Q = {q} | {q} references, {q} x {kw['taps']} | {erle:.2f} | {sdr_in:.2f} -> {sdr_out:.2f} |", flush=True)


if __name__ == "__main__":
    main()
