"""The cases of the echo canceller tests (tests/test_echo_host.py, tests/test_gpu_echo.py) -- TEST INFRASTRUCTURE.

Parity audio, per row: L = n_fft + (T - 1) n_fft / 4 samples; far = speech_like(L, seed) and near = speech_like(L, seed + 100),
each scaled to peak 0.5 (a row too short to hold a burst stays zero: its far end is digital silence and every frame is gated);
near[: L // 3] = 0; a room of 5 hop taps of standard_normal * exp(-n / hop) scaled to energy 0.49; mic = conv(far, room)[:L] + near +
1e-3 standard_normal.  The spectra are denoise_ref.stft's, rounded to complex64; the centred transform of L samples has T + 4
frames and a case keeps the first T, so that the frame counts are the ones named.  Three rows per case.

What the short cases of that grid do NOT show: at n_fft 64 the cases of 1, 3, 4 and 5 frames (24 of the 60) are 64 ... 128 samples
long, the far end's first burst has not begun, every frame is gated and e = Y exactly (floor 2^-23).  They hold the gated path, the
stores and the layouts' edges at frame counts around one block of four, and nothing of the update.  The SHORT cases beside the
grid do: the same frame counts cut out of the 97-frame case where its far end is active (frames 80 ..., 75 ... 98 % of the (frame,
bin) cells above `quiet`), run as frames 0 ... T - 1 of a fresh row, one parameter set per lane layout.

    python tests/echo_cases.py      prints the fp32 floor of every parity case on the host's own inputs and the quality table of
                                    the restatement (both are copied into profiles/bench_echo.md)
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_bounds as sb  # noqa: E402  (first: it completes dereverb_cases -> baseline_cases)
import baseline_cases as bc  # noqa: E402
import denoise_ref  # noqa: E402
import echo_ref as er  # noqa: E402
import recursive_bounds as rb  # noqa: E402

SR = 8000
# F = 33 and 257: neither is a multiple of the 32, 16 or 8 bins of a workgroup (G = 8, 16, 32 lanes per bin).  The frame counts sit
# around a block of four, the largest ring (D + K = 40 frames) and several wraps of the small ones.
PARITY_N_FFT = (64, 512)
PARITY_FRAMES = {64: (1, 3, 4, 5, 23, 24, 40, 97), 512: (5, 40)}
PARITY_ROWS = (1, 3)
# one per lane layout and its edges: G = 8 full, G = 8 at one lane, G = 16 at its first and last tap count, G = 32 likewise
PARITY_PARAMS = (None, dict(taps=1), dict(taps=9, delay=2, forget=0.95), dict(taps=16, forget=0.97),
                 dict(taps=17, delay=1, forget=0.99), dict(taps=32, delay=8, forget=0.984375))
PARAM_IDS = ("defaults", "K1", "K9-D2", "K16", "K17-D1", "K32-D8")
SHORT_FRAMES, SHORT_FROM = (1, 3, 4, 5), 80            # frames SHORT_FROM ... of the (64, 97) case as a fresh row: an active far end
# one per lane layout, all at delay 0: with a delay the first D frames see x~ = 0 and a case this short would not adapt at all
SHORT_PARAMS = (PARITY_PARAMS[0], PARITY_PARAMS[3], dict(taps=32, forget=0.984375))
SHORT_IDS = ("defaults", "K16", "K32")
TILTED_FRAMES = 97
TILTED_PARAMS = (None, PARITY_PARAMS[5])
E2E_FRAMES = 97
LONG_FRAMES, LONG_SILENCE = 3750, (1000, 3000)
LONG_BINS = tuple(range(2, 257, 17))                 # 15 of the 257 bins: the host run is a Python loop over frames


def parity_length(n_fft, n_frames):
    return n_fft + (n_frames - 1) * (n_fft // 4)


def _peak(x, peak=0.5):
    m = np.abs(x).max()
    return x * (peak / m) if m > 0 else x


def _room(rng, taps, decay, lead=0):
    room = rng.standard_normal(taps) * np.exp(-np.arange(taps) / decay)
    room[:lead] = 0.0
    return room * np.sqrt(0.49 / np.sum(room ** 2))


@functools.lru_cache(maxsize=None)
def parity_audio(n_fft, n_frames):
    """-> mic, far, near, each (3, L) float64 (read-only)."""
    L, hop = parity_length(n_fft, n_frames), n_fft // 4
    out = []
    for c in range(3):
        seed = 1000 * n_fft + 10 * n_frames + c
        rng = np.random.default_rng(seed + 50000)
        far, near = _peak(bc.speech_like(L, seed)), _peak(bc.speech_like(L, seed + 100))
        near[: L // 3] = 0.0
        room = _room(rng, 5 * hop, hop)
        out.append((np.convolve(far, room)[:L] + near + 1e-3 * rng.standard_normal(L), far, near))
    arrays = tuple(np.stack([row[i] for row in out]) for i in range(3))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def parity_spec(n_fft, n_frames):
    """-> mic, far, each (3, T, F) complex64 (read-only)."""
    mic, far, _ = parity_audio(n_fft, n_frames)
    out = tuple(np.stack([denoise_ref.stft(row, n_fft, n_fft // 4)[:n_frames].astype(np.complex64) for row in a]) for a in (mic, far))
    for a in out:
        a.setflags(write=False)
    return out


def short_spec(n_frames):
    """-> mic, far, each (3, n_frames, 33) complex64 (read-only): the short cases whose far end is NOT silent."""
    out = tuple(np.ascontiguousarray(s[:, SHORT_FROM:SHORT_FROM + n_frames]) for s in parity_spec(64, 97))
    assert all((np.abs(out[1][c]) ** 2 > 1e-8).mean() > 0.5 for c in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def parity_cases():
    """(n_fft, n_frames, params or None) of every parity case."""
    for n_fft in PARITY_N_FFT:
        for n_frames in PARITY_FRAMES[n_fft]:
            for params in PARITY_PARAMS:
                yield n_fft, n_frames, params


def label(n_fft, n_frames, kw, kind="parity"):
    return f"aec_online {kind} n_fft {n_fft} T {n_frames} {kw or 'defaults'}"


@functools.lru_cache(maxsize=None)
def _bounds(mic, far, params):
    kw = None if params is None else dict(params)
    n = mic.a.shape[0]
    wide_m, wide_f = (np.concatenate(list(s.a), axis=-1) for s in (mic, far))     # the rows as more bins of one call
    f32 = {a: np.stack(np.split(er.aec_online(wide_m, wide_f, kw, dtype=np.float32, arithmetic=a), n, axis=-1)) for a in rb.ARITHMETICS}
    ref = np.stack([er.aec_online(m.astype(np.complex128), f.astype(np.complex128), kw) for m, f in zip(mic.a, far.a)])
    return rb.Bounds(ref, f32)


def aec_bounds(mic, far, params=None):
    """mic, far (rows, T, F) complex64 -> recursive_bounds.Bounds of adn_aec_online on them from frame 0."""
    return _bounds(sb.Frozen(np.asarray(mic, np.complex64)), sb.Frozen(np.asarray(far, np.complex64)), rb._items(params))


def tilted(spec):
    return sb.scale_spec(spec, sb.tilt(spec.shape[-1]))


# ---- quality: the prototype's recipe --------------------------------------------------------------------------------------------
QUALITY_FRAMES = 372
ERLE_FRAMES = slice(40, 120)
SDR_FIRST = 130


@functools.lru_cache(maxsize=None)
def quality_audio():
    """-> mic, far, near (L,) float64 at 8 kHz (read-only): n_fft 512, hop 128, 372 frames = 48 000 samples; the near end is silent
    for the first 2 s (single talk), then both talk."""
    L = 512 + (QUALITY_FRAMES - 1) * 128
    far, near = _peak(bc.speech_like(L, 7)), _peak(bc.speech_like(L, 11))
    near[:16000] = 0.0
    rng = np.random.default_rng(0)
    room = _room(rng, 640, 120.0, lead=16)
    mic = np.convolve(far, room)[:L] + near + 1e-3 * rng.standard_normal(L)
    for a in (mic, far, near):
        a.setflags(write=False)
    return mic, far, near


def spec_of(x):
    return denoise_ref.stft(x, 512, 128)[:QUALITY_FRAMES]


def si_sdr_spec(est, ref):
    """SI-SDR in dB of a spectrogram against a reference spectrogram, both as one complex vector."""
    est, ref = np.ravel(est), np.ravel(ref)
    target = (np.vdot(ref, est) / np.vdot(ref, ref)) * ref
    return float(10.0 * np.log10(np.sum(np.abs(target) ** 2) / np.sum(np.abs(est - target) ** 2)))


def quality_of(e_spec):
    """-> (ERLE in dB over the single-talk frames 40 ... 119, SI-SDR in dB of the microphone and of e_spec against the near-end
    spectrum over frames 130 ... end) of a (372, 257) output spectrogram of the quality recipe."""
    mic, _, near = (spec_of(a) for a in quality_audio())
    erle = 10.0 * np.log10(np.sum(np.abs(mic[ERLE_FRAMES]) ** 2) / np.sum(np.abs(e_spec[ERLE_FRAMES]) ** 2))
    return float(erle), si_sdr_spec(mic[SDR_FIRST:], near[SDR_FIRST:]), si_sdr_spec(e_spec[SDR_FIRST:], near[SDR_FIRST:])


@functools.lru_cache(maxsize=None)
def quality_restatement():
    """quality_of the float64 restatement at the defaults, on the complex64 spectra."""
    mic, far, _ = quality_audio()
    return quality_of(er.aec_online(spec_of(mic).astype(np.complex64), spec_of(far).astype(np.complex64)))


def quality_of_audio(out):
    """quality_of the first 372 frames of the STFT of an end-to-end result (48 000 samples)."""
    return quality_of(spec_of(np.asarray(out, np.float64)))


# ---- the long run with silence ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_spec():
    """-> mic, far (LONG_FRAMES, 15) complex64 (read-only): 60 s of the parity recipe at n_fft 512 / hop 128 on a comb of bins, the
    far end digital silence for frames 1000 ... 3000."""
    L = 128 * (LONG_FRAMES - 1) + 64
    rng = np.random.default_rng(3)
    far, near = _peak(bc.speech_like(L, 21)), _peak(bc.speech_like(L, 121))
    far[128 * LONG_SILENCE[0] - 256:128 * LONG_SILENCE[1] + 256] = 0.0
    mic = np.convolve(far, _room(rng, 640, 128.0))[:L] + near + 1e-3 * rng.standard_normal(L)
    fs = denoise_ref.stft(far, 512, 128)[:, list(LONG_BINS)].astype(np.complex64)
    ms = denoise_ref.stft(mic, 512, 128)[:, list(LONG_BINS)].astype(np.complex64)
    assert fs.shape[0] == LONG_FRAMES and not fs[LONG_SILENCE[0]:LONG_SILENCE[1]].any()
    ms.setflags(write=False)
    fs.setflags(write=False)
    return ms, fs


def main():
    worst = 0.0
    for n_fft, n_frames, kw in parity_cases():
        b = aec_bounds(*parity_spec(n_fft, n_frames), kw)
        worst = max(worst, b.floor)
        print(f"| {label(n_fft, n_frames, kw)} | {b.by_arithmetic['plain']:.2e} | {b.by_arithmetic['fma']:.2e} |", flush=True)
    for n_frames in SHORT_FRAMES:
        for kw in SHORT_PARAMS:
            b = aec_bounds(*short_spec(n_frames), kw)
            worst = max(worst, b.floor)
            print(f"| {label(64, n_frames, kw, 'short')} | {b.by_arithmetic['plain']:.2e} | {b.by_arithmetic['fma']:.2e} |", flush=True)
    for n_fft in PARITY_N_FFT:
        for kw in TILTED_PARAMS:
            mic, far = parity_spec(n_fft, TILTED_FRAMES if n_fft == 64 else 40)
            b = aec_bounds(tilted(mic), tilted(far), kw)
            worst = max(worst, b.floor)
            print(f"| {label(n_fft, mic.shape[1], kw, 'tilted')} | {b.by_arithmetic['plain']:.2e} | {b.by_arithmetic['fma']:.2e} |", flush=True)
    print(f"largest floor {worst:.2e} (cap {rb.CAP:g})")
    erle, sdr_in, sdr_out = quality_restatement()
    print(f"quality, float64 restatement at the defaults: ERLE {erle:.2f} dB over frames 40 ... 119; SI-SDR against the near end over "
          f"frames 130 ... end {sdr_in:.2f} -> {sdr_out:.2f} dB")


if __name__ == "__main__":
    main()
