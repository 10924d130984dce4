"""The per-bin statistic of tests/solver_bounds.py and one float32 floor per case for the three operators that run a recursion per
bin: adn_spectral_gain, adn_wpe_online and adn_wpe_mc_online -- TEST INFRASTRUCTURE.  The stream, pool and window entry points rest
on these three through bit equalities, so these bounds are what holds their numbers.

`per_bin`, `worst`, `check`, `Frozen`, `EPS`, `MARGIN`, `tilt`, `pow2`, `scale_spec` and `assert_squares_stay_normal` are
solver_bounds', imported and not restated: E[r, b] = max_t |got - ref| / max_t |ref| per (row, bin), a dead bin exactly zero.  The
floor of a case is the largest E of the float32 restatement over every live bin of all three clips / groups, never below 2^-23,
measured when the test runs from the restatements alone (no device figure enters it); the bound is E <= 4 floor.

Two float32 arithmetics for the two WPE recursions: "plain" rounds every product (numpy's complex64 arithmetic, what the written
FLOOR constants were measured with), "fma" follows the header's pairing and order of every multiply-add
(tests/dereverb_stream_ref.py).  The case's floor is the larger of the two; the two floor columns of `solver_bounds.check`'s line
carry them in place of its two summation orders: "pairwise" holds plain, "sequential" holds fma.  The spectral gain has one
arithmetic (contraction off, one step), so both columns hold the same figure.

The spectral gain's state (3, F) is judged the same way, every (clip, row of P / Pmin / S, bin) against its own reference value:
`Bounds.state` is the Bounds of the state laid out as (clips * 3, 1, F).

CAP: a case whose floor exceeds 1e-4 bounds nothing and may not be in a grid.  It is a condition on the case, not a measurement of
the device: measured on the host's inputs the largest floors are 6e-6 (spectral gain), 3e-6 (wpe_online) and 4e-6 (wpe_mc_online),
15 x below it; the smallest structural change of tests/test_recursive_bounds_host.py (E 1.5e-3 in the clip that shows it the least) is
15 x above it.

References and floors are cached per case on the bits of the inputs, so the host file, the GPU files and the table share them.

    python tests/recursive_bounds.py [log of the GPU tests ...]   writes profiles/recursive_bins.md: the host columns from this
                                                                  run, the device column from the "per bin:" lines of the logs
"""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_bounds as sb  # noqa: E402  (first: it completes dereverb_cases -> baseline_cases)
import baseline_cases as bc  # noqa: E402
import baseline_ref as br  # noqa: E402
import denoise_ref  # noqa: E402
import dereverb_mc_stream_cases as msc  # noqa: E402
import dereverb_mc_stream_ref as ms  # noqa: E402
import dereverb_stream_cases as sc  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402

ROOT = sb.ROOT
CAP = 1e-4
ARITHMETICS = ds.ARITHMETICS
COLUMN = dict(plain="pairwise", fma="sequential")      # where solver_bounds.check's line shows each arithmetic
TILTED_FRAMES = 97
TILTED_GAIN = (64, 512)                                # n_fft, defaults
TILTED_ONLINE = (64, 512)                              # n_fft, at the defaults and at the largest parameter set
TILTED_ONLINE_PARAMS = (None, sc.PARITY_PARAMS[2])
TILTED_MC = ((2, 16), (8, 4))                          # (C, K), n_fft 64
POW2_GAIN = 64                                         # n_fft; the spectral gain alone is scale invariant


class Bounds:
    """ref: the float64 restatement (rows, T, F); f32: {arithmetic: the float32 restatement}; by_arithmetic: {arithmetic: its
    largest E}; floors: the same under the two names solver_bounds.check prints; floor: the case's floor."""

    def __init__(self, ref, f32):
        self.ref, self.f32 = ref, f32
        self.by_arithmetic = {a: float(sb.per_bin(f32[a], ref).max()) for a in ARITHMETICS}
        self.floors = {COLUMN[a]: self.by_arithmetic[a] for a in ARITHMETICS}
        self.floor = max(max(self.floors.values()), sb.EPS)


def assert_cap(label, bounds):
    assert bounds.floor <= CAP, (label, bounds.floor)


def state_rows(state):
    """(clips, 3, F) -> (clips * 3, 1, F): every state entry a bin of one frame, so per_bin judges it against its own value."""
    state = np.asarray(state)
    return state.reshape(-1, 1, state.shape[-1])


def _items(params):
    return None if params is None else tuple(sorted(params.items()))


@functools.lru_cache(maxsize=None)
def _spectral(spec, params):
    kw = None if params is None else dict(params)

    def run(dtype):
        outs = [br.spectral_gain(s, kw, dtype=dtype) for s in spec.a]
        return np.stack([m.T for m, _ in outs]), np.stack([st for _, st in outs])

    (m64, s64), (m32, s32) = run(np.float64), run(np.float32)
    b = Bounds(m64, {a: m32 for a in ARITHMETICS})
    b.state = Bounds(state_rows(s64), {a: state_rows(s32) for a in ARITHMETICS})
    return b


def spectral_bounds(spec, params=None):
    """spec (clips, T, F) complex64 -> Bounds of adn_spectral_gain on it from a fresh start: ref (clips, T, F) float64 (M
    transposed to frame-major), and .state the Bounds of the state after the last frame, (clips * 3, 1, F)."""
    return _spectral(sb.Frozen(np.asarray(spec, np.complex64)), _items(params))


def _bins_side_by_side(rows):
    """(rows, ..., T, F) -> (..., T, rows * F): the bins of a restatement are independent and every float32 statement is
    elementwise, so the rows of a case run as more bins of one call, bit for bit what they give alone."""
    return np.concatenate(list(rows), axis=-1)


@functools.lru_cache(maxsize=None)
def _wpe_online(spec, params):
    kw = None if params is None else dict(params)
    n, t, f = spec.a.shape
    wide = _bins_side_by_side(spec.a)
    f32 = {a: np.stack(np.split(ds.wpe_online(wide, kw, dtype=np.float32, arithmetic=a), n, axis=-1)) for a in ARITHMETICS}
    return Bounds(np.stack([ds.wpe_online(s.astype(np.complex128), kw) for s in spec.a]), f32)


def wpe_online_bounds(spec, params=None):
    """spec (rows, T, F) complex64 -> Bounds of adn_wpe_online on it from frame 0."""
    return _wpe_online(sb.Frozen(np.asarray(spec, np.complex64)), _items(params))


@functools.lru_cache(maxsize=None)
def _wpe_mc_online(spec, channels, params):
    kw = dict(params)
    groups = spec.a.reshape((-1, channels) + spec.a.shape[1:])
    n = groups.shape[0]
    wide = _bins_side_by_side(groups)

    def run(a):
        d = ms.wpe_mc_online(wide, kw, dtype=np.float32, arithmetic=a)                 # (C, T, groups * F)
        return np.concatenate(np.split(d, n, axis=-1))

    return Bounds(np.concatenate([ms.wpe_mc_online(g.astype(np.complex128), kw) for g in groups]), {a: run(a) for a in ARITHMETICS})


def wpe_mc_online_bounds(spec, channels, params):
    """spec (groups * C, T, F) complex64, the channels of a group consecutive -> Bounds of adn_wpe_mc_online on it from frame 0
    (rows = groups * C)."""
    return _wpe_mc_online(sb.Frozen(np.asarray(spec, np.complex64)), channels, _items(params))


# ---- the host's inputs: the parity audio through the float64 STFT, rounded to complex64 --------------------------------------------
@functools.lru_cache(maxsize=None)
def gain_spec(n_fft, n_frames):
    """(3, T, F) complex64 (read-only): the spectral baseline's parity clips."""
    x = bc.parity_audio(n_fft, n_frames, 3)
    out = np.stack([denoise_ref.stft(row, n_fft, n_fft // 4).astype(np.complex64) for row in x])
    out.setflags(write=False)
    return out


online_spec = sb.wpe_spec                              # (n_fft, n_frames) -> (3, T, F): dereverb_stream_cases.parity_audio's
mc_spec = sb.mc_spec                                   # (n_fft, n_frames, channels) -> (3 C, T, F): dereverb_mc_stream_cases'


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def gain_label(n_fft, n_frames, kind="parity"):
    return f"spectral_gain {kind} n_fft {n_fft} T {n_frames}"


def online_label(n_fft, n_frames, kw, kind="parity"):
    return f"wpe_online {kind} n_fft {n_fft} T {n_frames} {kw or 'defaults'}"


def mc_label(n_fft, n_frames, ck, extra, kind="parity"):
    return f"wpe_mc_online {kind} n_fft {n_fft} T {n_frames} (C, K) {ck} {extra or 'defaults'}"


def _scaled(spec, factor):
    return spec if factor is None else sb.scale_spec(spec, factor(spec.shape[-1]))


def _gain_rows(n_fft, n_frames, kind, factor=None):
    thunk = lambda: spectral_bounds(_scaled(gain_spec(n_fft, n_frames), factor))  # noqa: E731
    yield gain_label(n_fft, n_frames, kind), thunk
    yield gain_label(n_fft, n_frames, kind) + " state", lambda: thunk().state


def variant_cases():
    """(label, thunk -> Bounds) of every variant case of adn_wpe_mc_online (the channel counts of tests/variant_cover.py that the
    parity grid does not reach) on the host's own inputs."""
    for n_fft, n_frames, ck, extra in msc.variant_cases():
        yield (mc_label(n_fft, n_frames, ck, extra, "variant"),
               lambda a=(n_fft, n_frames, ck[0]), p=msc.params_of(ck, extra): wpe_mc_online_bounds(mc_spec(*a), a[2], p))


def host_cases():
    """(label, thunk -> Bounds) of every parity, tilted, power-of-two and variant case on the host's own inputs; nothing is
    computed before a thunk is called.  A spectral-gain case has two rows: M, and the state."""
    for n_fft in bc.PARITY_N_FFT:
        for n_frames in bc.PARITY_FRAMES:
            yield from _gain_rows(n_fft, n_frames, "parity")
    for n_fft, n_frames, kw in sc.parity_cases():
        yield online_label(n_fft, n_frames, kw), lambda a=(n_fft, n_frames), kw=kw: wpe_online_bounds(online_spec(*a), kw)
    for n_fft, n_frames, ck, extra in msc.parity_cases():
        yield (mc_label(n_fft, n_frames, ck, extra),
               lambda a=(n_fft, n_frames, ck[0]), p=msc.params_of(ck, extra): wpe_mc_online_bounds(mc_spec(*a), a[2], p))
    for n_fft in TILTED_GAIN:
        yield from _gain_rows(n_fft, TILTED_FRAMES, "tilted", sb.tilt)
    for n_fft in TILTED_ONLINE:
        for kw in TILTED_ONLINE_PARAMS:
            yield (online_label(n_fft, TILTED_FRAMES, kw, "tilted"),
                   lambda n_fft=n_fft, kw=kw: wpe_online_bounds(_scaled(online_spec(n_fft, TILTED_FRAMES), sb.tilt), kw))
    for ck in TILTED_MC:
        yield (mc_label(64, TILTED_FRAMES, ck, None, "tilted"),
               lambda ck=ck: wpe_mc_online_bounds(_scaled(mc_spec(64, TILTED_FRAMES, ck[0]), sb.tilt), ck[0], msc.params_of(ck)))
    yield from _gain_rows(POW2_GAIN, TILTED_FRAMES, "pow2", sb.pow2)
    yield from variant_cases()


LINE = re.compile(r"per bin: (.*?): floor pairwise (\S+) sequential (\S+); worst E (\S+) = (\S+) floors \(bound 4\) at row (\d+) bin (\d+)")


def device_figures(logs):
    """{case label: (worst E in floors, E, the run, row, bin, that run's floor)} from the "per bin:" lines of the given logs: the
    worst run of every case (1 and 3 clips / groups)."""
    device = {}
    for path in logs:
        for m in LINE.finditer(open(path).read()):
            label, ratio = m.group(1), float(m.group(5))
            floor = max(float(m.group(2)), float(m.group(3)), sb.EPS)
            base = re.sub(r" \[[^\]]*\]$", "", label)                      # the run within a case: [clips 3], [groups 1]
            if base not in device or ratio > device[base][0]:
                device[base] = (ratio, m.group(4), label[len(base):].strip(" []"), m.group(6), m.group(7), floor)
    return device


def main(logs):
    device = device_figures(logs)
    rows, largest = [], {}
    for label, thunk in host_cases():
        b = thunk()
        d = device.get(label)
        there = "–" if d is None else f"{d[0]:.2f} of {d[5]:.2e} (E {d[1]}; {d[2] + ', ' if d[2] else ''}row {d[3]}, bin {d[4]})"
        plain, fma = b.by_arithmetic["plain"], b.by_arithmetic["fma"]
        rows.append(f"| {label} | {plain:.2e} | {fma:.2e} | {f'{fma / plain:.2f}' if plain > 0 else '–'} | {there} |")
        print(rows[-1], flush=True)
        if d is not None:
            op = label.split()[0] + (" state" if label.endswith(" state") else "")
            for name in (op, op + ", variant cases") if " variant " in label else (op,):
                if name not in largest or d[0] > largest[name][0]:
                    largest[name] = (d[0], label)
    top = "".join(f"* `{op}`: {v:.2f} floors ({label})\n" for op, (v, label) in largest.items()) or "* no device log was given\n"
    text = ("# Per-bin float32 floors of the recursions\n\n"
            "Written by `python tests/recursive_bounds.py <logs of the GPU tests>`.  One row per parity, tilted, power-of-two "
            "and variant (`tests/variant_cover.py`) case of `adn_spectral_gain` (two rows: the magnitudes, and the state, every entry against its own reference value), "
            "`adn_wpe_online` and `adn_wpe_mc_online`.  `E` is the largest error of a (row, bin) relative to that bin's own maximum "
            "over the frames, against the float64 restatement (`tests/recursive_bounds.py`).  The two floor columns are the float32 "
            "restatement's largest `E` in its two arithmetics, \"plain\" (every product rounded: numpy's complex64) and \"fma\" (the "
            "header's pairing and order of every multiply-add), **measured on the host** from the host's own float64 STFT of the "
            "parity audio; the spectral gain has one arithmetic.  The case's floor is the larger of the two and never below 2^-23, "
            "the bound 4 floors, the cap on a floor 1e-4.  The last column is **measured on the MI355X**: the device's largest `E` "
            "in floors of the floor its own test measured (for the parity cases on the downloaded device spectrogram, whose last "
            "bits are not the host's), over every run of the case (1 and 3 clips / groups), with the place it sits.\n\n"
            "Largest device `E` in floors per operator (bound 4):\n\n" + top + "\n"
            "| case | floor, plain | floor, fma | fma / plain | device: worst E in floors of its run's floor, where |\n"
            "|---|---|---|---|---|\n" + "\n".join(rows) + "\n")
    open(os.path.join(ROOT, "profiles", "recursive_bins.md"), "w").write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
