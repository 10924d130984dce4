"""One statistic and one float32 floor for the three batch solvers adn_wpe, adn_wpe_mc and adn_mvdr -- TEST INFRASTRUCTURE.

For a result `got` and the float64 restatement `ref`, both (rows, T, F), every (row, bin) is judged against its own level:

    scale[r, b] = max_t |ref[r, t, b]|          E[r, b] = max_t |got - ref| / scale[r, b]          (scale > 0)

and a bin with scale == 0 has to be exactly zero in `got`.  The floor of a case is the largest E of the float32 restatement over
every live bin, all three clips / groups, both reference channels (MVDR) and both summation orders of the restatement ("pairwise",
numpy's; "sequential", frame after frame, the order include/adn.h states), never below 2^-23.  It is measured when the test runs,
from the restatements alone: no device figure enters it.  The bound is E <= 4 floor, the project's margin over a float32 floor.
The maximum over the bins is deliberate: a single bin's float32 error varies by 30 x between the bins of one clip.

References and floors are cached per case on the bits of the inputs, so the host file, the GPU files and the table share them.

    python tests/solver_bounds.py [log of the GPU tests ...]      writes profiles/solver_bins.md: the host columns from this run,
                                                                  the device column from the "per bin:" lines of the given logs
"""
import functools
import hashlib
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_ref as bf  # noqa: E402
import denoise_ref  # noqa: E402
import dereverb_cases as dc  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_ref as mr  # noqa: E402
import dereverb_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0
EPS = 2.0 ** -23
ORDERS = ("pairwise", "sequential")
TILTED_FRAMES = 97
TILTED_WPE = (64, 512)                       # n_fft, defaults
TILTED_MC = ((2, 10), (8, 4))                # (C, K), n_fft 64
TILTED_MVDR = (4, 8)                         # C, n_fft 64, both reference channels


class Frozen:
    """A read-only array that hashes and compares by its bits: the key of the caches below."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a).copy()
        self.a.setflags(write=False)
        self.key = (self.a.shape, self.a.dtype.str, hashlib.sha1(self.a.tobytes()).digest())

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, Frozen) and self.key == other.key


class Bounds:
    """ref: float64 pairwise restatement, (rows, T, F) complex128 (MVDR: {ref_channel: (groups, T, F)}); f32: {order: the float32
    restatement, shaped like ref}; floors: {order: its largest E}; floor: the case's floor."""

    def __init__(self, ref, f32):
        self.ref, self.f32 = ref, f32
        self.floors = {o: max(float(per_bin(g, r).max()) for _, g, r in self.views(o)) for o in ORDERS}
        self.floor = max(max(self.floors.values()), EPS)

    def views(self, order):
        """[(reference channel or None, the float32 restatement of `order`, the reference)], each (rows, T, F)."""
        if isinstance(self.ref, dict):
            return [(k, self.f32[order][k], self.ref[k]) for k in self.ref]
        return [(None, self.f32[order], self.ref)]


def per_bin(got, ref):
    """got, ref (rows, T, F) -> E (rows, F): max_t |got - ref| / max_t |ref| of every live bin; a bin the reference has all zero
    gives 0 if `got` is exactly zero there and inf if not."""
    ref = np.asarray(ref, np.complex128)
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == ref.shape and ref.ndim == 3
    scale, err = np.abs(ref).max(axis=1), np.abs(got - ref).max(axis=1)
    live = scale > 0
    with np.errstate(all="ignore"):
        e = np.where(live, err / np.where(live, scale, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(e), np.inf, e)


def worst(got, ref):
    """-> (largest E, row, bin)."""
    e = per_bin(got, ref)
    r, b = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[r, b]), int(r), int(b)


def check(label, got, ref, bounds):
    """Print the case's line, then assert E <= 4 floor for every row and bin.  -> the largest E / floor."""
    e, r, b = worst(got, ref)
    print(f"per bin: {label}: floor pairwise {bounds.floors['pairwise']:.3g} sequential {bounds.floors['sequential']:.3g}; "
          f"worst E {e:.3g} = {e / bounds.floor:.2f} floors (bound {MARGIN:g}) at row {r} bin {b}")
    assert e <= MARGIN * bounds.floor, (label, e, bounds.floor, r, b)
    return e / bounds.floor


def _items(params):
    return None if params is None else tuple(sorted(params.items()))


@functools.lru_cache(maxsize=None)
def _wpe(spec, params):
    kw = None if params is None else dict(params)
    run = lambda dtype, order: np.stack([dr.wpe(s, kw, dtype=dtype, order=order) for s in spec.a])  # noqa: E731
    return Bounds(run(np.float64, "pairwise"), {o: run(np.float32, o) for o in ORDERS})


def wpe_bounds(spec, params=None):
    """spec (clips, T, F) complex64 -> Bounds of adn_wpe on it."""
    return _wpe(Frozen(np.asarray(spec, np.complex64)), _items(params))


@functools.lru_cache(maxsize=None)
def _wpe_mc(spec, channels, params):
    kw = None if params is None else dict(params)
    groups = spec.a.reshape((-1, channels) + spec.a.shape[1:])
    run = lambda dtype, order: np.concatenate([mr.wpe_mc(g, kw, dtype=dtype, order=order) for g in groups])  # noqa: E731
    return Bounds(run(np.float64, "pairwise"), {o: run(np.float32, o) for o in ORDERS})


def wpe_mc_bounds(spec, channels, params=None):
    """spec (groups * C, T, F) complex64, the channels of a group consecutive -> Bounds of adn_wpe_mc on it (rows = groups * C)."""
    return _wpe_mc(Frozen(np.asarray(spec, np.complex64)), channels, _items(params))


@functools.lru_cache(maxsize=None)
def _mvdr(spec, mags, channels, params, refs):
    kw = dict(params or ())
    sg = spec.a.reshape((-1, channels) + spec.a.shape[1:])
    mg = mags.a.reshape((-1, channels) + mags.a.shape[1:])

    def run(dtype, order):
        return {r: np.stack([bf.mvdr(s, m, dict(kw, ref_channel=r), dtype=dtype, order=order) for s, m in zip(sg, mg)]) for r in refs}

    return Bounds(run(np.float64, "pairwise"), {o: run(np.float32, o) for o in ORDERS})


def mvdr_bounds(spec, mags, channels, params=None, refs=None):
    """spec (groups * C, T, F) complex64, mags (groups * C, F, width) float32 -> Bounds of adn_mvdr on them at every reference
    channel of `refs` (both ends by default): ref and f32 are {ref_channel: (groups, T, F)}, the floor is over all of them."""
    refs = bc.refs_of(channels) if refs is None else tuple(refs)
    params = {k: v for k, v in (params or {}).items() if k != "ref_channel"} or None
    return _mvdr(Frozen(np.asarray(spec, np.complex64)), Frozen(np.asarray(mags, np.float32)), channels, _items(params), refs)


# ---- the host's inputs: the parity audio through the float64 STFT, rounded to complex64 --------------------------------------------
@functools.lru_cache(maxsize=None)
def wpe_spec(n_fft, n_frames):
    """(3, T, F) complex64 (read-only)."""
    x = dc.parity_audio(n_fft, n_frames, 3)
    out = np.stack([denoise_ref.stft(row, n_fft, n_fft // 4).astype(np.complex64) for row in x])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mc_spec(n_fft, n_frames, channels):
    """(3 * C, T, F) complex64 (read-only), the channels of a group consecutive."""
    out = np.concatenate([mc.group_specs(n_fft, n_frames, channels, g) for g in range(3)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mvdr_inputs(n_fft, n_frames, channels, uniform_mask=False):
    """-> spec (3 * C, T, F) complex64, mags (3 * C, F, T) float32 (read-only)."""
    groups = [bc.group_specs(n_fft, n_frames, channels, g) for g in range(3)]
    mags = np.concatenate([bc.magnitudes_of(s, dict(uniform_mask=uniform_mask)) for s in groups])
    spec = np.concatenate(groups)
    spec.setflags(write=False)
    mags.setflags(write=False)
    return spec, mags


def tilt(n_bins):
    """An 80 dB tilt over the bins: 10^(-4 b / (F - 1))."""
    return 10.0 ** (-4.0 * np.arange(n_bins) / (n_bins - 1))


def pow2(n_bins):
    """A power of two per bin, 2^-((5 b) mod 13): exact in every format."""
    return 2.0 ** -((5 * np.arange(n_bins)) % 13).astype(np.float64)


def scale_spec(spec, factor):
    """(..., T, F) complex64 times a factor per bin, rounded once to complex64."""
    return (np.asarray(spec).astype(np.complex128) * factor).astype(np.complex64)


def scale_mags(mags, factor):
    """(..., F, width) float32 times a factor per bin, rounded once to float32."""
    return (np.asarray(mags).astype(np.float64) * factor[:, None]).astype(np.float32)


def assert_squares_stay_normal(*arrays):
    """The power-of-two argument holds only while no square of a non-zero component leaves float32's normal range."""
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    for a in arrays:
        a = np.asarray(a)
        v = np.concatenate([a.real.ravel(), a.imag.ravel()]) if np.iscomplexobj(a) else a.ravel()
        sq = v[v != 0].astype(np.float64) ** 2
        assert sq.size and tiny <= sq.min() and sq.max() <= huge, (float(sq.min()), float(sq.max()))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def wpe_label(n_fft, n_frames, kw, kind="parity"):
    return f"wpe {kind} n_fft {n_fft} T {n_frames} {kw or 'defaults'}"


def mc_label(n_fft, n_frames, ck, extra, kind="parity"):
    return f"wpe_mc {kind} n_fft {n_fft} T {n_frames} (C, K) {ck} {extra or 'defaults'}"


def mvdr_label(n_fft, n_frames, channels, extra, kind="parity"):
    return f"mvdr {kind} n_fft {n_fft} T {n_frames} C {channels} {extra or 'defaults'}"


def mvdr_mags(mags, extra):
    """The parity case's magnitudes at its own pitch: `mag_extra` NaN columns beyond T, as the device test has them."""
    pad = (extra or {}).get("mag_extra", 0)
    return mags if not pad else np.concatenate([mags, np.full(mags.shape[:2] + (pad,), np.nan, np.float32)], axis=2)


def _mvdr_case(n_fft, n_frames, channels, extra, factor=None):
    spec, mags = mvdr_inputs(n_fft, n_frames, channels, bool(extra.get("uniform_mask")))
    if factor is not None:
        spec, mags = scale_spec(spec, factor(spec.shape[-1])), scale_mags(mags, factor(spec.shape[-1]))
    return mvdr_bounds(spec, mvdr_mags(mags, extra), channels, bc.params_of(extra, 0))


def _scaled(spec, factor):
    return spec if factor is None else scale_spec(spec, factor(spec.shape[-1]))


VARIANT_CAP = 5e-4                           # a variant case whose floor exceeds this bounds nothing and may not be in a table


def mvdr_variant_extra(channels, refs):
    """What a variant case's label carries: nothing at both ends of the reference channel, the channel where it names one."""
    return None if tuple(refs) == bc.refs_of(channels) else dict(ref_channel=refs[0])


def variant_cases():
    """(label, thunk -> Bounds) of every variant case (the kernel layouts of tests/variant_cover.py that the parity grids do not
    reach) on the host's own inputs."""
    for n_fft, n_frames, kw in dc.variant_cases():
        yield wpe_label(n_fft, n_frames, kw, "variant"), lambda a=(n_fft, n_frames), kw=kw: wpe_bounds(wpe_spec(*a), kw)
    for n_fft, n_frames, ck, extra in mc.variant_cases():
        yield (mc_label(n_fft, n_frames, ck, extra, "variant"),
               lambda a=(n_fft, n_frames, ck[0]), p=mc.params_of(ck, extra): wpe_mc_bounds(mc_spec(*a), a[2], p))
    for n_fft, n_frames, channels, refs in bc.variant_cases():
        yield (mvdr_label(n_fft, n_frames, channels, mvdr_variant_extra(channels, refs), "variant"),
               lambda a=(n_fft, n_frames, channels), r=refs: mvdr_bounds(*mvdr_inputs(*a), a[2], None, r))


def host_cases():
    """(label, thunk -> Bounds) of every parity, tilted, power-of-two and variant case on the host's own inputs; nothing is
    computed before a thunk is called."""
    for n_fft, n_frames, kw in dc.parity_cases():
        yield wpe_label(n_fft, n_frames, kw), lambda a=(n_fft, n_frames), kw=kw: wpe_bounds(wpe_spec(*a), kw)
    for n_fft, n_frames, ck, extra in mc.parity_cases():
        yield (mc_label(n_fft, n_frames, ck, extra),
               lambda a=(n_fft, n_frames, ck[0]), p=mc.params_of(ck, extra): wpe_mc_bounds(mc_spec(*a), a[2], p))
    for case in bc.parity_cases():
        yield mvdr_label(*case), lambda case=case: _mvdr_case(*case)
    for kind, factor in (("tilted", tilt), ("pow2", pow2)):
        for n_fft in TILTED_WPE if kind == "tilted" else TILTED_WPE[:1]:
            yield (wpe_label(n_fft, TILTED_FRAMES, None, kind),
                   lambda n_fft=n_fft, f=factor: wpe_bounds(_scaled(wpe_spec(n_fft, TILTED_FRAMES), f)))
        for ck in TILTED_MC:
            yield (mc_label(64, TILTED_FRAMES, ck, None, kind),
                   lambda ck=ck, f=factor: wpe_mc_bounds(_scaled(mc_spec(64, TILTED_FRAMES, ck[0]), f), ck[0], mc.params_of(ck)))
        for channels in TILTED_MVDR:
            yield (mvdr_label(64, TILTED_FRAMES, channels, None, kind),
                   lambda c=channels, f=factor: _mvdr_case(64, TILTED_FRAMES, c, dict(), f))
    yield from variant_cases()


def main(logs):
    device = {}
    for path in logs:
        for m in re.finditer(r"per bin: (.*?): floor pairwise (\S+) sequential (\S+); worst E (\S+) = (\S+) floors \(bound 4\) at row (\d+) bin (\d+)", open(path).read()):
            label, ratio = m.group(1), float(m.group(5))
            floor = max(float(m.group(2)), float(m.group(3)), EPS)
            base = re.sub(r" \[[^\]]*\]$", "", label)                      # the run within a case: [clips 3], [ref 7 groups 1]
            if base not in device or ratio > device[base][0]:
                device[base] = (ratio, m.group(4), label[len(base):].strip(" []"), m.group(6), m.group(7), floor)
    rows, largest = [], {}
    for label, thunk in host_cases():
        b = thunk()
        d = device.get(label)
        there = "–" if d is None else f"{d[0]:.2f} of {d[5]:.2e} (E {d[1]}; {d[2] + ', ' if d[2] else ''}row {d[3]}, bin {d[4]})"
        spread = f"{b.floors['sequential'] / b.floors['pairwise']:.2f}" if b.floors["pairwise"] > 0 else "–"
        rows.append(f"| {label} | {b.floors['pairwise']:.2e} | {b.floors['sequential']:.2e} | {spread} | {there} |")
        print(rows[-1], flush=True)
        if d is not None:
            for op in (label.split()[0], label.split()[0] + ", variant cases") if " variant " in label else (label.split()[0],):
                if op not in largest or d[0] > largest[op][0]:
                    largest[op] = (d[0], label)
    top = "".join(f"* `{op}`: {v:.2f} floors ({label})\n" for op, (v, label) in sorted(largest.items())) or "* no device log was given\n"
    text = ("# Per-bin float32 floors of the batch solvers\n\n"
            "Written by `python tests/solver_bounds.py <logs of the GPU tests>`.  One row per parity, tilted, power-of-two and variant "
            "case (the kernel layouts of `tests/variant_cover.py` that the parity grids do not reach) of "
            "`adn_wpe`, `adn_wpe_mc` and `adn_mvdr`.  `E` is the largest error of a (row, bin) relative to that bin's own maximum over "
            "the frames, against the float64 restatement (`tests/solver_bounds.py`).  The two floor columns are the float32 "
            "restatement's largest `E` with numpy's pairwise sums over t and with sequential sums, **measured on the host** from the "
            "host's own float64 STFT of the parity audio; the case's floor is the larger of the two and never below 2^-23, the bound "
            "4 floors.  The last column is **measured on the MI355X**: the device's largest `E` in floors, and the floor its own test measured "
            "(for the parity cases on the downloaded device spectrogram, whose last bits are not the host's: where T is a few "
            "frames the solve is conditioned by the loading alone and the two floors differ by up to 3 x, which is why a floor is "
            "measured on the very input the device ran on), over every run of the case (1 and 3 clips / groups, both reference channels), with the place it sits.\n\n"
            "Largest device `E` in floors per operator (bound 4):\n\n" + top + "\n"
            "| case | floor, pairwise | floor, sequential | sequential / pairwise | device: worst E in floors of its run's floor, where |\n"
            "|---|---|---|---|---|\n" + "\n".join(rows) + "\n")
    open(os.path.join(ROOT, "profiles", "solver_bins.md"), "w").write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
