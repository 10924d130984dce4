"""Float64 numpy restatement of the resampler inside a stream (include/adn.h, "resample stream"): the plan functions and a
push-by-push resampler built on resample_ref.design.  Test infrastructure (like oracle/): the package does not import it.

For a stream that has received n samples, output m is final once m * down + half < n * up; an ended stream of length L has
ceil(L * up / down) outputs and reads zeros from L on.  ``StreamRef`` keeps only the last H samples between pushes and asserts
that no output ever needs an older one.
"""
import numpy as np

import resample_ref
from resample_ref import ZEROS, ratio


def half_of(up, down):
    return ZEROS * max(up, down)


def emitted(n, src_rate, dst_rate, final=False):
    up, down = ratio(src_rate, dst_rate)
    if up == down:
        return n
    if final:
        return -(-n * up // down)
    half = half_of(up, down)
    return 0 if n * up <= half else (n * up - half - 1) // down + 1


def history(src_rate, dst_rate):
    up, down = ratio(src_rate, dst_rate)
    if up == down:
        return 0
    return 2 * (half_of(up, down) // up) + -(-down // up) + 1


def latency(src_rate, dst_rate):
    up, down = ratio(src_rate, dst_rate)
    return 0 if up == down else -(-half_of(up, down) // up)


def first_input(m, src_rate, dst_rate):
    """Smallest i with |m * down - i * up| <= half (may be negative: zero extension)."""
    up, down = ratio(src_rate, dst_rate)
    return -((half_of(up, down) - m * down) // up)


def last_input(m, src_rate, dst_rate):
    up, down = ratio(src_rate, dst_rate)
    return (m * down + half_of(up, down)) // up


class StreamRef:
    """One stream, float64: push(block) -> the outputs that became final, flush() -> the rest."""

    def __init__(self, src_rate, dst_rate):
        self.src, self.dst = int(src_rate), int(dst_rate)
        self.up, self.down = ratio(src_rate, dst_rate)
        self.h = resample_ref.design(self.up, self.down)
        self.half = half_of(self.up, self.down)
        self.H = history(src_rate, dst_rate)
        self.reset()

    def reset(self):
        self.received = 0
        self.hist = np.zeros(0)                 # the last min(H, received) samples

    def _outputs(self, x, first, m0, m1, end, final):
        """Outputs [m0, m1) from `x`, which holds samples [first, end) of the stream."""
        up, down, half = self.up, self.down, self.half
        m = np.arange(m0, m1, dtype=np.int64)
        k = half // up
        i = (m * down // up)[:, None] - k + np.arange(2 * k + 2, dtype=np.int64)[None, :]
        j = m[:, None] * down - i * up
        ok = (np.abs(j) <= half) & (i >= 0) & (i < end)
        if not final:                           # every input of a final output has arrived
            assert np.all((np.abs(j) > half) | (i < end))
        assert np.all(i[ok] >= first), "an output needs a sample older than the carried history"
        c = np.where(ok, self.h[np.clip(j, -half, half) + half], 0.0)
        v = np.where(ok, x[np.clip(i - first, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
        return (c * v).sum(axis=1)

    def _step(self, block, final):
        block = np.asarray(block, dtype=np.float64)
        before, end = self.received, self.received + len(block)
        x = np.concatenate([self.hist, block])
        first = before - len(self.hist)
        if self.up == self.down:
            out = block.copy()
        else:
            out = self._outputs(x, first, emitted(before, self.src, self.dst), emitted(end, self.src, self.dst, final), end, final)
        self.received = end
        self.hist = x[max(len(x) - self.H, 0):] if self.H else np.zeros(0)
        return out

    def push(self, block):
        return self._step(block, False)

    def flush(self):
        out = self._step(np.zeros(0), True)
        self.reset()
        return out


SANITY_PAIRS = ((44100, 8000), (8000, 44100), (48000, 8000), (8000, 48000), (16000, 8000), (44100, 48000), (3, 2), (8000, 8000))


def split_patterns(length, seed):
    """A dozen ways to cut `length` samples into pushes: whole, fixed sizes, and seeded mixes of long and very short pushes."""
    rng = np.random.default_rng(seed)
    pats = [[length], [1] * min(length, 40) + [length], [480] * (length // 480 + 1), [7] * 30 + [1000] * (length // 1000 + 1),
            [length - 1, 1], [1, length - 1]]
    while len(pats) < 12:
        sizes = []
        while sum(sizes) < length:
            sizes.append(int(rng.integers(1, 8)) if len(sizes) % 3 == 1 else int(rng.integers(1, 1201)))
        pats.append(sizes)
    return pats


def run_splits(x, src_rate, dst_rate, sizes):
    s = StreamRef(src_rate, dst_rate)
    pos, outs = 0, []
    for size in sizes:
        if pos >= len(x):
            break
        outs.append(s.push(x[pos:pos + size]))
        pos += size
    assert pos >= len(x)
    outs.append(s.flush())
    return np.concatenate(outs)


def sanity(length=1501):
    """The concatenation of the pushes equals resample_ref.resample_ref of the whole, to 1e-12, for every pair and split."""
    worst = 0.0
    for src, dst in SANITY_PAIRS:
        x = np.random.default_rng([src, dst, length]).uniform(-1.0, 1.0, length)
        want = resample_ref.resample_ref(x, src, dst)[0]
        for sizes in split_patterns(length, [src, dst]):
            got = run_splits(x, src, dst, sizes)
            assert got.shape == want.shape, (src, dst, got.shape, want.shape)
            worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 1e-12, worst
    return worst


if __name__ == "__main__":
    print("worst difference from resample_ref over all pairs and splits:", sanity())
