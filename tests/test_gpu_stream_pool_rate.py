"""StreamPool at each feed's own rate on the device (audiodenoiser_amd/stream.py, csrc/stream_resample_kernels.hip, include/adn.h
"stream pool at a rate"): the rows of adn_stream_pool_emit_rate / adn_stream_pool_push_rate against the lockstep resampler and the
offline one, and the pool against the solo stream, StreamDenoiser(n_streams=1, input_rate=rate).

Bounds (none derived here):
* "bit for bit": torch.equal -- a row is DEFINED as an adn_resample_stream call of one stream, whose outputs are adn_resample's of
  the finished signal; the pool as independent instances of the stream (with model.set_batch_invariant(True)).
* against float64: tests/test_gpu_stream_resample.py's per-element bound 1.01 (taps + 2) 2^-24 sum |h||x| from
  resample_ref.resample_ref; exactly 0 where that sum is 0.
* without batch invariance 2e-5 of the maximum, fp16 1e-2 of the fp32 maximum: the bounds of
  tests/test_gpu_stream_resample.py::test_denoiser_at_a_rate_without_batch_invariance_and_fp16.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref  # noqa: E402
import stream_resample_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PLANS = ((64, 16, 16, 1, 0), (512, 128, 48, 8, 4))              # n_fft, hop, W, B, A
RATES = (48000, 44100, 16000, 8000)
WORK = 8000
ADN_ERR_INVALID = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _net(weights_np, dev, dtype="f32"):
    from audiodenoiser_amd.model import UNet
    m = UNet(1, 1)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights_np.items()}, strict=True)
    return m.to(dev).eval().set_compute_dtype(dtype)


@pytest.fixture(scope="module")
def net(weights_np, dev):
    m = _net(weights_np, dev)
    yield m
    m._workspace = None


@pytest.fixture(scope="module")
def net16(weights_np, dev):
    m = _net(weights_np, dev, "f16")
    yield m
    m._workspace = None


def _pool(model, plan, **kw):
    from audiodenoiser_amd import StreamPool
    n_fft, hop, w, b, a = plan
    kw.setdefault("input_rates", RATES)
    return StreamPool(model, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a, **kw)


def _signal(tag, length):
    x = np.random.default_rng(list(tag) + [length]).uniform(-1.0, 1.0, length).astype(np.float32)
    x.setflags(write=False)
    return x


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _table(rows):
    from audiodenoiser_amd._lib import StreamPoolRateRow
    return (StreamPoolRateRow * len(rows))(*[StreamPoolRateRow(*r) for r in rows])


# ---- the rows of one call against the lockstep resampler ----------------------------------------------------------------------------
def _cuts(tag, length, h):
    """Pushes of a stream of `length` samples: a short one, one longer than 2 H, one shorter than H, then seeded sizes."""
    rng = np.random.default_rng(list(tag) + [length, 5])
    sizes = [3, 2 * h + 5, max(h - 1, 1)]
    while sum(sizes) < length:
        sizes.append(int(rng.integers(1, 8)) if len(sizes) % 3 == 1 else int(rng.integers(1, 1500)))
    cut, pos = [], 0
    for s in sizes:
        if pos < length:
            cut.append(min(s, length - pos))
            pos += cut[-1]
    return cut


@pytest.mark.parametrize("work", (8000, 48000))
def test_rows_equal_the_lockstep_resampler(dev, work):
    """Seven streams in one rate state, one row each per call while they last: four rate pairs, lengths 2501, 100 and 1, every
    stream cut its own way, the last block final for some and a call of no samples final for the others."""
    from audiodenoiser_amd import StreamResampler, _lib
    from audiodenoiser_amd.resample import resample
    L = _lib.load()
    # the last one: equal rates, a copy.  (No pair that reduces to 1:3 -- test_gpu_stream_resample.py needs that table cold.)
    dsts = {8000: [48000, 44100, 16000], 48000: [8000, 44100, 32000]}[work] + [work]
    streams = [(dsts[0], 2501), (dsts[1], 2501), (dsts[2], 2501), (dsts[3], 2501), (dsts[0], 100), (dsts[1], 1), (dsts[2], 1)]
    n_slots = len(streams) + 2
    max_h = max(ref.history(work, d) for d in dsts)
    need = ctypes.c_size_t()
    assert L.adn_stream_pool_rate_state_bytes(n_slots, max_h, ctypes.byref(need)) == 0
    state = torch.full((need.value // 4,), float("nan"), device=dev)                 # call 0 of a stream reads none of it
    slots = [8, 0, 5, 3, 1, 7, 2]                                                     # not the row order
    xs = [_signal((work, d, i), n) for i, (d, n) in enumerate(streams)]
    cuts = [_cuts((work, d, i), n, ref.history(work, d)) for i, (d, n) in enumerate(streams)]
    for (d, n), c in zip(streams[:3], cuts):
        h = ref.history(work, d)
        assert min(c) < h and max(c) > 2 * h, (d, c, h)
    final_with_last_block = [i % 2 == 0 for i in range(len(streams))]
    pos, calls, got = [0] * len(streams), [0] * len(streams), [[] for _ in streams]
    ended = [False] * len(streams)
    in_stride = max(max(c) for c in cuts) + 3
    out_stride = max(ref.emitted(in_stride, work, d, True) for d in dsts) + 70
    while not all(ended):
        rows, live = [], [i for i in range(len(streams)) if not ended[i]]
        audio = torch.full((len(live), in_stride), float("nan"), device=dev)
        out = torch.full((len(live), out_stride), float("nan"), device=dev)
        counts = []
        for j, i in enumerate(live):
            d, n = streams[i]
            m = cuts[i][calls[i]] if calls[i] < len(cuts[i]) else 0
            final = pos[i] + m == n and (m == 0 or final_with_last_block[i])
            audio[j, :m] = torch.from_numpy(xs[i][pos[i]:pos[i] + m].copy()).to(dev)
            rows.append((slots[i], d, calls[i], pos[i], m, 1 if final else 0, 0))
            counts.append(ref.emitted(pos[i] + m, work, d, final) - ref.emitted(pos[i], work, d))
            pos[i] += m
            calls[i] += 1
            ended[i] = final
        rc = L.adn_stream_pool_emit_rate(state.data_ptr(), need.value, n_slots, max_h, work, _table(rows), len(rows), audio.data_ptr(),
                                         in_stride, out.data_ptr(), out_stride, _st(dev))
        assert rc == 0, L.adn_last_error()
        for j, i in enumerate(live):
            assert torch.isnan(out[j, counts[j]:]).all(), "nothing is written beyond a row's outputs"
            got[i].append(out[j, :counts[j]].clone())
    for i, (d, n) in enumerate(streams):
        g = torch.cat(got[i])
        xd = torch.from_numpy(xs[i].copy()).to(dev)[None]
        whole = resample(xd, work, d)[0]
        assert g.shape == whole.shape and torch.equal(g, whole), (i, d, n)
        rs = StreamResampler(work, d, n_streams=1)
        p, outs = 0, []
        for m in cuts[i]:
            outs.append(rs.push(xd[:, p:p + m]))
            p += m
        outs.append(rs.flush())
        assert torch.equal(g, torch.cat(outs, dim=1)[0]), (i, d, n)
        y_ref, sum_abs, taps = resample_ref.resample_ref(xs[i][None], work, d)
        err = np.abs(g.cpu().numpy().astype(np.float64) - y_ref[0])
        bound = 1.01 * (taps + 2) * EPS * sum_abs[0]
        assert np.all(g.cpu().numpy()[sum_abs[0] == 0] == 0) and np.all(err <= bound), (i, d, n, float(err.max()))
        if d == work:
            assert torch.equal(g, xd[0])


# ---- the ring destination -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
def test_ring_destination(dev, net, plan):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.resample import resample
    L = _lib.load()
    pool = _pool(net, plan, max_streams=4, backlog_steps=1)
    ring, n_slots = pool.book.ring_samples, 4
    sentinel = -7.25
    state = torch.full((pool._state.numel() // 4,), sentinel, device=dev)
    ring_off = state.numel() - n_slots * ring                    # adn.h, "stream pool": the rings are the state's last section
    feeds = {1: 48000, 3: 44100, 2: 8000}                        # slot -> rate (8000: a copy into the ring); slot 0 stays idle
    # three pushes: short of the ring's end, across it (the outputs straddle the wrap), and a final call of no samples
    first = {s: int(0.6 * ring * r / WORK) for s, r in feeds.items()}
    second = {s: int(0.8 * ring * r / WORK) for s, r in feeds.items()}
    xs = {s: _signal((ring, s), first[s] + second[s]) for s in feeds}
    want = {s: resample(torch.from_numpy(xs[s].copy()).to(dev)[None], r, WORK)[0] for s, r in feeds.items()}

    def push(rows, audio):
        rc = L.adn_stream_pool_push_rate(state.data_ptr(), state.numel() * 4, *pool._args, *pool._rate_args[:2], *pool._rate_args[3:],
                                         _table(rows), len(rows), audio.data_ptr() if audio is not None else None, _st(dev))
        assert rc == 0, L.adn_last_error()

    def rings():
        return state[ring_off:].view(n_slots, ring).clone()

    def expect(written):
        e = torch.full((n_slots, ring), sentinel, device=dev)
        for s, m1 in written.items():
            for m0 in range(0, m1, ring):                        # ascending: a later output replaces the one ring_samples before
                seg = want[s][m0:min(m0 + ring, m1)]
                e[s, :seg.shape[0]] = seg
        return e

    order = (3, 1, 2)
    offs = np.cumsum([5] + [first[s] + 3 for s in order])        # the blocks lie anywhere in the one buffer
    audio = torch.full((int(offs[-1]),), float("nan"), device=dev)
    for s, o in zip(order, offs):
        audio[o:o + first[s]] = torch.from_numpy(xs[s][:first[s]].copy()).to(dev)
    push([(s, feeds[s], 0, 0, first[s], 0, int(o)) for s, o in zip(order, offs)], audio)
    m1 = {s: ref.emitted(first[s], feeds[s], WORK) for s in feeds}
    assert all(0 < m < ring for m in m1.values())
    assert torch.equal(rings(), expect(m1))
    offs = np.cumsum([0] + [second[s] for s in order])
    audio = torch.cat([torch.from_numpy(xs[s][first[s]:].copy()) for s in order]).to(dev)
    push([(s, feeds[s], 1, first[s], second[s], 0, int(o)) for s, o in zip(order, offs)], audio)
    m2 = {s: ref.emitted(first[s] + second[s], feeds[s], WORK) for s in feeds}
    assert all(m2[s] > ring and m2[s] - m1[s] <= ring for s in feeds), (m1, m2, ring)
    assert torch.equal(rings(), expect(m2))
    push([(s, feeds[s], 2, first[s] + second[s], 0, 1, 0) for s in (1, 3)], None)
    m3 = {**m2, **{s: ref.emitted(first[s] + second[s], feeds[s], WORK, True) for s in (1, 3)}}
    assert all(m3[s] > m2[s] and m3[s] == want[s].shape[0] for s in (1, 3))
    assert torch.equal(rings(), expect(m3))
    assert (state[:ring_off] == sentinel).all(), "nothing outside the rings is written"


# ---- the pool against the solo stream -----------------------------------------------------------------------------------------
_SOLO = {}


def _solo(model, dtype, plan, rate, x, key):
    """The stream alone: a fresh StreamDenoiser(n_streams=1, input_rate=rate) fed the whole signal and flushed; once per signal,
    left unchanged.  The caller has chosen the model's batch invariance."""
    key = (dtype, plan, rate) + tuple(key)
    if key not in _SOLO:
        from audiodenoiser_amd import StreamDenoiser
        n_fft, hop, w, b, a = plan
        sd = StreamDenoiser(model, n_streams=1, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a,
                            input_rate=rate)
        xd = torch.from_numpy(x.copy()).to(sd.device)[None]
        _SOLO[key] = torch.cat([sd.push(xd), sd.flush()], dim=1)[0].cpu()
        assert _SOLO[key].shape == (len(x),)
    return _SOLO[key]


def _drive(pool, feeds, seed, after=None):
    """Feed `feeds` (a list of (rate, samples), stream i) to the pool in a seeded interleaving of open / push / push_many / close /
    step(): stream i opens at a random tick after stream i - 1, and only once stream after[i] has finished if that is given; blocks
    are of 0, 1, less than a step's or several steps' samples, numpy for even i and device tensors for odd i.
    -> per stream the concatenated samples (cpu tensor), its slot, the tick it opened at; how often push_many carried several."""
    book, dev = pool.book, pool.device
    rng = np.random.default_rng(seed)
    n = len(feeds)
    after = after or {}
    state = ["waiting"] * n                     # waiting -> open -> closed -> finished
    pos, slot, opened_at = [0] * n, [None] * n, [None] * n
    outs = [[] for _ in range(n)]
    by_slot, tick, many = {}, 0, 0

    def take(result):
        for sid, samples, finished in result:
            i = by_slot[sid]
            assert isinstance(samples, np.ndarray) == (i % 2 == 0), "samples come back in the kind of the stream's pushes"
            outs[i].append(torch.from_numpy(samples) if isinstance(samples, np.ndarray) else samples.cpu())
            if finished:
                assert state[i] == "closed"
                state[i] = "finished"
                del by_slot[sid]

    def block_of(i):
        rate, x = feeds[i]
        per = book.block_frames * book.hop_length * rate // WORK
        m = (0, 1, int(rng.integers(1, per + 1)), int(rng.integers(2 * per, 3 * per + 1)))[int(rng.integers(0, 4))]
        return min(m, len(x) - pos[i])

    for _ in range(100000):
        if all(s == "finished" for s in state):
            break
        for i in range(n):
            if (state[i] == "waiting" and all(s != "waiting" for s in state[:i]) and (i not in after or state[after[i]] == "finished")
                    and rng.integers(0, 2)):
                slot[i], opened_at[i], state[i] = pool.open(input_rate=feeds[i][0]), tick, "open"
                by_slot[slot[i]] = i
        live = [i for i in range(n) if state[i] == "open"]
        if not live or rng.integers(0, 3) == 0:
            take(pool.step())
            tick += 1
            continue
        chosen = [i for i in live if rng.integers(0, 2)] or [live[int(rng.integers(0, len(live)))]]
        done = [i for i in chosen if pos[i] == len(feeds[i][1])]
        if done and rng.integers(0, 2):
            i = done[0]
            state[i] = "closed"
            if pool.close(slot[i]):
                assert len(feeds[i][1]) == 0
                state[i] = "finished"
                del by_slot[slot[i]]
            continue
        sizes = {i: block_of(i) for i in chosen}
        if any(m > pool.room(slot[i]) for i, m in sizes.items()):
            take(pool.step())
            tick += 1
            sizes = {i: min(m, pool.room(slot[i])) for i, m in sizes.items()}
        blocks = {}
        for i, m in sizes.items():
            b = feeds[i][1][pos[i]:pos[i] + m]
            blocks[slot[i]] = b if i % 2 == 0 else torch.from_numpy(b.copy()).to(dev)
        if len(blocks) == 1 and rng.integers(0, 2):
            (sid, b), = blocks.items()
            pool.push(sid, b)
        else:
            pool.push_many(blocks)
            many += len(blocks) > 1
        for i, m in sizes.items():
            pos[i] += m
            assert pool.received(slot[i]) == pos[i]
    else:
        raise AssertionError("the drive did not end")
    got = [torch.cat(o) if o else torch.empty(0) for o in outs]
    return got, slot, opened_at, many


def _feeds(plan):
    """Streams at the four rates, a few steps long; the third ends early (before the first step at its rate can run) and the last
    one, at another rate, takes over its slot."""
    n_fft, hop, w, b, a = plan
    per, e0 = b * hop, (b + a - 1) * hop + n_fft // 2
    lengths = ((48000, 6 * (e0 + 3 * per) + 77), (44100, 44100 * (e0 + 2 * per) // 8000 + 5), (16000, e0), (8000, e0 + 2 * per + 9),
               (44100, 44100 * (e0 + per) // 8000 + 1), (16000, 0))
    assert all(n < 60000 for _, n in lengths)
    return [(rate, _signal(plan + (rate, i), n)) for i, (rate, n) in enumerate(lengths)]


@pytest.mark.parametrize("plan", PLANS)
def test_equals_the_solo_stream(dev, net, plan):
    feeds = _feeds(plan)
    net.set_batch_invariant(True)
    try:
        pool = _pool(net, plan, max_streams=5)
        got, slot, opened_at, many = _drive(pool, feeds, list(plan) + [2], after={4: 2})
        assert slot[4] == slot[2] and feeds[4][0] != feeds[2][0], "a stream at another rate reuses the slot (no reset in between)"
        assert len(set(opened_at)) > 1 and many >= 2, (opened_at, many)
        for i, (rate, x) in enumerate(feeds):
            want = _solo(net, "f32", plan, rate, x, (len(x), i))
            assert got[i].shape == want.shape == (len(x),), (i, rate, got[i].shape)
            assert torch.equal(got[i], want), (i, rate, float((got[i] - want).abs().max()))
            assert torch.isfinite(got[i]).all()
        assert pool.step() == [] and pool.book.status == [pool.book.FREE] * 5
    finally:
        net.set_batch_invariant(False)


@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_without_batch_invariance_and_fp16(dev, net, net16, dtype):
    plan = PLANS[1]
    feeds = _feeds(plan)[:4]
    net.set_batch_invariant(False)
    pool = _pool(net if dtype == "f32" else net16, plan, max_streams=4)
    got, _, _, _ = _drive(pool, feeds, list(plan) + [5])
    tol = 2e-5 if dtype == "f32" else 1e-2
    for i, (rate, x) in enumerate(feeds):
        want = _solo(net, "f32-free", plan, rate, x, (len(x), i))                    # fp32, the default kernel choice
        assert got[i].shape == want.shape == (len(x),)
        e = float((got[i] - want).abs().max() / want.abs().max())
        print(f"pool at {rate} Hz {dtype}: {e:.3g} of the solo stream's maximum (allowed {tol:g})")
        assert e <= tol, (i, rate, e)


def test_neighbours_do_not_matter(dev, net):
    plan = PLANS[1]
    n_fft, hop, w, b, a = plan
    per, e0 = b * hop, (b + a - 1) * hop + n_fft // 2
    x = _signal(plan + (44100, 10), 44100 * (e0 + 2 * per) // 8000 + 101)
    others = [(48000, _signal(plan + (11,), 6 * (e0 + per) + 5)), (16000, _signal(plan + (12,), 2 * (e0 + 2 * per))),
              (8000, _signal(plan + (13,), e0 + per + 17))]
    net.set_batch_invariant(True)
    try:
        alone, slot_a, _, _ = _drive(_pool(net, plan, max_streams=2), [(44100, x)], list(plan) + [3])
        among, slot_b, _, _ = _drive(_pool(net, plan, max_streams=8, backlog_steps=2), others + [(44100, x)], list(plan) + [4])
        assert slot_a[0] == 0 and slot_b[3] == 3
        assert alone[0].shape == (len(x),) and torch.equal(alone[0], among[3])
        assert torch.equal(alone[0], _solo(net, "f32", plan, 44100, x, (len(x), 10)))
    finally:
        net.set_batch_invariant(False)


def test_more_rows_than_one_call_holds(dev, net):
    """70 streams at the four rates, pushed by one push_many and all with a step ready in the same tick: the rate entry points are
    called for 64 rows and for the rest -- twice per tick although two working-rate streams sit among the rows.  Every stream
    is compared with its solo stream."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.stream import POOL_RATE_MAX_ROWS
    L = _lib.load()
    counts = {"adn_stream_pool_push_rate": 0, "adn_stream_pool_emit_rate": 0}

    def counted(name, fn):
        def call(*a):
            counts[name] += 1
            return fn(*a)
        return call
    originals = {name: getattr(L, name) for name in counts}
    plan = PLANS[0]
    n_fft, hop, w, b, a = plan
    n = POOL_RATE_MAX_ROWS + 6
    rates = [RATES[i % 3] for i in range(n)]                     # 48, 44.1 and 16 kHz: every stream goes through the rate calls
    rates[5] = rates[66] = 8000                                  # ... but two
    e0 = (b + a - 1) * hop + n_fft // 2
    signals = [_signal(plan + (100 + i,), (e0 + 3 * b * hop + 40 + i) * r // WORK) for i, r in enumerate(rates)]
    net.set_batch_invariant(True)
    try:
        pool = _pool(net, plan, max_streams=n, backlog_steps=8)
        assert [pool.open(input_rate=r) for r in rates] == list(range(n))
        for name in counts:
            setattr(L, name, counted(name, originals[name]))
        pool.push_many({i: signals[i] for i in range(n)})
        assert counts["adn_stream_pool_push_rate"] == 2
        first = pool.step()
        assert [s for s, _, _ in first] == list(range(n)) and not any(f for _, _, f in first)
        assert counts["adn_stream_pool_emit_rate"] == 0, "steps 0 and 1 return nothing at this plan: no call"
        second = pool.step()
        assert counts["adn_stream_pool_emit_rate"] == 0 and all(len(t[1]) == 0 for t in first + second)
        third = pool.step()                                      # 16 samples per stream at the working rate: 68 rows go back
        assert counts["adn_stream_pool_emit_rate"] == 2 and [s for s, _, _ in third] == list(range(n))
        for name in counts:
            setattr(L, name, originals[name])
        mid = pool.drain()
        for i in range(n):
            assert pool.close(i) is False
        rest = pool.drain()
        assert [(s, f) for s, _, f in rest] == [(i, True) for i in range(n)]
        for i in range(n):
            got = torch.from_numpy(np.concatenate([first[i][1], second[i][1], third[i][1], mid[i][1], rest[i][1]]))
            want = _solo(net, "f32", plan, rates[i], signals[i], (len(signals[i]), 100 + i))
            assert got.shape == want.shape and torch.equal(got, want), i
    finally:
        for name in counts:
            setattr(L, name, originals[name])
        net.set_batch_invariant(False)


def test_kinds_refusals_and_a_pool_without_rates(dev, net):
    plan = PLANS[0]
    x = _signal(plan + (30,), 3000)
    net.set_batch_invariant(True)
    try:
        pool = _pool(net, plan, max_streams=2, backlog_steps=64)
        want = _solo(net, "f32", plan, 48000, x, (3000, 30))
        # numpy in -> numpy out, a device tensor in -> a tensor there out, per stream
        a, b = pool.open(input_rate=48000), pool.open(48000)
        pool.push_many({a: x[:1700], b: torch.from_numpy(x[:1700].copy()).to(dev)})
        with pytest.raises(RuntimeError, match=r"call step\(\)"):
            pool.push_many({a: x[1700:1701], b: torch.zeros(pool.room(b) + 1, device=dev)})
        assert pool.received(a) == pool.received(b) == 1700, "a refused push_many changes no stream"
        outs = {a: [], b: []}
        pool.push(a, x[1700:])
        pool.push(b, torch.from_numpy(x[1700:].copy()).to(dev))
        assert pool.close(a) is False and pool.close(b) is False
        for sid, samples, finished in pool.drain():
            assert finished and isinstance(samples, np.ndarray) == (sid == a)
            outs[sid] = samples
        assert np.array_equal(outs[a], want.numpy()) and torch.equal(outs[b].cpu(), want)
        with pytest.raises(ValueError, match="input_rates"):
            pool.open(input_rate=22050)
        with pytest.raises(TypeError):
            pool.push(pool.open(48000), torch.zeros(4, dtype=torch.float64, device=dev))
        # a pool made without input_rates: the working rate only, by name or not, and exactly the parent's object
        from audiodenoiser_amd import StreamDenoiser, StreamPool
        plain = StreamPool(net, n_fft=plan[0], hop_length=plan[1], window_frames=plan[2], block_frames=plan[3], lookahead_frames=plan[4],
                           max_streams=2)
        assert plain._rate_state is None and plain.book.ring_samples == plan[0] - plan[1] + plan[0] // 2 + 4 * plan[1]
        with pytest.raises(ValueError, match="input_rates"):
            plain.open(input_rate=48000)
        c, d = plain.open(), plain.open(input_rate=8000)
        low = x[:140]
        plain.push(c, low)
        plain.push_many({d: low})
        plain.close(c), plain.close(d)
        sd = StreamDenoiser(net, n_streams=1, n_fft=plan[0], hop_length=plan[1], window_frames=plan[2], block_frames=plan[3],
                            lookahead_frames=plan[4])
        solo = np.concatenate([sd.push(low), sd.flush()], axis=1)[0]
        for sid, samples, finished in plain.drain():
            assert finished and np.array_equal(samples, solo)
    finally:
        net.set_batch_invariant(False)


def test_cold_call_inside_a_capture_is_refused(dev, net):
    """adn.h: a cold adn_stream_pool_push_rate / _emit_rate on a capturing stream enqueues nothing and returns ADN_ERR_INVALID, as
    adn_resample_stream does; after adn_resample_prepare the same call is captured and replays."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.resample import prepare_resample, resample
    L = _lib.load()
    # ORDER DEPENDENCY, as in tests/test_gpu_stream_resample.py's capture test: the table of 8000 -> 12000 (2:3 reduced to up 3,
    # down 2) must be cold in this process, so no test that runs before this one may resample at a pair that reduces to 3:2
    rate, n = 12000, 900
    max_h = max(ref.history(rate, WORK), ref.history(WORK, rate))
    need = ctypes.c_size_t()
    assert L.adn_stream_pool_rate_state_bytes(2, max_h, ctypes.byref(need)) == 0
    state = torch.zeros(need.value // 4, device=dev)
    x = torch.from_numpy(_signal((rate,), n).copy()).to(dev)
    n_out = ref.emitted(n, WORK, rate)
    out = torch.full((n_out + 8,), -3.0, device=dev)
    rows = _table([(1, rate, 0, 0, n, 0, 0)])

    def call(stream):
        return L.adn_stream_pool_emit_rate(state.data_ptr(), need.value, 2, max_h, WORK, rows, 1, x.data_ptr(), n, out.data_ptr(),
                                           out.numel(), stream)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            rc_cold = call(side.cuda_stream)
            msg = L.adn_last_error()
        finally:
            graph.capture_end()
    assert rc_cold == ADN_ERR_INVALID and b"adn_resample_prepare" in msg and b"adn_stream_pool_emit_rate" in msg
    torch.cuda.synchronize(dev)
    assert (out == -3.0).all() and (state == 0).all()
    prepare_resample(WORK, rate, dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            rc = call(side.cuda_stream)
        finally:
            graph.capture_end()
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out[:n_out], resample(x[None], WORK, rate)[0, :n_out]) and (out[n_out:] == -3.0).all()
