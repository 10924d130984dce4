"""StreamPool on the device (audiodenoiser_amd/stream.py, csrc/stream_kernels.hip, include/adn.h "stream pool"): independent streams
whose ready steps are batched, against the solo stream (a fresh StreamDenoiser(n_streams=1) fed the whole signal and flushed) and
against the float64 restatement in tests/stream_ref.py.

Bounds (none derived here):
* "bit for bit": torch.equal with model.set_batch_invariant(True) -- the pool is DEFINED as independent instances of the stream.
* float64 restatement: the inputs, the network wrapper and the bounds of tests/test_gpu_stream.py::test_end_to_end -- TOL = 1e-4 of
  max |ref| in fp32 with the same device network as the restatement's callable, 1e-2 in fp16 against the fp32 device network.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
PLANS = ((512, 128, 64, 16, 0), (512, 128, 48, 8, 4), (256, 64, 32, 16, 16), (64, 16, 16, 1, 0))     # n_fft, hop, W, B, A
N_STREAMS = 3
ADN_ERR_INVALID, ADN_ERR_WORKSPACE = 1, 3


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
    return StreamPool(model, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a, **kw)


def _end_of(plan, k):
    n_fft, hop, w, b, a = plan
    return (k * b + b + a - 1) * hop + n_fft // 2


def _signal(plan, length, tag):
    """Uniform [-1, 1] audio seeded from the parameters."""
    x = np.random.default_rng(list(plan) + [length, tag]).uniform(-1.0, 1.0, length).astype(np.float32)
    x.setflags(write=False)
    return x


_SOLO = {}


def _solo(model, dtype, plan, x, key):
    """The stream alone: a fresh StreamDenoiser(n_streams=1) fed the whole signal and flushed; computed once per signal and left
    unchanged.  The caller has set the model batch invariant."""
    key = (dtype,) + plan + key
    if key not in _SOLO:
        from audiodenoiser_amd import StreamDenoiser
        n_fft, hop, w, b, a = plan
        sd = StreamDenoiser(model, n_streams=1, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a)
        xd = torch.from_numpy(x.copy()).to(sd.device)[None]
        _SOLO[key] = torch.cat([sd.push(xd), sd.flush()], dim=1)[0].cpu()
        assert _SOLO[key].shape == (len(x),)
    return _SOLO[key]


def _drive(pool, signals, seed, after=None, first_push=None):
    """Feed `signals` (a list of arrays, stream i) to the pool in a seeded interleaving of open / push / close / step(): stream i
    opens at a random tick after stream i - 1, and only once stream after[i] has finished if that is given; its pushes are of 0, 1, less than a step
    or several steps' samples (first_push[i]: the size of its first one), numpy for even i and device tensors for odd i.
    -> per stream the concatenated samples (cpu tensor), its slot, the tick it opened at; the kinds of pushes that happened."""
    book, dev = pool.book, pool.device
    per = book.block_frames * book.hop_length
    rng = np.random.default_rng(seed)
    n = len(signals)
    after = after or {}
    first_push = dict(first_push or {})
    state = ["waiting"] * n                     # waiting -> open -> closed -> finished
    pos, slot, opened_at = [0] * n, [None] * n, [None] * n
    outs = [[] for _ in range(n)]
    by_slot, kinds, tick = {}, set(), 0

    def take(result):
        for sid, samples, finished in result:
            i = by_slot[sid]
            assert isinstance(samples, np.ndarray) == (i % 2 == 0), "samples come back in the kind of the stream's pushes"
            outs[i].append(torch.from_numpy(samples) if isinstance(samples, np.ndarray) else samples.cpu())
            if finished:
                assert state[i] == "closed"
                state[i] = "finished"
                del by_slot[sid]

    for _ in range(100000):
        if all(s == "finished" for s in state):
            break
        for i in range(n):
            if (state[i] == "waiting" and all(s != "waiting" for s in state[:i]) and (i not in after or state[after[i]] == "finished")
                    and rng.integers(0, 2)):
                slot[i], opened_at[i], state[i] = pool.open(), tick, "open"
                by_slot[slot[i]] = i
        live = [i for i in range(n) if state[i] == "open"]
        if not live or rng.integers(0, 3) == 0:
            take(pool.step())
            tick += 1
            continue
        i = live[int(rng.integers(0, len(live)))]
        left = len(signals[i]) - pos[i]
        if left == 0 and rng.integers(0, 2):
            state[i] = "closed"
            if pool.close(slot[i]):
                assert len(signals[i]) == 0
                state[i] = "finished"
                del by_slot[slot[i]]
            continue
        kind = int(rng.integers(0, 4))
        m = first_push.pop(i, (0, 1, int(rng.integers(1, per + 1)), int(rng.integers(2 * per, 3 * per + 1)))[kind])
        m = min(m, left)
        assert pool.room(slot[i]) >= 0
        if m > pool.room(slot[i]):
            take(pool.step())
            tick += 1
            m = min(m, pool.room(slot[i]))
        kinds.add("none" if m == 0 else "one" if m == 1 else "sub-step" if m < per else "multi-step" if m >= 2 * per else "step")
        block = signals[i][pos[i]:pos[i] + m]
        pool.push(slot[i], block if i % 2 == 0 else torch.from_numpy(block.copy()).to(dev))
        pos[i] += m
        assert pool.received(slot[i]) == pos[i]
    else:
        raise AssertionError("the drive did not end")
    got = [torch.cat(o) if o else torch.empty(0) for o in outs]
    return got, slot, opened_at, kinds


@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("plan", PLANS)
def test_equals_the_solo_stream(dev, net, net16, plan, dtype):
    n_fft, hop, w, b, a = plan
    model = net if dtype == "f32" else net16
    per = b * hop
    # a stream that ends exactly where a step becomes ready; several steps and an odd remainder; (in the first one's slot) one
    # sample more than a step's end; less than half a frame; nothing at all
    lengths = [_end_of(plan, 2), 5 * per + 77, _end_of(plan, 1) + 1, n_fft // 2 - 3, 0]
    signals = [_signal(plan, length, i) for i, length in enumerate(lengths)]
    model.set_batch_invariant(True)
    try:
        pool = _pool(model, plan, max_streams=4)
        got, slot, opened_at, kinds = _drive(pool, signals, list(plan) + [1], after={2: 0}, first_push={1: 2 * per + 3})
        assert slot[2] == slot[0], "the third stream reuses the first one's slot (no reset in between)"
        assert len(set(opened_at)) > 1, opened_at
        assert {"none", "one", "sub-step", "multi-step"} <= kinds, kinds
        for i, x in enumerate(signals):
            want = _solo(model, dtype, plan, x, (len(x), i))
            assert got[i].shape == want.shape == (len(x),), (i, got[i].shape)
            assert torch.equal(got[i], want), (i, float((got[i] - want).abs().max()))
            assert torch.isfinite(got[i]).all()
        assert pool.step() == [] and pool.book.status == [pool.book.FREE] * 4
    finally:
        model.set_batch_invariant(False)


@pytest.mark.parametrize("plan", PLANS[1:3])
def test_neighbours_do_not_matter(dev, net, plan):
    n_fft, hop, w, b, a = plan
    per = b * hop
    x = _signal(plan, 3 * per + 101, 10)
    others_a = [_signal(plan, 2 * per + 5, 11), _signal(plan, 4 * per, 12)]
    others_b = [_signal(plan, per + 901, 13), _signal(plan, 17, 14), _signal(plan, 6 * per + 1, 15)]
    net.set_batch_invariant(True)
    try:
        # pool A: the stream in slot 0 with two neighbours; pool B: three slots taken by streams that wait for more samples, the
        # stream in slot 3, other neighbours, another ring size, another interleaving
        got_a, slot_a, _, _ = _drive(_pool(net, plan, max_streams=8), [x] + others_a, list(plan) + [2])
        pool_b = _pool(net, plan, max_streams=8, backlog_steps=2)
        for i in range(3):
            pool_b.push(pool_b.open(), _signal(plan, 17 + i, 16 + i))
        got_b, slot_b, _, _ = _drive(pool_b, [x] + others_b, list(plan) + [3])
        assert slot_a[0] == 0 and slot_b[0] == 3
        assert torch.equal(got_a[0], got_b[0])
        assert torch.equal(got_a[0], _solo(net, "f32", plan, x, (len(x), 10)))
    finally:
        net.set_batch_invariant(False)


@pytest.mark.parametrize("plan", (PLANS[3], PLANS[1]))
def test_ring_wrap(dev, net, plan):
    n_fft, hop, w, b, a = plan
    net.set_batch_invariant(True)
    try:
        pool = _pool(net, plan, max_streams=2, backlog_steps=1)
        ring = pool.book.ring_samples
        assert ring == n_fft - hop + _end_of(plan, 0) + b * hop             # the smallest ring the library takes
        x = _signal(plan, 8 * ring + 13, 20)
        want = _solo(net, "f32", plan, x, (len(x), 20))
        rng = np.random.default_rng(list(plan) + [4])
        pool.open()                                                          # slot 0 stays idle
        sid = pool.open()
        pos, outs, refused = 0, [], 0
        while pos < len(x):
            room = pool.room(sid)
            assert room >= 0
            if room < len(x) - pos and rng.integers(0, 3) == 0:              # one sample too many: refused, nothing changes
                with pytest.raises(RuntimeError, match=r"call step\(\)"):
                    pool.push(sid, x[pos:pos + room + 1])
                assert pool.received(sid) == pos and pool.room(sid) == room
                refused += 1
            m = min(room if rng.integers(0, 2) else int(rng.integers(0, room + 1)), len(x) - pos)
            pool.push(sid, x[pos:pos + m])
            pos += m
            for s, samples, finished in pool.step():
                assert s == sid and not finished
                outs.append(samples)
        assert refused >= 2 and pos >= 8 * ring
        assert pool.close(sid) is False
        tail = pool.drain()
        assert [(s, f) for s, _, f in tail] == [(sid, True)]
        got = torch.from_numpy(np.concatenate(outs + [tail[0][1]]))
        assert got.shape == want.shape and torch.equal(got, want)
    finally:
        net.set_batch_invariant(False)


def test_more_than_one_group(dev, net):
    """260 streams, all with a step ready in the same tick: the entry points are called for 256 rows and for 4."""
    plan = PLANS[3]
    n, length = 260, _end_of(plan, 0) + 8
    signals = [_signal(plan, length, 100 + i) for i in range(n)]
    net.set_batch_invariant(True)
    try:
        pool = _pool(net, plan, max_streams=n)
        assert [pool.open() for _ in range(n)] == list(range(n))
        for i in range(n):
            pool.push(i, signals[i])
        first = pool.step()
        assert [s for s, _, _ in first] == list(range(n)) and not any(f for _, _, f in first)
        for i in range(n):
            assert pool.close(i) is False
        rest = pool.drain()
        assert [(s, f) for s, _, f in rest] == [(i, True) for i in range(n)]
        for i in (0, 255, 256, 259):
            got = torch.from_numpy(np.concatenate([first[i][1], rest[i][1]]))
            want = _solo(net, "f32", plan, signals[i], (length, 100 + i))
            assert got.shape == want.shape and torch.equal(got, want), i
    finally:
        net.set_batch_invariant(False)


def lengths(hop, block):
    return (10007, 24000, block * hop, hop - 1, 1)


def _audio(plan, length):
    """The audio of tests/test_gpu_stream.py's case (plan, length): uniform [-1, 1], seeded from the parameters."""
    return np.random.default_rng(list(plan) + [length]).uniform(-1.0, 1.0, (N_STREAMS, length)).astype(np.float32)


def _device_net(model, dev):
    """The device network as the restatement's callable: (K, F, W) float64 -> (K, F, W) float64, 64 windows at a time."""
    def call(win):
        x = torch.from_numpy(win.astype(np.float32)).to(dev)[:, None]
        with torch.no_grad():
            y = torch.cat([model(x[i:i + 64]) for i in range(0, x.shape[0], 64)])
        return y[:, 0].cpu().numpy().astype(np.float64)
    return call


_WANT = {}


def _restated(net, dev, plan):
    """The float64 restatement of every stream of a plan's cases, with the fp32 device network: once per plan, left unchanged."""
    if plan not in _WANT:
        call = _device_net(net, dev)
        _WANT[plan] = [(x, ref.denoise(x.astype(np.float64), call, *plan))
                       for length in lengths(plan[1], plan[3]) for x in _audio(plan, length)]
    return _WANT[plan]


@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("plan", PLANS)
def test_against_the_restatement(dev, net, net16, plan, dtype):
    """The default kernel choice (not batch invariant).  All streams of the plan's cases share one pool; each is pushed whole or
    as far as its ring has room, closed, and the pool is drained tick by tick."""
    cases = _restated(net, dev, plan)
    pool = _pool(net if dtype == "f32" else net16, plan, max_streams=len(cases))
    pos, got = [0] * len(cases), [[] for _ in cases]
    sids = [pool.open() for _ in cases]
    open_ = set(sids)
    while open_:
        for sid in sorted(open_):
            if pool.book.status[sid] != pool.book.RUNNING:
                continue
            x = cases[sid][0]
            m = min(pool.room(sid), len(x) - pos[sid])
            pool.push(sid, x[pos[sid]:pos[sid] + m])
            pos[sid] += m
            if pos[sid] == len(x):
                assert pool.close(sid) is False
        for sid, samples, finished in pool.step():
            got[sid].append(samples)
            if finished:
                open_.discard(sid)
    tol = TOL if dtype == "f32" else 1e-2
    worst = 0.0
    for (x, want), g in zip(cases, got):
        g = np.concatenate(g).astype(np.float64)
        assert g.shape == want.shape == x.shape and np.isfinite(g).all()
        e = float(np.abs(g - want).max() / np.abs(want).max())
        worst = max(worst, e)
        assert e <= tol, (len(x), e)
    print(f"pool against the restatement {dtype} plan {plan}: {len(cases)} streams, {worst:.3g} of the maximum (allowed {tol:g})")


def test_c_abi_refusals_on_the_device(dev, net):
    """Each refused call returns its documented code, launches nothing (state, windows and audio keep their bytes) and leaves the
    following valid call correct (equal to the same call on a state that saw no refusal)."""
    from audiodenoiser_amd import _lib
    L = _lib.load()
    plan = PLANS[1]
    n_fft, hop, w, b, a = plan
    pool = _pool(net, plan, max_streams=4, backlog_steps=1)
    args, f = pool._args, n_fft // 2 + 1
    stride = b * hop + n_fft // 2
    length = _end_of(plan, 0) + 40                                   # T = 1 + length // hop frames, K steps
    k_last = -(-(1 + length // hop) // b)
    x = torch.from_numpy(_signal(plan, length, 30).copy()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def rows(*r):
        return (_lib.StreamPoolRow * len(r))(*[_lib.StreamPoolRow(*v) for v in r])

    def fresh():
        state = torch.zeros_like(pool._state)
        assert L.adn_stream_pool_reset(state.data_ptr(), state.numel(), *args, -1, st) == 0
        for slot in (0, 2):
            assert L.adn_stream_pool_write(state.data_ptr(), state.numel(), *args, slot, x.data_ptr(), length, 0, st) == 0
        return state

    def valid(state):
        """Step 0 of slots 2 and 0 (in that row order), the windows in the network's place."""
        r = rows((2, 0, -1), (0, 0, length))
        win = torch.full((2, 1, f, w), float("nan"), device=dev)
        out = torch.full((2, stride), float("nan"), device=dev)
        assert L.adn_stream_pool_analyze(state.data_ptr(), state.numel(), *args, r, 2, win.data_ptr(), st) == 0, L.adn_last_error()
        assert L.adn_stream_pool_emit(state.data_ptr(), state.numel(), *args, r, 2, win.data_ptr(), out.data_ptr(), stride, st) == 0
        return win, out

    want_win, want_out = valid(fresh())
    n0 = pool.book.count(0, -1)
    assert torch.isfinite(want_win).all() and torch.isfinite(want_out[:, :n0]).all()
    assert torch.equal(want_win[0], want_win[1]) and torch.equal(want_out[0, :n0], want_out[1, :n0])     # the same audio in both slots

    state = fresh()
    before = state.clone()
    win = torch.full((257, 1, f, w), float("nan"), device=dev)
    out = torch.full((257, stride), float("nan"), device=dev)
    many = rows(*[(i % 4, 0, -1) for i in range(257)])
    refusals = (
        ("a short state", ADN_ERR_WORKSPACE, state.numel() - 1, rows((0, 0, -1)), 1),
        ("a row past K - 1 of a closed stream", ADN_ERR_INVALID, state.numel(), rows((2, 0, -1), (0, k_last, length)), 2),
        ("a duplicate slot", ADN_ERR_INVALID, state.numel(), rows((2, 0, -1), (0, 0, -1), (2, 1, -1)), 3),
        ("n_rows = 257", ADN_ERR_INVALID, state.numel(), many, 257),
        ("slot = n_slots", ADN_ERR_INVALID, state.numel(), rows((0, 0, -1), (4, 0, -1)), 2),
    )
    for why, code, nbytes, r, n in refusals:
        assert L.adn_stream_pool_analyze(state.data_ptr(), nbytes, *args, r, n, win.data_ptr(), st) == code, why
        assert b"adn_stream_pool_analyze" in L.adn_last_error(), why
        assert L.adn_stream_pool_emit(state.data_ptr(), nbytes, *args, r, n, win.data_ptr(), out.data_ptr(), stride, st) == code, why
        assert b"adn_stream_pool_emit" in L.adn_last_error(), why
    torch.cuda.synchronize(dev)
    assert torch.equal(state, before) and torch.isnan(win).all() and torch.isnan(out).all()
    got_win, got_out = valid(state)
    assert torch.equal(got_win, want_win) and torch.equal(got_out[:, :n0], want_out[:, :n0])
