"""The pool form of the echo canceller on the device: adn_aec_stream_pool (include/adn_call.h, libadn_call.so) and EchoStreamPool.

There is no new arithmetic -- every (microphone, bin) row is the "echo stream" recursion of include/adn_echo.h from the same step
function -- so every comparison but the last is exact bit equality against code that tests/test_gpu_echo.py bounds against float64:
1. Pool call against lockstep call: a pool state of 5 calls and a lockstep state (max_steps = 1: the same ring geometry) of 3 mics
   pairs hold the same cells, the pool's calls named in scrambled order, the lockstep far ends the calls' far ends repeated; the pool
   call must leave the microphone ring cells, window columns and state records the lockstep call leaves, and no other byte.
2. Three calls at different steps in one launch against each alone.
3. Pool against solo objects: the scenario of test_gpu_stream_pool_mc.py (staggered opens, uneven pushes of numpy arrays and device
   tensors, a call closed mid-way, a call's slots reused without a reset, one call at 48 kHz).
4. A tick of more than 256 stream rows, cut into two library calls.
5. The overlap-add section of a far-end slot never changes.
6. One call against the float64 chain of tests/echo_ref.py: within 4 floors, the bound and the floor of
   test_gpu_echo.py::test_stream_against_the_float64_end_to_end_form.

n_fft 64, hop 16, window 16, block 4, ring 1024 (check 6 also at n_fft 512): F = 33 is two tiles at G = 8, the second with one
live bin, and five tiles at G = 32; a step is 64 samples.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import echo_cases as ec  # noqa: E402
import echo_ref as er  # noqa: E402
import footprint as fp  # noqa: E402
import solver_bounds as sb  # noqa: E402
from test_gpu_stream_pool_mc import _LENGTHS, _RATES, _scenario  # noqa: E402  (the scenario itself, not a copy of it)

pytestmark = pytest.mark.gpu

N_FFT, HOP, WINDOW, BLOCK = 64, 16, 16, 4
F = N_FFT // 2 + 1
PLAN = (N_FFT, HOP, WINDOW, BLOCK, 0)
KW = dict(n_fft=N_FFT, hop_length=HOP, block_frames=BLOCK)
RING = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _lib():
    from audiodenoiser_amd import _lib as lib
    return lib


def _stream(dev):
    from audiodenoiser_amd._host import current_stream
    return current_stream(dev)


def _size(fn, *args):
    need = ctypes.c_size_t(0)
    assert fn(*args, ctypes.byref(need)) == 0, fn.__name__
    return need.value


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rows(rows):
    lib = _lib()
    return (lib.StreamPoolRow * len(rows))(*[lib.StreamPoolRow(*r) for r in rows])


def _ring(state, n):
    """The X ring of a pool or lockstep (max_steps = 1) state of n slots: [slot][B][F] float2, the first section."""
    return state.view(torch.float32)[:n * BLOCK * F * 2].view(n, BLOCK, F, 2)


def _struct(kw):
    from audiodenoiser_amd.echo import AecParams
    return AecParams(**kw).to_struct() if kw else None


def _ref(s):
    return ctypes.byref(s) if s is not None else None


def _pool_call(dev, pstate, n_slots, mics, rows, y, p, astate):
    lib = _lib()
    lib.check_call(lib.load_call().adn_aec_stream_pool(pstate.data_ptr(), pstate.numel(), n_slots, mics, *PLAN, RING, _rows(rows), len(rows),
                                                       y.data_ptr(), _ref(p), astate.data_ptr(), astate.numel(), _stream(dev)),
                   "adn_aec_stream_pool")


# ---- 1. pool call against lockstep call ------------------------------------------------------------------------------------------------
CALLS, NAMED = 5, (4, 1, 2)                             # the pool's calls; the ones a call names, scrambled; 0 and 3 are not
STEPS = ((0, -1), (1, -1), (2, 165))                    # fresh; carried; the last step of 11 frames: three frames
# (step index, order in NAMED) whose far end is all zero: in the fresh step every tap of every frame is zero, so the gate holds for
# every parameter set; in the carried one it holds where the taps reach no further back than the step (K1)
SILENT = ((0, 1), (1, 2))


@pytest.mark.parametrize("kw", ec.PARITY_PARAMS, ids=ec.PARAM_IDS)
@pytest.mark.parametrize("mics", (1, 2, 4, 7), ids=lambda m: f"M{m}")
def test_pool_call_leaves_what_the_lockstep_call_leaves(dev, mics, kw):
    lib = _lib()
    L, E = lib.load(), lib.load_echo()
    M, C = mics, mics + 1
    p = _struct(kw)
    n_slots, pairs = CALLS * C, len(NAMED) * M
    pool_need = _size(E.adn_aec_stream_state_bytes, CALLS * M, F, _ref(p))
    lock_need = _size(E.adn_aec_stream_state_bytes, pairs, F, _ref(p))
    per = pool_need // (CALLS * M)
    assert per * CALLS * M == pool_need and per * pairs == lock_need
    gen = torch.Generator(device="cpu").manual_seed(300 + M)
    with torch.cuda.device(dev):
        pstate = torch.randn(_size(L.adn_stream_pool_state_bytes, n_slots, *PLAN, RING) // 4, generator=gen).to(dev).view(torch.uint8)
        sstate = torch.randn(_size(L.adn_stream_state_bytes, 2 * pairs, *PLAN, 1) // 4, generator=gen).to(dev).view(torch.uint8)
        p_astate, h_astate = fp.carve(pool_need, 0xFF, dev)
        l_astate = torch.full((lock_need,), 0xFF, dtype=torch.uint8, device=dev)
        mic_slots = [r * C + m for r in NAMED for m in range(M)]
        far_slots = [r * C + M for r in NAMED]
        mic_rows = [i * C + m for i in range(len(NAMED)) for m in range(M)]      # the microphones' rows of the pool's table
        far_rows = [i * C + M for i in range(len(NAMED))]
        records = [r * M + m for r in NAMED for m in range(M)]                   # pair (call, m) of the pool = pair order M + m
        gated = 0
        for si, (step, final) in enumerate(STEPS):
            mic_cells = torch.randn((pairs, BLOCK, F, 2), generator=gen).to(dev)
            far_cells = torch.randn((len(NAMED), BLOCK, F, 2), generator=gen).to(dev)
            for s, order in SILENT:
                if s == si:
                    far_cells[order] = 0.0
            _ring(pstate, n_slots)[mic_slots] = mic_cells
            _ring(pstate, n_slots)[far_slots] = far_cells
            _ring(sstate, 2 * pairs)[0::2] = mic_cells
            _ring(sstate, 2 * pairs)[1::2] = far_cells.repeat_interleave(M, dim=0)
            y = torch.rand((len(NAMED) * C, 1, F, WINDOW), generator=gen).to(dev)
            y_lock = torch.empty((2 * pairs, 1, F, WINDOW), device=dev)
            y_lock[0::2], y_lock[1::2] = y[mic_rows], y[far_rows].repeat_interleave(M, dim=0)
            y_pool, h_y = fp.carve_copy(y, dev)
            before, a_before = pstate.clone(), p_astate.clone()
            lib.check_echo(E.adn_aec_stream(sstate.data_ptr(), sstate.numel(), y_lock.data_ptr(), 2 * pairs, step, 1, final, *PLAN, 1,
                                            _ref(p), l_astate.data_ptr(), l_astate.numel(), _stream(dev)), "adn_aec_stream")
            rows = [(r * C + ch, step, final) for r in NAMED for ch in range(C)]
            _pool_call(dev, pstate, n_slots, M, rows, y_pool, p, p_astate)
            torch.cuda.synchronize(dev)
            what = (M, kw, step)
            # the microphones' ring cells and window columns of the lockstep call, bit for bit, and something was written
            assert _same(_ring(pstate, n_slots)[mic_slots], _ring(sstate, 2 * pairs)[0::2]), what
            assert _same(y_pool[mic_rows], y_lock[0::2]) and not _same(y_pool[mic_rows], y[mic_rows]), what
            # the state records: pair (NAMED[i], m) of the pool is pair i M + m of the lockstep state
            po, lo = p_astate.view(CALLS * M, per), l_astate.view(pairs, per)
            assert torch.equal(po[records], lo) and not torch.equal(po[records], a_before.view(CALLS * M, per)[records]), what
            # and not one byte else: the far-end slots' cells and window rows, the unnamed slots, the rest of the pool state, the
            # unnamed records, the guards
            want = before.clone()
            _ring(want, n_slots)[mic_slots] = _ring(sstate, 2 * pairs)[0::2]
            assert torch.equal(pstate, want), what
            assert _same(_ring(pstate, n_slots)[far_slots], far_cells), what
            y_want = y.clone()
            y_want[mic_rows] = y_lock[0::2]
            assert _same(y_pool, y_want) and _same(y_pool[far_rows], y[far_rows]), what
            others = [r * M + m for r in range(CALLS) if r not in NAMED for m in range(M)]
            assert bool((po[others] == 0xFF).all()), what
            fp.assert_guards_intact(h_astate, "echo state of the pool")
            fp.assert_guards_intact(h_y, "windows of the pool")
            # the gate ran.  Fresh step, silent far end: every tap of every frame is zero, so P is still (1 / loading) I, bit for bit
            # (ungated it is that over forget^4); carried step at K1: the tap is the silent step's own frame, P and h stay as they were
            K, D = (kw or {}).get("taps", 8), (kw or {}).get("delay", 0)
            floats = p_astate.view(torch.float32).view(CALLS * M, F, per // F // 4)
            for s, order in SILENT:
                silent = [NAMED[order] * M + m for m in range(M)]
                if s == si == 0:
                    p0 = np.float32(1.0) / np.float32((kw or {}).get("loading", 10.0))
                    assert bool((floats[silent][..., 0] == float(p0)).all()) and not floats[silent][..., 2 * K * K:2 * K * K + 2 * K].any(), what
                    if D < BLOCK:                                                # a loud far end reaches the taps within the step: P moved
                        loud = [NAMED[0] * M + m for m in range(M)]
                        assert not bool((floats[loud][..., 0] == float(p0)).any()), what
                    gated += 1
                elif s == si == 1 and K == 1 and D == 0:
                    was = a_before.view(torch.float32).view(CALLS * M, F, per // F // 4)
                    assert _same(floats[silent][..., :2 * K * K + 2 * K], was[silent][..., :2 * K * K + 2 * K]), what
                    gated += 1
        assert gated == (2 if (kw or {}).get("taps", 8) == 1 else 1)


# ---- 2. different steps in one launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", ec.PARITY_PARAMS, ids=ec.PARAM_IDS)
def test_calls_at_different_steps_in_one_launch_equal_each_alone(dev, kw):
    lib = _lib()
    L, E = lib.load(), lib.load_echo()
    M, C, n_calls = 2, 3, 3
    p = _struct(kw)
    steps = ((0, -1), (5, -1), (2, 165))                 # fresh; carried; a last step of three frames
    n_slots = n_calls * C
    need = _size(E.adn_aec_stream_state_bytes, n_calls * M, F, _ref(p))
    per = need // (n_calls * M)
    gen = torch.Generator(device="cpu").manual_seed(17)
    with torch.cuda.device(dev):
        pstate = torch.randn(_size(L.adn_stream_pool_state_bytes, n_slots, *PLAN, RING) // 4, generator=gen).to(dev).view(torch.uint8)
        # a carried pair reads its record: small finite values, so that nothing overflows on the way (any bits would do for equality)
        astate = (0.1 * torch.randn(need // 4, generator=gen)).to(dev).view(torch.uint8)
        y = torch.rand((n_calls * C, 1, F, WINDOW), generator=gen).to(dev)
        rows = [(i * C + ch, step, final) for i, (step, final) in enumerate(steps) for ch in range(C)]
        joint = [pstate.clone(), astate.clone(), y.clone()]
        _pool_call(dev, joint[0], n_slots, M, rows, joint[2], p, joint[1])
        for i in range(n_calls):
            alone = [pstate.clone(), astate.clone(), y[i * C:(i + 1) * C].clone()]
            _pool_call(dev, alone[0], n_slots, M, rows[i * C:(i + 1) * C], alone[2], p, alone[1])
            torch.cuda.synchronize(dev)
            slots = list(range(i * C, (i + 1) * C))
            assert _same(_ring(joint[0], n_slots)[slots], _ring(alone[0], n_slots)[slots]), (kw, i)
            assert _same(joint[2][i * C:(i + 1) * C], alone[2]) and not _same(alone[2], y[i * C:(i + 1) * C]), (kw, i)
            records = slice(i * M, (i + 1) * M)
            assert torch.equal(joint[1].view(n_calls * M, per)[records], alone[1].view(n_calls * M, per)[records]), (kw, i)
            assert not torch.equal(alone[1].view(n_calls * M, per)[records], astate.view(n_calls * M, per)[records]), (kw, i)
            # the call alone left the other calls' slots, rows and records as they were
            rest = [s for s in range(n_slots) if s not in slots]
            assert _same(_ring(alone[0], n_slots)[rest], _ring(pstate, n_slots)[rest])
            keep = [r for r in range(n_calls * M) if not i * M <= r < (i + 1) * M]
            assert torch.equal(alone[1].view(n_calls * M, per)[keep], astate.view(n_calls * M, per)[keep])


# ---- 3. pool against solo objects --------------------------------------------------------------------------------------------------------
def _call_audio(group, start, length, mics):
    """One call: `mics` microphones that hear the far end of parity group `group` (each its own mix of the group's microphone and a
    delayed far end), then that far end -> (mics + 1, length) float32."""
    mic, far, _ = ec.parity_audio(N_FFT, 1000)
    rows = [(1.0 - 0.1 * m) * mic[group] + 0.1 * m * np.roll(far[group], 3 * m + 1) for m in range(mics)] + [far[group]]
    return np.ascontiguousarray(np.stack(rows)[:, start:start + length].astype(np.float32))


def _solo(dev, x, m, params, gain, rate, kw=KW):
    """What a solo lockstep pair returns for microphone `m` and the far end of the call `x` (mics + 1, L)."""
    from audiodenoiser_amd.echo import StreamEchoCanceller
    se = StreamEchoCanceller(dev, pairs=1, params=params, gain=gain, input_rate=rate, **kw)
    pair = torch.from_numpy(np.ascontiguousarray(x[[m, x.shape[0] - 1]])).to(dev)
    return torch.cat([se.push(pair), se.flush()], dim=-1).cpu()


@pytest.mark.parametrize("mics,gain,kw", ((1, False, None), (1, True, ec.PARITY_PARAMS[3]), (3, False, ec.PARITY_PARAMS[2]), (3, True, None)),
                         ids=("M1", "M1-gain-K16", "M3-K9-D2", "M3-gain"))
def test_every_microphone_of_every_call_equals_its_solo_pair(dev, mics, gain, kw):
    from audiodenoiser_amd.echo import AecParams, EchoStreamPool
    params = AecParams(**kw) if kw else None
    starts = ((0, 100), (1, 0), (2, 40), (0, 5000))
    sig = [_call_audio(g, at, n, mics) for (g, at), n in zip(starts, _LENGTHS)]
    pool = EchoStreamPool(dev, 3, mics, backlog_steps=64, params=params, gain=gain, input_rates=(48000,), **KW)
    assert pool.latency_samples == (BLOCK - 1) * HOP + N_FFT and pool.channels == mics + 1 and pool.max_streams == 3
    got = _scenario(pool, dev, sig, _RATES)
    for i, x in enumerate(sig):
        out = got[i][None] if mics == 1 else got[i]
        assert got[i].shape == ((_LENGTHS[i],) if mics == 1 else (mics, _LENGTHS[i])), (i, got[i].shape)      # as many samples as came in
        for m in range(mics):
            want = _solo(dev, x, m, params, gain, _RATES[i])
            assert want.shape == (_LENGTHS[i],) and torch.equal(out[m], want), (i, m, float((out[m] - want).abs().max()))
    with pytest.raises(RuntimeError):
        pool.network(None)
    with pytest.raises(ValueError):
        pool.push(pool.open(), np.zeros(10, np.float32))                                           # (mics + 1, m), not (m,)


# ---- 4. a tick cut into several library calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mics,n_calls", ((1, 129), (7, 33)), ids=("M1-129", "M7-33"))
def test_a_tick_of_more_than_256_rows(dev, mics, n_calls):
    from audiodenoiser_amd.echo import EchoStreamPool
    lengths = (330, 250)
    pool = EchoStreamPool(dev, n_calls, mics, **KW)
    assert len(pool.book.calls([(r, 0, -1) for r in range(n_calls)])) == 2 and n_calls * (mics + 1) > 256
    audio = {(g, n): _call_audio(g, 0, n, mics) for g in range(3) for n in lengths}
    which = {}
    for i in range(n_calls):
        c = pool.open()
        which[c] = (i % 3, lengths[i % 2])
        pool.push(c, audio[which[c]].copy())
    first = pool.step()
    assert [c for c, _, _ in first] == list(range(n_calls))                                       # all of them in one tick
    for c in which:
        pool.close(c)
    parts = {c: [samples] for c, samples, _ in first}
    for c, samples, finished in pool.drain():
        assert finished
        parts[c].append(samples)
    want = {}
    for c, key in which.items():
        if key not in want:
            want[key] = np.stack([_solo(dev, audio[key], m, None, False, None).numpy() for m in range(mics)])
        got = np.concatenate(parts[c], axis=-1)
        got = got[None] if mics == 1 else got
        assert got.shape == (mics, key[1]) and np.array_equal(got, want[key]), c


# ---- 5. the far end is never resynthesised ---------------------------------------------------------------------------------------------------
def test_the_overlap_add_section_of_a_far_end_slot_never_changes(dev):
    from audiodenoiser_amd.echo import EchoStreamPool
    mics, n_calls, length = 2, 2, 700
    C = mics + 1
    pool = EchoStreamPool(dev, n_calls, mics, **KW)
    n_slots, keep, S, RX = n_calls * C, N_FFT - HOP, 2, BLOCK
    tail_off = n_slots * 2 * F * RX + n_slots * F * WINDOW                # the sections before it: X rings, magnitudes
    ring = pool.book.ring_samples
    assert pool._state.numel() == 4 * (tail_off + n_slots * keep * S + n_slots * ring)            # ... and the one after: the layout is this
    tails = pool._state.view(torch.float32)[tail_off:tail_off + n_slots * keep * S].view(n_slots, keep * S)
    far = [c * C + mics for c in range(n_calls)]
    mic = [c * C + m for c in range(n_calls) for m in range(mics)]
    gen = torch.Generator(device="cpu").manual_seed(5)
    tails[far] = torch.randn((len(far), keep * S), generator=gen).to(dev)  # anything: no emit reads a far-end slot's tail
    x = [_call_audio(c, 10 * c, length, mics) for c in range(n_calls)]
    cids = [pool.open() for _ in range(n_calls)]
    outs, ticks = {c: [] for c in cids}, 0
    for lo in range(0, length, 175):
        for c in cids:
            pool.push(c, x[c][:, lo:lo + 175].copy())
        while True:                                                  # a tick runs one step of each call: until nothing is ready
            before = tails.clone()
            tick = pool.step()
            torch.cuda.synchronize(dev)
            if not tick:
                break
            ticks += 1
            assert len(tick) == n_calls and _same(tails[far], before[far]), lo
            assert not _same(tails[mic], before[mic]), lo
            for c, samples, _ in tick:
                outs[c].append(samples)
    for c in cids:
        pool.close(c)
    before = tails.clone()
    for c, samples, finished in pool.drain():
        assert finished
        outs[c].append(samples)
    assert ticks >= 2 and _same(tails[far], before[far])
    for c in cids:
        got = np.concatenate(outs[c], axis=-1)
        want = np.stack([_solo(dev, x[c], m, None, False, None).numpy() for m in range(mics)])
        assert got.shape == (mics, length) and np.array_equal(got, want), c


# ---- 6. one call against the float64 chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", (False, True))
@pytest.mark.parametrize("n_fft", ec.PARITY_N_FFT)
def test_one_call_meets_the_float64_chain(dev, n_fft, gain):
    """Within 4 audio floors, a floor the float32 end-to-end restatement's max |a32 - a64| / max |a64| on the same pair (never below
    2^-23): the bound, the floor, the audio and the chain of test_gpu_echo.py::test_stream_against_the_float64_end_to_end_form."""
    from audiodenoiser_amd.echo import EchoStreamPool
    mic, far, _ = ec.parity_audio(n_fft, ec.E2E_FRAMES)
    hop = n_fft // 4
    pool = EchoStreamPool(dev, 4, 1, n_fft=n_fft, hop_length=hop, block_frames=BLOCK, gain=gain)
    pool.open()                                                     # the calls under test are not the pool's first
    cids = [pool.open() for _ in range(3)]
    x = [np.stack([mic[c], far[c]]).astype(np.float32) for c in range(3)]
    length = x[0].shape[1]
    outs, pos = {c: [] for c in cids}, 0
    while pos < length:
        m = min([length - pos, 5 * BLOCK * hop // 2] + [pool.room(c) for c in cids])
        for i, c in enumerate(cids):
            pool.push(c, x[i][:, pos:pos + m].copy())
        pos += m
        for c, samples, _ in pool.step():
            outs[c].append(samples)
    for c in cids:
        pool.close(c)
    for c, samples, finished in pool.drain():
        assert finished
        outs[c].append(samples)
    for i, c in enumerate(cids):
        got = np.concatenate(outs[c]).astype(np.float64)
        assert got.shape == (length,)
        m32, f32 = x[i][0], x[i][1]                                                  # what the device was given
        want = er.echo_cancel(m32.astype(np.float64), f32.astype(np.float64), n_fft, hop, gain=gain)
        a32 = er.echo_cancel(m32, f32, n_fft, hop, gain=gain, dtype=np.float32)
        scale = float(np.abs(want).max())
        floor = max(float(np.abs(a32.astype(np.float64) - want).max()) / scale, sb.EPS)
        err = float(np.abs(got - want).max())
        print(f"pool n_fft {n_fft} gain {gain} call {i}: {err / scale:.3g} of the maximum, floor {floor:.3g} ({err / scale / floor:.2f} floors; bound 4)")
        assert err <= 4.0 * floor * scale, (i, err / scale, floor)
