"""Recordings in the stream pools, on the device: adn_wpe_mc_stream_pool and adn_mvdr_stream_pool (include/adn.h, "dereverb stream
multichannel" and "beamform stream"), DereverbStreamPool(channels=C) and BeamformStreamPool.

There is no new arithmetic, so every comparison but the last is exact bit equality, and the float64 bounds of the lockstep forms
(tests/test_gpu_dereverb_mc_stream.py, tests/test_gpu_beamform_stream.py) carry over through it:
* C call against C call: a pool state and a lockstep state (max_steps = 1: the same ring geometry, [slot][B][F] float2 first) hold
  the same ring cells, the pool's recordings in scrambled order; the pool call must leave the ring cells, the window columns and
  the operator-state slots the lockstep call leaves, and no other byte of the pool state, of the unnamed operator-state slots
  (handed over as 0xFF bytes) or around them.  Three steps: a fresh one, a carried one, a last one of three frames.
* Pool against solo: the scenario of test_pool_streams_equal_solo_streams -- staggered opens, uneven pushes of numpy arrays and
  device tensors, a recording closed mid-way, a slot reused without a reset, one recording at 48 kHz.
* 33 recordings of 8 channels: 264 stream rows in one tick, cut 32 + 1.
* One recording against the float64 chain of tests/beamform_stream_ref.py: max |a - a64| <= 4 floor max |a64|, the floor the same
  chain in float32 on the host -- the bound and the floor of the lockstep stream's audio.

n_fft 64, hop 16, block 4 everywhere: F = 33 is a multiple of no tile (16, 8 bins), a step is 64 samples.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_stream_ref as bs  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import footprint as fp  # noqa: E402
import solver_bounds as sb  # noqa: E402

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
    _lib().check(fn(*args, ctypes.byref(need)), fn.__name__)
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


# ---- 1. C call against C call --------------------------------------------------------------------------------------------------------
RECORDINGS, NAMED = 5, (4, 1, 2)                        # the pool's recordings; the ones a call names, scrambled; 0 and 3 are not
STEPS = ((0, -1), (1, -1), (2, 165))                    # fresh; carried; the last step of 11 frames: three frames


def _against_lockstep(dev, channels, pool_call, lock_call, pool_need, lock_need):
    """`pool_call(pstate, rows, y, ostate)` against `lock_call(sstate, y, first_step, final_length, ostate)` on the same cells."""
    L, c = _lib().load(), channels
    n_slots, n = RECORDINGS * c, len(NAMED) * c
    gen = torch.Generator(device="cpu").manual_seed(100 + c)
    pstate = torch.randn(_size(L.adn_stream_pool_state_bytes, n_slots, *PLAN, RING) // 4, generator=gen).to(dev).view(torch.uint8)
    sstate = torch.randn(_size(L.adn_stream_state_bytes, n, *PLAN, 1) // 4, generator=gen).to(dev).view(torch.uint8)
    p_ostate, h_ostate = fp.carve(pool_need, 0xFF, dev)
    l_ostate = torch.full((lock_need,), 0xFF, dtype=torch.uint8, device=dev)
    per = pool_need // RECORDINGS
    assert per * RECORDINGS == pool_need and per * len(NAMED) == lock_need
    slots = [r * c + ch for r in NAMED for ch in range(c)]
    for step, final in STEPS:
        cells = torch.randn((n, BLOCK, F, 2), generator=gen).to(dev)
        _ring(pstate, n_slots)[slots] = cells
        _ring(sstate, n)[:] = cells
        y = torch.rand((n, 1, F, WINDOW), generator=gen).to(dev)
        y_lock = y.clone()
        y_pool, h_y = fp.carve_copy(y, dev)
        before, o_before = pstate.clone(), p_ostate.clone()
        lock_call(sstate, y_lock, step, final, l_ostate)
        pool_call(pstate, [(s, step, final) for s in slots], y_pool, p_ostate)
        torch.cuda.synchronize(dev)
        what = (c, step)
        # the ring cells and the window columns of the lockstep call, bit for bit, and something was written
        assert _same(_ring(pstate, n_slots)[slots], _ring(sstate, n)), what
        assert _same(y_pool, y_lock) and not _same(y_lock, y), what
        # the operator state: slot NAMED[g] of the pool is slot g of the lockstep state
        po, lo = p_ostate.view(RECORDINGS, per), l_ostate.view(len(NAMED), per)
        assert torch.equal(po[list(NAMED)], lo) and not torch.equal(po[list(NAMED)], o_before.view(RECORDINGS, per)[list(NAMED)]), what
        # and not one byte else: the other slots' cells, the rest of the pool state, the unnamed operator-state slots, the guards
        want = before.clone()
        _ring(want, n_slots)[slots] = _ring(sstate, n)
        assert torch.equal(pstate, want), what
        others = [r for r in range(RECORDINGS) if r not in NAMED]
        assert bool((po[others] == 0xFF).all()), what
        fp.assert_guards_intact(h_ostate, "operator state of the pool")
        fp.assert_guards_intact(h_y, "windows of the pool")


@pytest.mark.parametrize("channels", (2, 5, 7, 8), ids=lambda c: f"C{c}")      # 4 lanes per bin, and 8; 7: the least round record
def test_mvdr_pool_call_leaves_what_the_lockstep_call_leaves(dev, channels):
    lib, c = _lib(), channels
    L = lib.load()
    p = lib.MvdrStreamParamsStruct(c - 1, 2, 0.99, 1e-3, 1e-3)
    n = len(NAMED) * c

    def pool_call(pstate, rows, y, ostate):
        lib.check(L.adn_mvdr_stream_pool(pstate.data_ptr(), pstate.numel(), RECORDINGS * c, c, *PLAN, RING, _rows(rows), len(rows),
                                         y.data_ptr(), ctypes.byref(p), ostate.data_ptr(), ostate.numel(), _stream(dev)),
                  "adn_mvdr_stream_pool")

    def lock_call(sstate, y, step, final, ostate):
        lib.check(L.adn_mvdr_stream(sstate.data_ptr(), sstate.numel(), y.data_ptr(), n, c, step, 1, final, *PLAN, 1, ctypes.byref(p),
                                    ostate.data_ptr(), ostate.numel(), _stream(dev)), "adn_mvdr_stream")

    with torch.cuda.device(dev):
        _against_lockstep(dev, c, pool_call, lock_call, _size(L.adn_mvdr_stream_state_bytes, RECORDINGS, c, F, ctypes.byref(p)),
                          _size(L.adn_mvdr_stream_state_bytes, len(NAMED), c, F, ctypes.byref(p)))


@pytest.mark.parametrize("channels,taps", ((2, 16), (4, 8), (7, 4)), ids=("C2K16", "C4K8", "C7K4"))
def test_wpe_pool_call_leaves_what_the_lockstep_call_leaves(dev, channels, taps):
    lib, c = _lib(), channels
    L = lib.load()
    p = lib.WpeStreamParamsStruct(taps, 3, 0.99, 300.0, 0.01, 0.9)
    n = len(NAMED) * c

    def pool_call(pstate, rows, y, ostate):
        lib.check(L.adn_wpe_mc_stream_pool(pstate.data_ptr(), pstate.numel(), RECORDINGS * c, c, *PLAN, RING, _rows(rows), len(rows),
                                           y.data_ptr(), ctypes.byref(p), ostate.data_ptr(), ostate.numel(), _stream(dev)),
                  "adn_wpe_mc_stream_pool")

    def lock_call(sstate, y, step, final, ostate):
        lib.check(L.adn_wpe_mc_stream(sstate.data_ptr(), sstate.numel(), y.data_ptr(), n, c, step, 1, final, *PLAN, 1, ctypes.byref(p),
                                      ostate.data_ptr(), ostate.numel(), _stream(dev)), "adn_wpe_mc_stream")

    with torch.cuda.device(dev):
        _against_lockstep(dev, c, pool_call, lock_call, _size(L.adn_wpe_mc_stream_state_bytes, RECORDINGS, c, F, ctypes.byref(p)),
                          _size(L.adn_wpe_mc_stream_state_bytes, len(NAMED), c, F, ctypes.byref(p)))


def test_one_channel_is_the_single_channel_pool_call_bit_for_bit(dev):
    lib = _lib()
    L = lib.load()
    p = lib.WpeStreamParamsStruct(20, 3, 0.99, 300.0, 0.01, 0.9)
    n_slots, slots = 5, (3, 0, 4)
    gen = torch.Generator(device="cpu").manual_seed(7)
    start = torch.randn(_size(L.adn_stream_pool_state_bytes, n_slots, *PLAN, RING) // 4, generator=gen).to(dev).view(torch.uint8)
    need = _size(L.adn_wpe_mc_stream_state_bytes, n_slots, 1, F, ctypes.byref(p))
    assert need == _size(L.adn_wpe_stream_state_bytes, n_slots, F, ctypes.byref(p))
    states = [start.clone(), start.clone()]
    ostates = [torch.full((need,), 0xFF, dtype=torch.uint8, device=dev) for _ in range(2)]
    with torch.cuda.device(dev):
        for step, final in STEPS:
            cells = torch.randn((len(slots), BLOCK, F, 2), generator=gen).to(dev)
            y = torch.rand((len(slots), 1, F, WINDOW), generator=gen).to(dev)
            ys = [y.clone(), y.clone()]
            rows = [(s, step, final) for s in slots]
            for st in states:
                _ring(st, n_slots)[list(slots)] = cells
            lib.check(L.adn_wpe_stream_pool(states[0].data_ptr(), states[0].numel(), n_slots, *PLAN, RING, _rows(rows), len(rows),
                                            ys[0].data_ptr(), ctypes.byref(p), ostates[0].data_ptr(), need, _stream(dev)),
                      "adn_wpe_stream_pool")
            lib.check(L.adn_wpe_mc_stream_pool(states[1].data_ptr(), states[1].numel(), n_slots, 1, *PLAN, RING, _rows(rows), len(rows),
                                               ys[1].data_ptr(), ctypes.byref(p), ostates[1].data_ptr(), need, _stream(dev)),
                      "adn_wpe_mc_stream_pool")
            assert torch.equal(states[0], states[1]) and _same(ys[0], ys[1]) and torch.equal(ostates[0], ostates[1]), step
            assert not _same(ys[0], y)


# ---- 2. pool against solo ------------------------------------------------------------------------------------------------------------
def _push_all(sd, xd):
    return torch.cat([sd.push(xd), sd.flush()], dim=-1)


def _scenario(pool, dev, sig, rates):
    """Four recordings through a pool of three: staggered opens, uneven pushes (numpy and device tensors in turn), recordings 0 and
    1 closed while 2 is in mid-flight, recording 3 in recording 0's slots without a reset.  -> the samples of each, on the host."""
    lengths = [s.shape[1] for s in sig]
    outs, rid, pos, by_rid = [[] for _ in sig], {}, [0] * 4, {}

    def take(result):
        for r, samples, finished in result:
            i = by_rid[r]
            outs[i].append(torch.from_numpy(samples) if isinstance(samples, np.ndarray) else samples.cpu())
            if finished:
                del by_rid[r]

    def open_(i):
        rid[i] = pool.open(rates[i])
        by_rid[rid[i]] = i

    def push(i, m):
        m = min(m, lengths[i] - pos[i], pool.room(rid[i]))
        block = np.ascontiguousarray(sig[i][:, pos[i]:pos[i] + m])
        pool.push(rid[i], block if i % 2 == 0 else torch.from_numpy(block.copy()).to(dev))
        pos[i] += m

    open_(0)
    push(0, 350)
    take(pool.step())
    open_(1)
    open_(2)
    for m0, m1, m2 in ((750, 3, 4500), (1, 1000, 1), (1000, 547, 3500), (899, 0, 1999)):
        push(0, m0)
        push(1, m1)
        push(2, m2)
        take(pool.step())
    assert pos[0] == lengths[0] == 3000 and pos[1] == lengths[1] == 1550
    pool.close(rid[0])                                           # closed while recording 2 is in mid-flight
    pool.close(rid[1])
    while 0 in by_rid.values() or 1 in by_rid.values():
        take(pool.step())
    open_(3)                                                     # the first recording's slots, left as they were: no reset
    assert rid[3] == rid[0]
    while pos[2] < lengths[2] or pos[3] < lengths[3]:
        push(2, 1250)
        push(3, 617)
        take(pool.step())
    pool.close(rid[2])
    pool.close(rid[3])
    take(pool.drain())
    assert not by_rid and pool.step() == []
    return [torch.cat(o, dim=-1) for o in outs]


_LENGTHS, _RATES = (3000, 1550, 13000, 2000), (None, None, 48000, None)


def _signals(audio, channels):
    """Four recordings of `channels` microphones out of the three groups of a cases module's parity audio (the fourth: the first
    one from another place)."""
    c = channels
    starts = ((0, 100), (1, 0), (2, 40), (0, 5000))
    return [np.ascontiguousarray(audio[g * c:(g + 1) * c, at:at + n]) for (g, at), n in zip(starts, _LENGTHS)]


@pytest.mark.parametrize("channels,wpe,gain", ((2, False, False), (3, True, True), (5, False, True), (4, True, False), (7, True, False)),
                         ids=("C2", "C3-wpe-gain", "C5-gain", "C4-wpe", "C7-wpe"))
def test_every_recording_of_the_beamformer_pool_equals_its_solo_run(dev, channels, wpe, gain):
    from audiodenoiser_amd.beamform import BeamformStreamPool, MvdrStreamParams, StreamBeamformer
    c = channels
    params = MvdrStreamParams(ref_channel=c - 1, refresh=2)
    sig = _signals(bc.parity_audio(N_FFT, 1000, c), c)
    pool = BeamformStreamPool(dev, 3, c, backlog_steps=64, params=params, wpe=wpe, gain=gain, input_rates=(48000,), **KW)
    assert pool.latency_samples == (BLOCK - 1) * HOP + N_FFT and pool.channels == c and pool.max_streams == 3
    got = _scenario(pool, dev, sig, _RATES)
    for i, s in enumerate(sig):
        solo = StreamBeamformer(dev, n_streams=c, channels=c, params=params, wpe=wpe, gain=gain, input_rate=_RATES[i], **KW)
        want = _push_all(solo, torch.from_numpy(s.copy()).to(dev)).cpu()
        assert got[i].shape == want.shape == (_LENGTHS[i],), (i, got[i].shape, want.shape)         # as many samples as came in
        assert torch.equal(got[i], want), (i, float((got[i] - want).abs().max()))
    with pytest.raises(RuntimeError):
        pool.network(None)
    with pytest.raises(ValueError):
        pool.push(pool.open(), np.zeros(10, np.float32))                                           # (C, m), not (m,)


@pytest.mark.parametrize("channels,gain", ((2, False), (4, True), (7, False)), ids=("C2", "C4-gain", "C7"))
def test_every_recording_of_the_dereverb_pool_equals_its_solo_run(dev, channels, gain):
    from audiodenoiser_amd.dereverb import DereverbStreamPool, StreamDereverberator
    c = channels
    sig = _signals(mc.parity_audio(N_FFT, 1000, c), c)
    pool = DereverbStreamPool(dev, max_streams=3, backlog_steps=64, gain=gain, input_rates=(48000,), channels=c, **KW)
    assert pool.params.taps == 32 // c and pool.channels == c
    got = _scenario(pool, dev, sig, _RATES)
    for i, s in enumerate(sig):
        solo = StreamDereverberator(dev, n_streams=c, channels=c, gain=gain, input_rate=_RATES[i], **KW)
        want = _push_all(solo, torch.from_numpy(s.copy()).to(dev)).cpu()
        assert got[i].shape == want.shape == (c, _LENGTHS[i]), (i, got[i].shape, want.shape)
        assert torch.equal(got[i], want), (i, float((got[i] - want).abs().max()))


# ---- 3. more than 256 stream rows in one tick ------------------------------------------------------------------------------------------
def test_33_recordings_of_8_channels_in_one_tick(dev):
    from audiodenoiser_amd.beamform import BeamformStreamPool, StreamBeamformer
    c, n = 8, 33
    audio = bc.parity_audio(N_FFT, 40, c)
    lengths = (330, 250)
    pool = BeamformStreamPool(dev, n, c, **KW)
    assert len(pool.book.calls([(r, 0, -1) for r in range(n)])) == 2
    which = {}
    for i in range(n):
        r = pool.open()
        which[r] = (i % 3, lengths[i % 2])
        g, length = which[r]
        pool.push(r, audio[g * c:(g + 1) * c, :length].copy())
    first = pool.step()
    assert [r for r, _, _ in first] == list(range(n))                                             # 264 stream rows: 256 + 8
    for r in which:
        pool.close(r)
    parts = {r: [samples] for r, samples, _ in first}
    for r, samples, finished in pool.drain():
        assert finished
        parts[r].append(samples)
    solo, want = StreamBeamformer(dev, n_streams=c, channels=c, **KW), {}
    for r, (g, length) in which.items():
        if (g, length) not in want:
            want[g, length] = _push_all(solo, torch.from_numpy(audio[g * c:(g + 1) * c, :length].copy()).to(dev)).cpu().numpy()
        got = np.concatenate(parts[r])
        assert got.shape == (length,) and np.array_equal(got, want[g, length]), r


# ---- 4. one recording against the float64 chain ------------------------------------------------------------------------------------------
def test_one_recording_meets_the_float64_chain(dev):
    from audiodenoiser_amd.beamform import BeamformStreamPool, MvdrStreamParams
    c, length = 2, 22 * HOP + 5                                     # 23 frames: five whole blocks and one of three frames
    x = np.ascontiguousarray(bc.parity_audio(N_FFT, 23, c)[:c, :length])
    pool = BeamformStreamPool(dev, 2, c, params=MvdrStreamParams(ref_channel=c - 1), **KW)
    pool.open()                                                     # the recording under test is not the pool's first
    r = pool.open()
    outs = []
    for block in (x[:, :200], x[:, 200:]):
        pool.push(r, block.copy())
        outs += [samples for rid, samples, _ in pool.step() if rid == r]
    pool.close(r)
    outs += [samples for rid, samples, _ in pool.drain() if rid == r]
    got = np.concatenate(outs).astype(np.float64)
    assert got.shape == (length,)
    kw = dict(ref_channel=c - 1)
    want = bs.stream_beamform(x.astype(np.float64), N_FFT, HOP, kw)
    a32 = bs.stream_beamform(x, N_FFT, HOP, kw, dtype=np.float32)
    scale = float(np.abs(want).max())
    floor = max(float(np.abs(a32.astype(np.float64) - want).max()) / scale, sb.EPS)
    err = float(np.abs(got - want).max())
    print(f"pool C {c}: floor {floor:.3g}; err {err / scale:.3g} = {err / scale / floor:.2f} floors (bound 4)")
    assert err <= 4.0 * floor * scale, (err / scale, floor)
