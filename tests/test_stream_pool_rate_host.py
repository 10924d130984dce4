"""Stream pool at each feed's own rate, the parts that need no device: PoolBook's bookkeeping for streams at 48 / 44.1 / 16 / 8 kHz
(room at the stream's rate, samples per tick, call counters, the final cut) against stream_rate_plan and the plan functions of
tests/stream_resample_ref.py, and the host-only refusals of adn_stream_pool_rate_state_bytes / _push_rate / _emit_rate."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_resample_ref as ref  # noqa: E402

PLANS = ((64, 16, 16, 1, 0), (512, 128, 48, 8, 4))              # n_fft, hop, W, B, A
RATES = (48000, 44100, 16000, 8000)
WORK = 8000
ADN_ERR_INVALID, ADN_ERR_WORKSPACE = 1, 3


def _book(plan, **kw):
    from audiodenoiser_amd.stream import PoolBook
    return PoolBook(kw.pop("max_streams", 4), kw.pop("backlog_steps", 2), *plan, input_rates=RATES, **kw)


def _push(book, slot, m):
    """What StreamPool.push books for a stream at its own rate (take_rate) or at the working rate (take)."""
    if book.rate[slot] is None:
        book.take(slot, m)
    elif m:
        book.take_rate(slot, m)
    else:
        book.check_rate(slot, 0)


def _close(book, slot):
    """What StreamPool.close books: the resampler in's final call, then the close."""
    if book.rate[slot] is not None and book.received_in[slot] > 0:
        call, before = book.close_rate(slot)
        assert (call, before) == (book.calls_in[slot] - 1, book.received_in[slot]) and call >= 1
    return book.close(slot)


def _tick(book):
    """What StreamPool.step books -> {slot: (samples returned at the stream's rate, finished)}."""
    out = {}
    for slot, k, final in book.rows():
        n = book.count(k, final)
        if book.rate[slot] is not None:
            last = final >= 0 and k == book.n_steps(final) - 1
            before = (book.calls_out[slot], book.work_out[slot])
            call = book.ran_rate(slot, n, last)
            if call is None:
                assert n == 0 and not last
                n = 0
            else:
                assert call[:2] == before and (call[0] == 0) == (call[1] == 0)
                assert n >= 1 or last
                n = call[2]
        out[slot] = (n, book.ran(slot))
    return out


def test_sizes_follow_from_the_rates():
    from audiodenoiser_amd.stream import PoolBook
    for plan in PLANS:
        plain, book = PoolBook(4, 2, *plan), _book(plan)
        same = PoolBook(4, 2, *plan, input_rates=(WORK,))
        assert plain.max_history == plain.reserve == 0 and plain.input_rates == ()
        assert same.ring_samples == plain.ring_samples and same.max_history == 0
        assert book.input_rates == (16000, 44100, 48000)
        assert book.max_history == max(ref.history(a, b) for r in RATES for a, b in ((r, WORK), (WORK, r)))
        # the reserve covers what any resampler in still releases at the end of a stream, whenever it ends
        worst = max(ref.emitted(n, r, WORK, True) - ref.emitted(n, r, WORK) for r in RATES for n in range(0, 3000, 7))
        assert worst <= book.reserve <= worst + 2
        assert book.ring_samples == plain.ring_samples + book.reserve
        # ... and one row of the resampler out holds what the longest step returns at the fastest rate
        n = book.out_stride
        worst = max(ref.emitted(w + n, WORK, r, True) - ref.emitted(w, WORK, r) for r in RATES for w in range(0, 4000, 13))
        assert worst <= book.rate_out_stride <= worst + 3
    with pytest.raises(ValueError, match="input_rates"):
        _book(PLANS[0]).open(22050)
    with pytest.raises(ValueError, match="input_rates"):
        PoolBook(4, 2, *PLANS[0], input_rates=(0,))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("plan", PLANS)
def test_plan_agreement(plan, rate):
    """Seeded open / push / step / close sequences of three streams at `rate` in one book, every number against the plans."""
    from audiodenoiser_amd.stream import stream_plan, stream_rate_plan
    book = _book(plan)
    rng = np.random.default_rng(list(plan) + [rate])
    per = plan[3] * plan[1] * rate // WORK                       # a step's samples at the stream's rate
    for stream in range(6):
        slot = book.open(rate)
        assert (book.rate[slot] is None) == (rate == WORK)
        assert book.calls_in[slot] == book.calls_out[slot] == book.received_in[slot] == book.emitted_in[slot] == 0
        length = int(rng.integers(1, 60000 // (1 if plan[0] == 512 else 8))) if stream else 1
        pos = returned = pushes = 0
        while pos < length:
            m = min(int(rng.integers(0, 3 * per)) if rng.integers(0, 4) else 1, length - pos)
            room = book.room(slot)
            assert room >= 0
            if m > room:
                ticked = _tick(book)
                returned += ticked.get(slot, (0, False))[0]
                m = min(m, book.room(slot))
            _push(book, slot, m)
            pos += m
            pushes += 1 if m else 0
            if rate == WORK:
                assert book.received[slot] == pos
            else:
                assert book.received_in[slot] == pos and book.calls_in[slot] == pushes
                assert book.received[slot] == ref.emitted(pos, rate, WORK)      # what the ring holds, at the working rate
            if rng.integers(0, 2):
                for s, (n, finished) in _tick(book).items():
                    assert s == slot and not finished
                    returned += n
                if rate != WORK:
                    assert book.emitted_in[slot] == returned
                    assert book.work_out[slot] == max(0, book.done[slot] * plan[3] * plan[1] - plan[0] // 2)
                    assert returned == ref.emitted(book.work_out[slot], WORK, rate)
        # every ready step run: the stream has returned what a StreamDenoiser(input_rate=rate) has after the same samples
        while True:
            ticked = _tick(book)
            if not ticked:
                break
            returned += ticked[slot][0]
        if rate == WORK:
            assert returned == stream_plan(length, *plan)[1]
        else:
            assert returned == stream_rate_plan(length, rate, *plan)[0]
        if _close(book, slot):
            raise AssertionError("a stream of at least one sample has steps left at its end")
        assert book.room(slot) == 0 or rate == WORK
        work_length = ref.emitted(length, rate, WORK, True)
        assert book.received[slot] == work_length
        if rate != WORK:
            assert book.calls_in[slot] == pushes + 1
        finished = False
        while not finished:
            n, finished = _tick(book)[slot]
            returned += n
        assert returned == length, (returned, length)             # exactly as many samples as the stream received
        if rate != WORK:
            assert book.work_out[slot] == work_length and book.emitted_in[slot] == length
            assert ref.emitted(work_length, WORK, rate, True) >= length           # the cut only removes samples
        assert book.status[slot] == book.FREE and _tick(book) == {}
    assert book.open(rate) == 0                                   # the slot is reused
    assert book.close(0) is True                                  # a stream of no samples closes at once, no call


@pytest.mark.parametrize("rate", RATES[:3])
@pytest.mark.parametrize("plan", PLANS)
def test_room_is_tight_and_close_always_fits(plan, rate):
    """room fits, room + 1 raises and changes nothing; after pushes that fill room exactly, at every point of a stream, the final
    call of the resampler in still fits the ring: nothing it writes replaces a sample the next step reads."""
    book = _book(plan, backlog_steps=1)
    keep = plan[0] - plan[1]
    for stop_after in range(0, 7):
        slot = book.open(rate)
        for _ in range(stop_after):
            while book.room(slot) == 0:                          # (the first steps free nothing: they read from sample 0 on)
                assert slot in _tick(book), "a full ring always has a step ready"
            m = book.room(slot)
            state = (book.received[slot], book.received_in[slot], book.calls_in[slot], book.room(slot))
            with pytest.raises(RuntimeError, match=r"call step\(\)"):
                book.take_rate(slot, m + 1)
            assert state == (book.received[slot], book.received_in[slot], book.calls_in[slot], book.room(slot))
            book.take_rate(slot, m)
            assert book.room(slot) == 0
            oldest = max(0, book.end_of(book.done[slot] - 1) - keep)
            assert book.received[slot] <= oldest + book.ring_samples
            assert ref.emitted(book.received_in[slot] + 1, rate, WORK, True) > oldest + book.ring_samples       # one more would not
            ticked = _tick(book)
            assert slot in ticked, "a full ring always has a step ready"
        if stop_after == 0:
            book.take_rate(slot, 1)
        book.take_rate(slot, book.room(slot)) if book.room(slot) else None
        oldest = max(0, book.end_of(book.done[slot] - 1) - keep)
        assert _close(book, slot) is False
        assert book.received[slot] <= oldest + book.ring_samples, "the final call's samples fit"
        with pytest.raises(RuntimeError, match="closed"):
            book.take_rate(slot, 1)
        while not _tick(book)[slot][1]:
            pass
        assert book.emitted_in[slot] == book.received_in[slot]


def test_a_mixed_tick_goes_back_in_one_call_per_64_rows(monkeypatch):
    """256 streams at 48 / 44.1 / 16 / 8 kHz, every fourth at the working rate, some still in the steps that return nothing:
    StreamPool.emit_rate makes ceil(rows with a call / 64) calls, whichever rows of the tick they are, and every row's
    audio_offset leads to its own row of what adn_stream_pool_emit wrote.  The library call is recorded, not made."""
    import torch
    from audiodenoiser_amd import stream
    plan = PLANS[0]
    n = 256
    book = _book(plan, max_streams=n, backlog_steps=8)
    for i in range(n):
        assert book.open(RATES[i % 4]) == i
        _push(book, i, 200 * RATES[i % 4] // WORK)
    for i in range(0, n, 5):                                      # every fifth stream is two steps ahead: past the empty steps
        book.ran(i), book.ran(i)
    rows = book.rows()
    assert len(rows) == n
    calls, where = book.rate_calls(rows)
    with_call = [i for i in range(n) if i % 4 != 3 and i % 5 == 0]
    assert [row for row, _ in calls] == with_call and len(where) == n - n // 4
    assert all(where[i] == (None, 0) for i in range(n) if i % 4 != 3 and i % 5)
    seen = []

    class Lib:
        @staticmethod
        def adn_stream_pool_emit_rate(state, nbytes, n_slots, max_h, work, table, n_rows, audio_in, in_stride, out, out_stride, st):
            seen.append([(table[i].slot, audio_in + 4 * (i * in_stride + table[i].audio_offset)) for i in range(n_rows)])
            return 0
    monkeypatch.setattr(stream._lib, "load", lambda: Lib)
    monkeypatch.setattr(stream, "_stream", lambda dev: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())       # no device here
    pool = stream.StreamPool.__new__(stream.StreamPool)
    pool.book, pool.device, pool._rate_args = book, None, (0, 0, n, book.max_history, WORK)
    for extra in (0, 100):                                        # 39 rows: one call; 139: three
        many = calls + [(n + j, calls[0][1]) for j in range(extra)]
        out = torch.zeros((n + extra, book.out_stride))
        del seen[:]
        rout = pool.emit_rate(out, many)
        assert rout.shape == (len(many), book.rate_out_stride)
        assert len(seen) == -(-len(many) // stream.POOL_RATE_MAX_ROWS) and [len(g) for g in seen][:-1] == [64] * (len(seen) - 1)
        flat = [x for g in seen for x in g]
        assert flat == [(c[0], out[row].data_ptr()) for row, c in many]


# ---- the C entry points, without a device ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from audiodenoiser_amd import _lib
    return _lib.load()


def test_rate_state_bytes(lib):
    v = ctypes.c_size_t()
    for n_slots, h in ((1, 0), (1, 391), (64, 391), (300, 16384)):
        assert lib.adn_stream_pool_rate_state_bytes(n_slots, h, ctypes.byref(v)) == 0
        assert v.value == n_slots * 2 * 2 * h * 4                 # per slot and direction two slots of max_history floats
    for n_slots, h in ((0, 391), ((1 << 20) + 1, 391), (4, -1), (4, 16385)):
        assert lib.adn_stream_pool_rate_state_bytes(n_slots, h, ctypes.byref(v)) == ADN_ERR_INVALID, (n_slots, h)
        assert b"adn_stream_pool_rate_state_bytes" in lib.adn_last_error()
    assert lib.adn_stream_pool_rate_state_bytes(4, 391, None) == ADN_ERR_INVALID


def test_bad_calls_launch_nothing(lib):
    """Every refusal below comes from the argument checks, before any HIP call: the pointers are host memory."""
    from audiodenoiser_amd._lib import StreamPoolRateRow
    plan = PLANS[1]
    n_slots, big, max_h = 8, 1 << 40, 391
    ring = plan[0] - plan[1] + (plan[3] + plan[4] - 1) * plan[1] + plan[0] // 2 + plan[3] * plan[1]
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    v = ctypes.c_size_t()
    assert lib.adn_stream_pool_state_bytes(n_slots, *plan, ring, ctypes.byref(v)) == 0
    need = v.value
    assert lib.adn_stream_pool_rate_state_bytes(n_slots, max_h, ctypes.byref(v)) == 0
    rate_need = v.value

    def table(r):
        return (StreamPoolRateRow * len(r))(*[StreamPoolRateRow(*x) for x in r])

    def push(r, n=None, state=ptr, nbytes=big, rate_state=ptr, rate_bytes=big, h=max_h, work=WORK, audio=ptr, slots=n_slots,
             ring=ring):
        return lib.adn_stream_pool_push_rate(state, nbytes, slots, *plan, ring, rate_state, rate_bytes, h, work, table(r),
                                             len(r) if n is None else n, audio, None)

    def emit(r, n=None, rate_state=ptr, rate_bytes=big, h=max_h, work=WORK, audio=ptr, in_stride=4096, out=ptr, out_stride=1 << 20,
             slots=n_slots, **_):
        r = [x[:6] + (0,) for x in r]
        return lib.adn_stream_pool_emit_rate(rate_state, rate_bytes, slots, h, work, table(r), len(r) if n is None else n, audio,
                                             in_stride, out, out_stride, None)

    # rows: (slot, rate, call_index, received_before, n_new, final, audio_offset)
    ok = (0, 48000, 0, 0, 480, 0, 0)
    for call, name in ((push, b"adn_stream_pool_push_rate"), (emit, b"adn_stream_pool_emit_rate")):
        def refused(*a, **kw):
            rc = call(*a, **kw)
            assert name in lib.adn_last_error(), lib.adn_last_error()
            return rc == ADN_ERR_INVALID
        assert call([ok], rate_bytes=rate_need - 1) == ADN_ERR_WORKSPACE and b"adn_stream_pool_rate_state_bytes" in lib.adn_last_error()
        assert refused([ok], rate_state=None) and b"null" in lib.adn_last_error()
        assert refused([ok], audio=None) and b"null" in lib.adn_last_error()
        assert refused([ok], n=0) and b"n_rows" in lib.adn_last_error()
        assert refused([(i % n_slots, 48000, 0, 0, 480, 0, 0) for i in range(65)]) and b"n_rows" in lib.adn_last_error()
        assert refused([(n_slots, 48000, 0, 0, 480, 0, 0)]) and b"slot" in lib.adn_last_error()
        assert refused([(-1, 48000, 0, 0, 480, 0, 0)])
        assert refused([ok, (3, 44100, 0, 0, 441, 0, 480), (0, 16000, 2, 99, 160, 0, 921)]) and b"twice" in lib.adn_last_error()
        # H of 44.1 <-> 8 kHz is 391 / 65, of 48 <-> 8 kHz 391 / 66: one less than a row needs is refused, row by row
        assert refused([ok, (1, 44100, 0, 0, 441, 0, 480)], h=390 if call is push else 65) and b"max_history" in lib.adn_last_error()
        assert refused([ok], h=16385)
        assert refused([ok], slots=0) and refused([ok], slots=(1 << 20) + 1)
        # everything adn_resample_stream refuses, row by row
        assert refused([(0, 48000, 0, 480, 480, 0, 0)]) and b"call_index" in lib.adn_last_error()      # call 0 with samples before
        assert refused([(0, 48000, 1, 0, 480, 0, 0)]) and b"call_index" in lib.adn_last_error()
        assert refused([(0, 48000, -1, 0, 480, 0, 0)]) and refused([(0, 48000, 1, -5, 480, 0, 0)])
        assert refused([ok, (1, 48000, 3, 960, 0, 0, 0)]) and b"n_new" in lib.adn_last_error()          # nothing new, not final
        assert refused([(1, 48000, 3, 960, -1, 1, 0)])
        assert refused([(0, 48000, 0, 0, 480, 2, 0)]) and b"final" in lib.adn_last_error()
        assert refused([(0, 0, 0, 0, 480, 0, 0)]) and refused([(0, -8000, 0, 0, 480, 0, 0)])
        assert refused([(0, 8000 * 4097, 0, 0, 480, 0, 0)]) and b"4096" in lib.adn_last_error()
        assert refused([ok], work=0)
        assert refused([(0, 48000, 5, (1 << 31) - 10, 480, 0, 0)]) and b"2^31" in lib.adn_last_error()
        assert refused([(0, 48000, 5, 10, 1 << 31, 0, 0)])
    # push: the pool's own arguments, the ring and the offsets
    assert push([ok], nbytes=need - 1) == ADN_ERR_WORKSPACE and b"adn_stream_pool_state_bytes" in lib.adn_last_error()
    assert push([ok], state=None) == ADN_ERR_INVALID
    assert push([ok], ring=ring - plan[3] * plan[1] - 1) == ADN_ERR_INVALID and b"ring_samples" in lib.adn_last_error()
    assert push([(0, 48000, 0, 0, 480, 0, -1)]) == ADN_ERR_INVALID and b"audio_offset" in lib.adn_last_error()
    assert lib.adn_stream_pool_emit_rate(ptr, big, n_slots, max_h, WORK, table([(0, 48000, 0, 0, 480, 0, -1)]), 1, ptr, 4096, ptr, 1 << 20,
                                         None) == ADN_ERR_INVALID and b"audio_offset" in lib.adn_last_error()
    n_long = (ring + 40) * 6                                      # 48 -> 8 kHz: more than ring_samples outputs in one row
    assert push([(0, 48000, 0, 0, n_long, 0, 0)]) == ADN_ERR_INVALID and b"ring_samples" in lib.adn_last_error()
    assert push([(0, 8000, 0, 0, ring + 1, 0, 0)]) == ADN_ERR_INVALID and b"ring_samples" in lib.adn_last_error()      # a copy row too
    assert push([(0, 12000, 7, (1 << 31) - 2000, 480, 0, 0)]) == ADN_ERR_INVALID and b"2^30" in lib.adn_last_error()
    # emit: the strides, once there is more than one row
    two = [(0, 48000, 0, 0, 480, 0, 0), (1, 44100, 0, 0, 300, 0, 0)]
    assert emit(two, in_stride=479) == ADN_ERR_INVALID and b"in_stride" in lib.adn_last_error()
    assert emit(two, out_stride=ref.emitted(480, WORK, 48000) - 1) == ADN_ERR_INVALID and b"out_stride" in lib.adn_last_error()
    assert emit(two, out=None) == ADN_ERR_INVALID and b"null" in lib.adn_last_error()
    assert emit(two, in_stride=-1) == ADN_ERR_INVALID and emit(two, out_stride=-1) == ADN_ERR_INVALID


def test_symbols_in_header_and_binding():
    from audiodenoiser_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "adn.h")).read()
    for name in ("adn_stream_pool_rate_state_bytes", "adn_stream_pool_push_rate", "adn_stream_pool_emit_rate"):
        assert name in _lib.EXPORTED_SYMBOLS and f"ADN_API int {name}(" in header and hasattr(_lib.load(), name)
    assert "#define ADN_STREAM_POOL_RATE_MAX_ROWS 64" in header
    from audiodenoiser_amd.stream import POOL_RATE_MAX_ROWS
    assert POOL_RATE_MAX_ROWS == 64 and ctypes.sizeof(_lib.StreamPoolRateRow) == 48
