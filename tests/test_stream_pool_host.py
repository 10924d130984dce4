"""Stream pool, the parts that need no device: adn_stream_pool_state_bytes against the section sizes include/adn.h documents, the
host-only limits of the adn_stream_pool_* entry points, and the bookkeeping of StreamPool (PoolBook: the ready rule, the samples
a tick returns, the room of a ring) against adn_stream_plan."""
import ctypes

import numpy as np
import pytest

PLANS = ((512, 128, 64, 16, 0), (512, 128, 48, 8, 4), (256, 64, 32, 16, 16), (64, 16, 16, 1, 0), (512, 128, 192, 16, 0))  # n_fft, hop, W, B, A
ADN_ERR_INVALID, ADN_ERR_WORKSPACE = 1, 3


@pytest.fixture(scope="module")
def lib():
    from audiodenoiser_amd import _lib
    return _lib.load()


def ring_min(n_fft, hop, w, b, a):
    return n_fft - hop + (b + a - 1) * hop + n_fft // 2 + b * hop


def _bytes(lib, n_slots, plan, ring):
    v = ctypes.c_size_t()
    assert lib.adn_stream_pool_state_bytes(n_slots, *plan, ring, ctypes.byref(v)) == 0, lib.adn_last_error()
    return v.value


@pytest.mark.parametrize("plan", PLANS)
def test_state_bytes_are_the_documented_sections(lib, plan):
    n_fft, hop, w, b, a = plan
    f, keep, r0 = n_fft // 2 + 1, n_fft - hop, ring_min(*plan)
    for n_slots in (1, 2, 7, 64, 300):
        for ring in (r0, r0 + 1, r0 + 5 * b * hop):
            want = 4 * n_slots * (2 * (b + a) * f + w * f + 2 * keep + ring)          # X, mag, tail, ring; floats
            assert _bytes(lib, n_slots, plan, ring) == want, (n_slots, ring)
    sizes = [_bytes(lib, n, plan, r0) for n in (1, 2, 3, 64, 65)]
    assert all(x < y for x, y in zip(sizes, sizes[1:]))                               # monotone in n_slots
    sizes = [_bytes(lib, 3, plan, r) for r in (r0, r0 + 1, r0 + 1000, 1 << 20)]
    assert all(x < y for x, y in zip(sizes, sizes[1:]))                               # ... and in ring_samples
    # the pool has no hist section: with the smallest ring a slot is n_fft/2 + (B + A - 1) hop + B hop - (n_fft - hop) floats larger
    # than a stream state of max_steps = 1 (which carries 2 (n_fft - hop) floats of history)
    v = ctypes.c_size_t()
    assert lib.adn_stream_state_bytes(1, *plan, 1, ctypes.byref(v)) == 0
    assert _bytes(lib, 1, plan, r0) - v.value == 4 * (r0 - 2 * keep)


@pytest.mark.parametrize("plan", PLANS)
def test_host_only_limits(lib, plan):
    n_fft, hop, w, b, a = plan
    v = ctypes.c_size_t()
    r0 = ring_min(*plan)
    assert lib.adn_stream_pool_state_bytes(1, *plan, r0 - 1, ctypes.byref(v)) == ADN_ERR_INVALID
    assert b"adn_stream_pool_state_bytes" in lib.adn_last_error() and b"ring_samples" in lib.adn_last_error()
    assert lib.adn_stream_pool_state_bytes(1, *plan, (1 << 28) + 1, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_stream_pool_state_bytes(0, *plan, r0, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_stream_pool_state_bytes((1 << 20) + 1, *plan, r0, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_stream_pool_state_bytes(1, *plan, r0, None) == ADN_ERR_INVALID
    for bad in ((n_fft, hop, w, w, 1), (n_fft, n_fft // 4 + 1, w, b, a), (n_fft, 0, w, b, a), (n_fft - 4, hop, w, b, a),
                (8192, hop, w, b, a), (n_fft, hop, 15, 8, 0), (n_fft, hop, w, 0, a), (n_fft, hop, w, b, -1)):
        assert lib.adn_stream_pool_state_bytes(4, *bad, 1 << 20, ctypes.byref(v)) == ADN_ERR_INVALID, bad
        assert b"block + lookahead <= window" in lib.adn_last_error()


def test_bad_calls_launch_nothing(lib):
    """Every refusal below comes from the argument checks, before any HIP call: the pointers are host memory."""
    from audiodenoiser_amd._lib import StreamPoolRow
    plan = (512, 128, 64, 16, 0)
    ring, n_slots, big = ring_min(*plan), 8, 1 << 40
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    need = _bytes(lib, n_slots, plan, ring)

    def rows(*r):
        return (StreamPoolRow * len(r))(*[StreamPoolRow(*x) for x in r]), len(r)

    def analyze(r, n=None, state=ptr, nbytes=big, out=ptr):
        arr, k = rows(*r)
        return lib.adn_stream_pool_analyze(state, nbytes, n_slots, *plan, ring, arr, k if n is None else n, out, None)

    def emit(r, n=None, state=ptr, nbytes=big, y=ptr, stride=16 * 128 + 256):
        arr, k = rows(*r)
        return lib.adn_stream_pool_emit(state, nbytes, n_slots, *plan, ring, arr, k if n is None else n, y, ptr, stride, None)

    for call in (analyze, emit):
        assert call([(0, 0, -1)], nbytes=need - 1) == ADN_ERR_WORKSPACE and b"adn_stream_pool_state_bytes" in lib.adn_last_error()
        assert call([(0, 0, -1)], state=None) == ADN_ERR_INVALID and b"null" in lib.adn_last_error()
        assert call([(0, 0, -1)], n=0) == ADN_ERR_INVALID and b"n_rows" in lib.adn_last_error()
        assert call([(i % n_slots, 0, -1) for i in range(257)]) == ADN_ERR_INVALID and b"n_rows" in lib.adn_last_error()
        assert call([(n_slots, 0, -1)]) == ADN_ERR_INVALID and b"slot" in lib.adn_last_error()
        assert call([(-1, 0, -1)]) == ADN_ERR_INVALID
        assert call([(0, 0, -1), (3, 2, -1), (0, 1, -1)]) == ADN_ERR_INVALID and b"twice" in lib.adn_last_error()
        # the stream section's limits, row by row: a stream of 1000 samples has T = 8 frames, K = 1 step
        assert call([(1, 0, 1000), (2, 1, 1000)]) == ADN_ERR_INVALID and b"last step" in lib.adn_last_error()
        assert call([(1, -1, -1)]) == ADN_ERR_INVALID
        assert call([(1, 0, 0)]) == ADN_ERR_INVALID and b"final_length" in lib.adn_last_error()
        assert call([(1, (1 << 30) // (16 * 128), -1)]) == ADN_ERR_INVALID and b"2^30" in lib.adn_last_error()
    assert analyze([(0, 0, -1)], out=None) == ADN_ERR_INVALID
    assert emit([(0, 0, -1)], y=None) == ADN_ERR_INVALID
    assert emit([(0, 0, -1)], stride=16 * 128 + 255) == ADN_ERR_INVALID and b"out_stride" in lib.adn_last_error()

    def write(slot=0, n=1, position=0, state=ptr, nbytes=big, audio=ptr):
        return lib.adn_stream_pool_write(state, nbytes, n_slots, *plan, ring, slot, audio, n, position, None)

    assert write(nbytes=need - 1) == ADN_ERR_WORKSPACE
    assert write(slot=n_slots) == ADN_ERR_INVALID and write(slot=-1) == ADN_ERR_INVALID
    assert write(n=ring + 1) == ADN_ERR_INVALID and b"ring_samples" in lib.adn_last_error()
    assert write(n=-1) == ADN_ERR_INVALID and write(position=-1) == ADN_ERR_INVALID
    assert write(position=(1 << 30) - 1) == ADN_ERR_INVALID
    assert write(audio=None) == ADN_ERR_INVALID and write(state=None) == ADN_ERR_INVALID
    assert write(n=0, audio=None) == 0                                   # nothing to copy: nothing is enqueued
    assert lib.adn_stream_pool_reset(ptr, need - 1, n_slots, *plan, ring, -1, None) == ADN_ERR_WORKSPACE
    assert lib.adn_stream_pool_reset(ptr, big, n_slots, *plan, ring, n_slots, None) == ADN_ERR_INVALID
    assert lib.adn_stream_pool_reset(ptr, big, n_slots, *plan, ring, -2, None) == ADN_ERR_INVALID
    assert lib.adn_stream_pool_reset(ptr, big, n_slots, *plan, ring - 1, -1, None) == ADN_ERR_INVALID


def _plan(lib, plan, received):
    s, e = ctypes.c_long(), ctypes.c_long()
    assert lib.adn_stream_plan(*plan, received, ctypes.byref(s), ctypes.byref(e), None) == 0
    return s.value, e.value


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("backlog", (1, 3))
def test_bookkeeping_agrees_with_the_plan(lib, plan, backlog):
    """Seeded streams through PoolBook alone: pushes of every kind (nothing, one sample, less than a step, as much as fits),
    ticks in between.  At every point the steps run are those adn_stream_plan allows, a tick returns emitted(e(k)) - emitted(e(k - 1))
    samples, the room is never negative, and a closed stream ends with exactly `received` samples."""
    from audiodenoiser_amd.stream import PoolBook
    n_fft, hop, w, b, a = plan
    book = PoolBook(3, backlog, *plan)
    assert book.ring_samples == ring_min(*plan) + (backlog - 1) * b * hop
    assert book.out_stride == b * hop + n_fft // 2
    rng = np.random.default_rng(list(plan) + [backlog])
    lengths = [0, int(rng.integers(1, n_fft // 2)), book.end_of(2), book.end_of(1) + 1, 5 * b * hop + 77]
    for length in lengths:
        sid = book.open()
        assert sid == 0 and book.ready(sid) is None                       # the freed slot is reused
        out, ticks = 0, 0
        while book.received[sid] < length:
            room = book.room(sid)
            assert room >= 0
            with pytest.raises(RuntimeError, match=r"call step\(\)"):
                book.take(sid, room + 1)
            kind = int(rng.integers(0, 4))
            m = min((0, 1, int(rng.integers(1, b * hop)), room)[kind], room, length - book.received[sid])
            at = book.take(sid, m)
            assert at + m == book.received[sid]
            steps, emitted = _plan(lib, plan, book.received[sid])
            while rng.integers(0, 3) or book.room(sid) == 0:
                r = book.ready(sid)
                assert (r is not None) == (book.done[sid] < steps)
                if r is None:
                    break
                k, final = r
                assert k == book.done[sid] and final == -1
                n = book.count(k, final)
                assert n == _plan(lib, plan, book.end_of(k))[1] - _plan(lib, plan, book.end_of(k - 1))[1]
                assert 0 <= n <= book.out_stride
                out, ticks = out + n, ticks + 1
                assert not book.ran(sid)
            assert out == _plan(lib, plan, book.end_of(book.done[sid] - 1))[1] <= emitted
        done_at_close = book.done[sid]
        finished = book.close(sid)
        assert finished == (length == 0)
        with pytest.raises((RuntimeError, ValueError)):
            book.take(sid, 1)
        t_frames = 1 + length // hop
        k_last = -(-t_frames // b) if length else 0
        assert book.n_steps(length) == k_last >= done_at_close
        while not finished:
            k, final = book.ready(sid)
            assert final == length and k == book.done[sid] < k_last
            n = book.count(k, final)
            assert 0 <= n <= book.out_stride
            out += n
            finished = book.ran(sid)
            assert finished == (k == k_last - 1)
        assert out == length and book.rows() == []
        assert book.status[sid] == book.FREE


def test_rows_ascend_and_slots_fill_up():
    from audiodenoiser_amd.stream import PoolBook
    book = PoolBook(4, 1, 64, 16, 16, 1, 0)
    sids = [book.open() for _ in range(4)]
    assert sids == [0, 1, 2, 3]
    with pytest.raises(RuntimeError, match="taken"):
        book.open()
    for sid in (3, 1):
        book.take(sid, book.end_of(0))
    book.take(2, book.end_of(0) - 1)
    assert book.rows() == [(1, 0, -1), (3, 0, -1)]
    assert book.close(0) is True and book.open() == 0                    # an empty stream frees its slot at close
    assert book.close(2) is False
    assert book.rows() == [(1, 0, -1), (2, 0, book.end_of(0) - 1), (3, 0, -1)]
    with pytest.raises(ValueError, match="not an open stream"):
        book.room(7)
    for kw in (dict(max_streams=0), dict(backlog_steps=0), dict(n_fft=500), dict(hop_length=129), dict(window_frames=15),
               dict(block_frames=0), dict(lookahead_frames=-1), dict(window_frames=32, block_frames=24, lookahead_frames=9)):
        with pytest.raises(ValueError):
            PoolBook(**kw)
