"""Recordings in the stream pools, on the host: the two entry points adn_wpe_mc_stream_pool and adn_mvdr_stream_pool (declared,
exported, loadable; every refusal include/adn.h lists for them, with its message) and the recording book of
audiodenoiser_amd/stream.py.  No test here needs a device: every call below is refused by the argument checks before the first
HIP call, so no pointer is followed (the buffers are host memory of the right size), and the book is plain Python.
"""
import ctypes
import os
import re

import pytest

from audiodenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("adn_wpe_mc_stream_pool", "adn_mvdr_stream_pool")
PLAN = dict(n_fft=64, hop=16, window=16, block=4, lookahead=0)
RING, F = 4096, 33
ORDER = ["pstate", "pbytes", "slots", "channels", *PLAN, "ring", "rows", "n_rows", "y", "params", "state", "state_bytes", "stream"]
INVALID, WORKSPACE = 1, 3                                # ADN_ERR_INVALID, ADN_ERR_WORKSPACE
FILL = 0x5A


# ---- the symbols ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_loadable():
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"ADN_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(ORDER), name
        assert re.search(r"^\s*adn_\*;", open(os.path.join(ROOT, "audiodenoiser_amd", "csrc", "libadn.map")).read(), re.M)
    assert int(re.search(r"The (\d+) functions below", header).group(1)) == len(_lib.EXPORTED_SYMBOLS) == 80
    for stale in ("Not here: the stream pool with multichannel streams", "look-ahead; an emit that skips the unused"):
        assert stale not in header
    def section(start, end):                                          # the comment's text, its line breaks and stars taken out
        return " ".join(header[header.index(start):header.index(end)].replace("\n *", " ").split())
    wpe = section("---- dereverb stream multichannel:", "ADN_API int adn_wpe_mc_stream_state_bytes")
    mvdr = section("---- beamform stream:", "ADN_API int adn_mvdr_stream_state_bytes")
    for phrase in ("adn_wpe_mc_stream_pool", "r C ... r C + C - 1", "n_slots / channels slots", "travels by value", "n_rows % channels != 0"):
        assert phrase in wpe, phrase
    for phrase in ("adn_mvdr_stream_pool", "FIRST row", "overlap-add tail", "nothing reads that tail but that slot's own later emits"):
        assert phrase in mvdr, phrase


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
class Host:
    """Host memory standing in for the device buffers of a call that is refused before it would touch them."""

    def __init__(self):
        self.mem = ctypes.create_string_buffer(bytes([FILL]) * (1 << 22), 1 << 22)
        base = (ctypes.addressof(self.mem) + 63) & ~63
        self.pstate, self.y, self.state = (base + i * (1 << 20) for i in range(3))

    def untouched(self):
        return self.mem.raw == bytes([FILL]) * (1 << 22)


def _size(fn, *args):
    need = ctypes.c_size_t(0)
    assert fn(*args, ctypes.byref(need)) == 0, _lib.load().adn_last_error()
    return need.value


def _rows(*r):
    return (_lib.StreamPoolRow * len(r))(*[_lib.StreamPoolRow(*x) for x in r])


def _table(channels, *recordings):
    """(recording, step, final_length) -> its C rows in channel order."""
    return [(r * channels + c, k, final) for r, k, final in recordings for c in range(channels)]


def _good(name, channels, host, plan=PLAN):
    L = _lib.load()
    slots = 3 * channels                                             # three recordings
    if name == "adn_wpe_mc_stream_pool":
        p = _lib.WpeStreamParamsStruct(2 if channels == 8 else 4, 3, 0.99, 300.0, 0.01, 0.9)
        need = _size(L.adn_wpe_mc_stream_state_bytes, 3, channels, F, ctypes.byref(p))
    else:
        p = _lib.MvdrStreamParamsStruct(channels - 1, 2, 0.99, 1e-3, 1e-3)
        need = _size(L.adn_mvdr_stream_state_bytes, 3, channels, F, ctypes.byref(p))
    pbytes = _size(L.adn_stream_pool_state_bytes, slots, *plan.values(), RING)
    assert pbytes <= 1 << 20 and need <= 1 << 20
    return dict(pstate=host.pstate, pbytes=pbytes, slots=slots, channels=channels, **plan, ring=RING,
                rows=_table(channels, (2, 1, -1), (0, 0, -1)), n_rows=2 * channels, y=host.y, params=p, state=host.state,
                state_bytes=need, stream=None)


def _call(name, args):
    L = _lib.load()
    vals = dict(args)
    vals["rows"] = _rows(*vals["rows"]) if vals["rows"] is not None else None
    vals["params"] = ctypes.byref(vals["params"]) if vals["params"] is not None else None
    rc = getattr(L, name)(*[vals[k] for k in ORDER])
    return rc, L.adn_last_error().decode()


def _refused(name, host, args, code, text):
    rc, msg = _call(name, args)
    assert rc == code, (name, text, rc, msg)
    assert msg.startswith(name + ": ") and text in msg, (name, text, msg)
    assert host.untouched(), (name, text)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("channels", (2, 3, 8))
def test_what_the_pool_call_and_the_lockstep_call_refuse(name, channels):
    host = Host()
    good = _good(name, channels, host)
    state_word = "WPE" if name == "adn_wpe_mc_stream_pool" else "MVDR"
    sizer = "adn_wpe_mc_stream_state_bytes" if name == "adn_wpe_mc_stream_pool" else "adn_mvdr_stream_state_bytes"
    ahead = dict(PLAN, lookahead=1)
    for change, code, text in (
            (dict(pstate=None), INVALID, "null pointer"),
            (dict(slots=0), INVALID, "1 <= n_slots <= 2^20"),
            (dict(n_fft=48), INVALID, "power-of-two n_fft"),
            (dict(ring=1), INVALID, "<= ring_samples <= 2^28"),
            (dict(pbytes=good["pbytes"] - 1), WORKSPACE, "state smaller than adn_stream_pool_state_bytes"),
            (dict(pstate=host.pstate + 4), INVALID, "state must be 8-byte aligned"),
            (dict(lookahead=1, pbytes=_size(_lib.load().adn_stream_pool_state_bytes, good["slots"], *ahead.values(), RING)), INVALID,
             "the operator is causal: lookahead must be 0"),
            (dict(y=None), INVALID, "null pointer"),
            (dict(y=host.y + 2), INVALID, "y must be 4-byte aligned"),
            (dict(rows=None), INVALID, "null pointer"),
            (dict(n_rows=0), INVALID, "1 <= n_rows <= ADN_STREAM_POOL_MAX_ROWS"),
            (dict(rows=_table(channels, *[(r % 3, 0, -1) for r in range(-(-257 // channels))])[:257], n_rows=257), INVALID,
             "1 <= n_rows <= ADN_STREAM_POOL_MAX_ROWS"),
            (dict(rows=_table(channels, (3, 1, -1), (0, 0, -1))), INVALID, "a row's slot is outside [0, n_slots)"),
            (dict(rows=_table(channels, (1, 0, -1), (1, 0, -1))), INVALID, "a slot is named twice in one call"),
            (dict(rows=_table(channels, (2, -1, -1), (0, 0, -1))), INVALID, "first_step >= 0"),
            (dict(rows=_table(channels, (2, 1, 0), (0, 0, -1))), INVALID, "final_length must be -1"),
            (dict(channels=0), INVALID, "need 1 <= channels <= 8"),
            (dict(channels=9), INVALID, "need 1 <= channels <= 8"),
            (dict(state=None), INVALID, f"null pointer (the {state_word} state)"),
            (dict(state_bytes=good["state_bytes"] - 1), WORKSPACE, f"the {state_word} state is smaller than {sizer}"),
            (dict(state=host.state + 4), INVALID, f"the {state_word} state must be 8-byte aligned")):
        _refused(name, host, {**good, **change}, code, text)


@pytest.mark.parametrize("channels", (2, 3, 8))
def test_the_parameter_rules_of_the_two_operators(channels):
    host = Host()
    name = "adn_wpe_mc_stream_pool"
    good = _good(name, channels, host)
    W = _lib.WpeStreamParamsStruct
    k = good["params"].taps
    for p, text in ((W(0, 3, 0.99, 300.0, 0.01, 0.9), "need 1 <= taps <= 32"), (W(k, 9, 0.99, 300.0, 0.01, 0.9), "need 1 <= delay <= 8"),
                    (W(k, 3, float("nan"), 300.0, 0.01, 0.9), "need 0.95 <= forget <= 1"), (W(k, 3, 0.99, 0.5, 0.01, 0.9), "need 1 <= loading <= 1e6"),
                    (W(k, 3, 0.99, 300.0, 0.0, 0.9), "need 0 < power_floor <= 1"), (W(k, 3, 0.99, 300.0, 0.01, 1.0), "need 0 <= smooth < 1"),
                    (W(32 // channels + 1, 3, 0.99, 300.0, 0.01, 0.9), "need channels * taps <= 32"),
                    (W(32 // channels, 3, 0.98, 300.0, 0.01, 0.9), "need 2 channels taps (1 - forget) <= 1")):
        _refused(name, host, {**good, "params": p}, INVALID, text)
    # params = NULL is taps = 32 // channels: a state one byte below ITS size is refused, the state of that size is what it wants
    L = _lib.load()
    default = _size(L.adn_wpe_mc_stream_state_bytes, 3, channels, F, None)
    assert default == _size(L.adn_wpe_mc_stream_state_bytes, 3, channels, F, ctypes.byref(W(32 // channels, 3, 0.99, 300.0, 0.01, 0.9)))
    _refused(name, host, {**good, "params": None, "state_bytes": default - 1}, WORKSPACE, "the WPE state is smaller than")
    name = "adn_mvdr_stream_pool"
    good = _good(name, channels, host)
    M = _lib.MvdrStreamParamsStruct
    for p, text in ((M(channels, 1, 0.99, 1e-3, 1e-3), "ref_channel"), (M(0, 0, 0.99, 1e-3, 1e-3), "need 1 <= refresh <= 64"),
                    (M(0, 65, 0.99, 1e-3, 1e-3), "need 1 <= refresh <= 64"), (M(0, 1, 0.89, 1e-3, 1e-3), "need 0.9 <= forget <= 1"),
                    (M(0, 1, float("nan"), 1e-3, 1e-3), "need 0.9 <= forget <= 1"), (M(0, 1, 0.99, 2.0, 1e-3), "loading"),
                    (M(0, 1, 0.99, 1e-3, 0.3), "mask_floor")):
        _refused(name, host, {**good, "params": p}, INVALID, text)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("channels", (2, 3, 8))
def test_the_rules_of_a_recording(name, channels):
    host = Host()
    good = _good(name, channels, host)
    L = _lib.load()
    C = channels
    more = _size(L.adn_stream_pool_state_bytes, good["slots"] + 1, *PLAN.values(), RING)
    shifted = [(1 + c, 0, -1) for c in range(C)]                           # C consecutive slots that start inside recording 0
    order = [(2 * C + c, 1, -1) for c in range(C)]
    order[-1], order[-2] = order[-2], order[-1]                            # the right slots, the last two channels swapped
    if C == 2:                                                             # (5, 4): the first slot is the second channel's
        order_text = "a group's first slot must be a multiple of channels"
    else:
        order_text = "a group's slots must be consecutive, in channel order"
    gap = [(0, 0, -1)] + [(C + c, 0, -1) for c in range(1, C)]             # channel 0 of recording 0, the rest of recording 1
    step = [(c, 1 if c == C - 1 else 0, -1) for c in range(C)]
    final = [(c, 0, 40 if c == C - 1 else -1) for c in range(C)]
    for change, text in (
            (dict(slots=good["slots"] + 1, pbytes=more), "n_slots must be a multiple of channels"),
            (dict(n_rows=2 * C - 1), "n_rows must be a multiple of channels"),
            (dict(rows=shifted, n_rows=C), "a group's first slot must be a multiple of channels"),
            (dict(rows=order, n_rows=C), order_text),
            (dict(rows=gap, n_rows=C), "a group's slots must be consecutive, in channel order"),
            (dict(rows=good["rows"][:C] + step, n_rows=2 * C), "the rows of a group must agree in step and final_length"),
            (dict(rows=final, n_rows=C), "the rows of a group must agree in step and final_length")):
        _refused(name, host, {**good, **change}, INVALID, text)


def test_one_channel_is_the_single_channel_pool_call_on_the_host_too():
    """channels = 1: every row is a recording, so none of the group rules can fire; what is refused is what adn_wpe_stream_pool
    refuses, under the new name."""
    host = Host()
    good = _good("adn_wpe_mc_stream_pool", 1, host)
    L = _lib.load()
    assert good["state_bytes"] == _size(L.adn_wpe_stream_state_bytes, 3, F, ctypes.byref(good["params"]))
    _refused("adn_wpe_mc_stream_pool", host, {**good, "rows": [(1, 0, -1), (1, 1, -1)]}, INVALID, "a slot is named twice in one call")
    _refused("adn_wpe_mc_stream_pool", host, {**good, "state_bytes": good["state_bytes"] - 1}, WORKSPACE, "the WPE state is smaller than")


# ---- the recording book --------------------------------------------------------------------------------------------------------------
def _book(max_recordings, channels, **kw):
    from audiodenoiser_amd.stream import RecordingBook
    return RecordingBook(max_recordings, channels, n_fft=64, hop_length=16, window_frames=16, block_frames=4, **kw)


def test_rows_expand_in_channel_order_and_a_tick_is_cut_into_whole_recordings():
    from audiodenoiser_amd.stream import POOL_MAX_ROWS, PoolBook
    book = _book(40, 8)
    assert isinstance(book, PoolBook) and book.channels == 8 and book.n_slots == 320 and book.max_streams == 40
    assert list(book.slots(3)) == list(range(24, 32))
    assert book.stream_rows([(2, 5, -1), (0, 7, 900)]) == [(16 + c, 5, -1) for c in range(8)] + [(c, 7, 900) for c in range(8)]
    rids = [book.open() for _ in range(33)]
    assert rids == list(range(33))
    for rid in rids:
        book.take(rid, book.end_of(0))
    rows = book.rows()
    assert rows == [(rid, 0, -1) for rid in rids]
    calls = book.calls(rows)
    assert [len(c) for c in calls] == [32, 1] and sum(calls, []) == rows                # 33 recordings of 8 channels: 32 + 1
    for call in calls:
        srows = book.stream_rows(call)
        assert len(srows) <= POOL_MAX_ROWS and len(srows) % 8 == 0
        for i in range(0, len(srows), 8):                                          # what the library demands of a group
            group = srows[i:i + 8]
            assert group[0][0] % 8 == 0 and [r[0] for r in group] == list(range(group[0][0], group[0][0] + 8))
            assert len({r[1:] for r in group}) == 1
    assert [len(c) for c in _book(200, 3).calls([(r, 0, -1) for r in range(200)])] == [85, 85, 30]       # 256 // 3 = 85
    assert [len(c) for c in _book(4, 1).calls([(r, 0, -1) for r in range(4)])] == [4]


def test_room_close_and_slot_reuse_act_per_recording():
    book = _book(2, 4, backlog_steps=2)
    a, b = book.open(), book.open()
    assert (a, b) == (0, 1)
    with pytest.raises(RuntimeError):
        book.open()                                                                 # two recordings, not eight streams
    room = book.room(a)
    assert room == book.ring_samples == 48 + book.end_of(0) + 2 * 64
    assert book.take(a, 70) == 0 and book.room(a) == room - 70 and book.room(b) == room
    with pytest.raises(RuntimeError):
        book.take(a, room)                                                          # beyond the room: nothing is booked
    assert book.received[a] == 70 and book.ready(a) is None
    assert book.take(a, 90) == 70
    assert book.ready(a) == (0, -1) and book.rows() == [(a, 0, -1)]
    assert book.stream_rows(book.rows()) == [(c, 0, -1) for c in range(4)]
    assert not book.ran(a) and book.done[a] == 1
    assert not book.close(a)                                                        # 160 samples: 11 frames, three steps
    assert book.n_steps(160) == 3 and book.rows() == [(a, 1, 160)]
    assert not book.ran(a) and book.ran(a)                                          # the last step frees the recording
    assert book.close(b)                                                            # a recording of no samples is free at once
    c = book.open()
    assert c == a and book.received[c] == 0 and book.done[c] == 0                   # the same four slots, no reset
    assert list(book.slots(c)) == [0, 1, 2, 3]


def test_a_recording_at_a_rate_is_booked_once():
    book = _book(3, 2, input_rates=(48000,))
    rid = book.open(48000)
    assert book.rate[rid] == 48000
    call, before = book.take_rate(rid, 1200)
    assert (call, before) == (0, 0) and book.received_in[rid] == 1200 and 0 < book.received[rid] <= 200
    assert book.take_rate(rid, 600) == (1, 1200)


def test_what_the_book_and_the_classes_refuse():
    from audiodenoiser_amd.stream import RecordingBook
    for channels in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="channels"):
            RecordingBook(4, channels)
    with pytest.raises(ValueError, match="max_recordings"):
        RecordingBook((1 << 20) // 8 + 1, 8)
    with pytest.raises(ValueError, match="max_recordings"):
        RecordingBook(0, 2)
    from audiodenoiser_amd.beamform import BeamformStreamPool, MvdrStreamParams
    from audiodenoiser_amd.dereverb import DereverbStreamPool, WpeStreamParams
    with pytest.raises(ValueError, match="ref_channel"):
        BeamformStreamPool(None, 4, 2, params=MvdrStreamParams(ref_channel=2))
    with pytest.raises(ValueError, match="channels"):
        BeamformStreamPool(None, 4, 9)
    with pytest.raises(TypeError, match="wpe_params"):
        BeamformStreamPool(None, 4, 2, wpe=True, wpe_params=object())
    with pytest.raises(ValueError, match="channels"):
        DereverbStreamPool(None, 4, channels=0)
    with pytest.raises(ValueError):
        DereverbStreamPool(None, 4, channels=4, params=WpeStreamParams(taps=9))     # 4 x 9 > 32
