"""The pool form of the echo canceller on the host (include/adn_call.h, libadn_call.so, audiodenoiser_amd.echo.EchoStreamPool): the
third library's symbol table, every refusal of adn_aec_stream_pool, and the argument errors of the Python face.  No test here needs
a device: every library call below is refused before a launch, on pointers that are never dereferenced.

The table of libadn_call.so is OPEN -- the next operator of a call goes into it -- so nothing here holds a count: the header, the
tuple in _lib and the library must name the same functions, whichever they are.
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_echo_host import ILLEGAL, WINDOW  # noqa: E402  (the illegal parameter values of adn_echo.h: one list)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = (64, 16, 16, 4, 0)
RING = 1024
F = 33
REC = 8 * 64 + 16 * 8                                        # bytes of a (slot, bin) record at the defaults
WHO = b"adn_aec_stream_pool:"


def _table(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split() and ln.split()[-2] in "TWVBDR"}


def test_the_call_library_exports_its_header_and_nothing_else():
    from audiodenoiser_amd import _lib
    C, E, M = _lib.load_call(), _lib.load_echo(), _lib.load()
    header = open(os.path.join(ROOT, "include", "adn_call.h")).read()
    declared = set(re.findall(r"\b(adn_[a-z0-9_]+)\s*\(", header))
    assert declared and declared == set(_lib.CALL_EXPORTED_SYMBOLS) and len(_lib.CALL_EXPORTED_SYMBOLS) == len(declared)
    assert _table(C) == declared
    for name in declared:
        assert re.search(rf"ADN_API [a-z *]+\b{name}\(", header) and hasattr(C, name), name
    # none of the other two tables' names, although their objects are linked in; and the other libraries have none of this one's
    assert not declared & set(_lib.ECHO_EXPORTED_SYMBOLS) and not declared & set(_lib.EXPORTED_SYMBOLS)
    for name in ("adn_aec_online", "adn_aec_stream", "adn_aec_stream_state_bytes", "adn_aec_last_error", "adn_last_error", "adn_version"):
        assert name not in _table(C), name
    assert not declared & _table(E) and not declared & _table(M)
    assert {"adn_call_last_error", "adn_aec_stream_pool"} <= declared
    # the version script names the functions one by one
    script = open(os.path.join(ROOT, "audiodenoiser_amd", "csrc", "libadn_call.map")).read()
    listed = set(re.findall(r"^\s*(adn_[a-z0-9_]+);", script.split("global:")[1].split("local:")[0], re.M))
    assert listed == declared
    # the two closed headers point here in prose and declare nothing of it
    for other in ("adn.h", "adn_echo.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "adn_call.h" in text and not re.search(r"adn_aec_stream_pool\s*\(", text), other
    assert "Not here:" in open(os.path.join(ROOT, "include", "adn_echo.h")).read()


class _Fake:
    """Aligned addresses inside one host buffer: never dereferenced, every call is refused before a launch."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(1 << 16)
        base = ctypes.addressof(self.buf) + (-ctypes.addressof(self.buf)) % 4096
        self.pstate, self.y, self.astate = base, base + 8192, base + 16384


def _rows(rows):
    from audiodenoiser_amd import _lib
    return (_lib.StreamPoolRow * len(rows))(*[_lib.StreamPoolRow(*r) for r in rows])


def _caller():
    from audiodenoiser_amd import _lib
    L, fake = _lib.load_call(), _Fake()
    pair = [(2, 0, -1), (3, 0, -1)]

    def call(rows=pair, n_rows=None, mics=1, n_slots=4, plan=PLAN, ring=RING, params=None, pstate=fake.pstate, pbytes=1 << 40,
             y=fake.y, astate=fake.astate, abytes=1 << 40):
        table = _rows(rows) if rows is not None else None
        n = n_rows if n_rows is not None else len(rows)
        return L.adn_aec_stream_pool(pstate, pbytes, n_slots, mics, *plan, ring, table, n, y, params, astate, abytes, None)

    return L, fake, call


def test_every_refusal_comes_before_a_launch_and_names_its_field():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.echo import AecParams
    L, fake, call = _caller()
    M, E = _lib.load(), _lib.load_echo()
    need = ctypes.c_size_t(0)
    M.adn_stream_state_bytes(0, 64, 16, 16, 4, 0, 2, ctypes.byref(need))            # a refusal of each other library ...
    E.adn_aec_stream_state_bytes(0, F, None, ctypes.byref(need))
    m_before, e_before = M.adn_last_error(), E.adn_aec_last_error()
    assert m_before.startswith(b"adn_stream_state_bytes") and e_before.startswith(b"adn_aec_stream_state_bytes:")
    assert M.adn_stream_pool_state_bytes(4, *PLAN, RING, ctypes.byref(need)) == 0
    pool_need = need.value
    two = [(0, 0, -1), (1, 0, -1), (2, 0, -1)]                                      # mics = 2: one call of three streams
    cases = (
        # the table: what adn_wpe_mc_stream_pool refuses with channels = mics + 1
        (dict(rows=[(0, 0, -1), (1, 0, -1), (2, 0, -1)]), b"n_rows", 1),             # an odd row count at mics = 1
        (dict(rows=two[:2], mics=2, n_slots=6), b"n_rows", 1),
        (dict(rows=[(3, 0, -1), (2, 0, -1)]), b"slot", 1),                           # microphone and far end swapped
        (dict(rows=[(1, 0, -1), (0, 0, -1)]), b"slot", 1),
        (dict(rows=[(1, 0, -1), (2, 0, -1)]), b"slot", 1),                           # two slots of two different calls
        (dict(rows=[(0, 0, -1), (2, 0, -1), (1, 0, -1)], mics=2, n_slots=6), b"order", 1),
        (dict(rows=[(2, 0, -1), (3, 1, -1)]), b"step", 1),                           # a call split over two steps
        (dict(rows=[(2, 3, 300), (3, 3, 301)]), b"final_length", 1),
        (dict(rows=[(2, 0, -1), (3, 0, -1), (2, 0, -1), (3, 0, -1)]), b"twice", 1),  # a call named twice
        (dict(rows=[(r, 0, -1) for r in range(257)], n_slots=258), b"n_rows", 1),    # 257 rows
        (dict(rows=[(r, 0, -1) for r in range(258)], n_slots=258), b"n_rows", 1),    # 129 whole calls: still too many
        (dict(rows=[], n_rows=0), b"n_rows", 1),
        (dict(rows=None, n_rows=2), b"null", 1),
        (dict(rows=[(4, 0, -1), (5, 0, -1)]), b"slot", 1),                           # a slot >= n_slots
        (dict(rows=[(-2, 0, -1), (-1, 0, -1)]), b"slot", 1),
        (dict(rows=[(0, 0, -1), (1, 0, -1)], n_slots=5), b"n_slots", 1),             # n_slots no multiple of mics + 1
        (dict(rows=two, mics=2, n_slots=4), b"n_slots", 1),
        (dict(rows=[(2, -1, -1), (3, -1, -1)]), b"step", 1),
        (dict(rows=[(2, 0, 0), (3, 0, 0)]), b"final_length", 1),
        (dict(rows=[(2, 9, 100), (3, 9, 100)]), b"step", 1),                         # past the last step of a finished call
        # the operator's own
        (dict(mics=0), b"mics", 1), (dict(mics=8, n_slots=9, rows=[(r, 0, -1) for r in range(9)]), b"mics", 1), (dict(mics=-1), b"mics", 1),
        (dict(plan=(64, 16, 16, 4, 1)), b"lookahead", 1),
        (dict(plan=(65, 16, 16, 4, 0)), b"n_fft", 1), (dict(ring=8), b"ring_samples", 1), (dict(n_slots=0), b"n_slots", 1),
        (dict(pstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(astate=None), b"null", 1),
        (dict(pstate=fake.pstate + 4), b"aligned", 1), (dict(y=fake.y + 2), b"aligned", 1), (dict(astate=fake.astate + 4), b"aligned", 1),
        (dict(pbytes=pool_need - 1), b"state", 3),
        (dict(abytes=2 * F * REC - 1), b"state", 3),                                 # a state one byte short: 4 slots / 2 * 1 = 2 pairs
        (dict(rows=two, mics=2, n_slots=6, abytes=4 * F * REC - 1), b"state", 3),    # 6 / 3 * 2 = 4 pairs
    )
    for kw, word, code in cases:
        rc = call(**kw)
        msg = L.adn_call_last_error()
        assert rc == code, (kw, rc, msg)
        assert msg.startswith(WHO) and word in msg, (kw, msg)
    # each illegal parameter, by the code that refuses it in front of adn_aec_stream
    for name, value in ILLEGAL:
        s = AecParams().to_struct()
        setattr(s, name, value)
        assert call(params=ctypes.byref(s)) == 1, (name, value)
        msg = L.adn_call_last_error()
        assert msg.startswith(WHO) and name.encode() in msg, (name, value, msg)
    for kw in WINDOW:
        s = AecParams().to_struct()
        s.taps, s.forget = kw["taps"], kw["forget"]
        assert call(params=ctypes.byref(s)) == 1, kw
        msg = L.adn_call_last_error()
        assert msg.startswith(WHO) and b"forget" in msg and b"taps" in msg, (kw, msg)
    # a larger record needs a larger state: K32-D8 against a state sized for the defaults
    s = AecParams(taps=32, delay=8, forget=0.984375).to_struct()
    assert call(params=ctypes.byref(s), abytes=2 * F * REC) == 3 and b"state" in L.adn_call_last_error()
    # ... and through all of it the other two libraries' messages stayed what they were
    assert M.adn_last_error() == m_before and E.adn_aec_last_error() == e_before


def test_the_python_face_refuses_before_it_looks_at_a_device():
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd import echo
    from audiodenoiser_amd.echo import AecParams, EchoStreamPool, aec_pool_state_bytes, aec_stream_state_bytes
    for name in ("EchoStreamPool", "aec_pool_state_bytes"):
        assert name in echo.__all__ and name in pkg.__all__ and getattr(pkg, name) is getattr(echo, name)
    for kw, word in ((dict(mics=0), "mics"), (dict(mics=8), "mics"), (dict(mics=True), "mics"), (dict(mics=2.0), "mics"),
                     (dict(max_calls=0), "max_calls"), (dict(max_calls="4"), "max_calls"), (dict(n_fft=100), "n_fft"),
                     (dict(hop_length=0), "hop"), (dict(block_frames=0), "block_frames"), (dict(backlog_steps=0), "backlog_steps"),
                     (dict(input_rates=(0,)), "input_rates")):
        with pytest.raises(ValueError, match=word):
            EchoStreamPool(**kw)
    with pytest.raises(TypeError, match="AecParams"):
        EchoStreamPool(params=dict(taps=4))
    with pytest.raises(TypeError, match="gain_params"):
        EchoStreamPool(gain=True, gain_params=dict())
    for max_calls, mics, params in ((1, 1, None), (16, 1, None), (5, 4, AecParams(taps=9, delay=2, forget=0.95)),
                                    (3, 7, AecParams(taps=32, delay=8, forget=0.984375))):
        assert aec_pool_state_bytes(max_calls, mics, F, params) == aec_stream_state_bytes(max_calls * mics, F, params)
    assert aec_pool_state_bytes(4, 2, 257) == 8 * 257 * REC
    for args, word in (((4, 0, F), "mics"), ((4, 8, F), "mics"), ((0, 1, F), "max_calls")):
        with pytest.raises(ValueError, match=word):
            aec_pool_state_bytes(*args)
    with pytest.raises(TypeError, match="AecParams"):
        aec_pool_state_bytes(1, 1, F, dict(taps=4))
