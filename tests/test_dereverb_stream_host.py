"""Streaming dereverberation without a device: the restatement's own properties (tests/dereverb_stream_ref.py), the Python face
(audiodenoiser_amd/dereverb.py) and the argument checks of adn_wpe_stream_state_bytes / adn_wpe_online / adn_wpe_stream /
adn_wpe_stream_pool, which refuse before anything is launched.
Measured on the host (python tests/dereverb_stream_cases.py; profiles/bench_dereverb_stream.md has the table): the batch identity
holds to 7.8e-16 (alpha 1) and 2.4e-15 (alpha 0.98) at T = 40, K = 6; the float32 restatement stays finite over 3750 frames at the
defaults, at (forget 0.95, K 32, D 1) and at forget 1.0, its per-quarter error 1.6e-6 ... 4.4e-6, 4.3e-5 ... 8.5e-5 and
1.9e-7 ... 6e-7 of the maximum, growing 1.79 x, 1.49 x and 1.09 x from the second quarter to the fourth (allowed: 4), so no legal
range was narrowed; SI-SDR of the quality clip 3.33 dB in, 5.27 dB out (7.65 dB with the gain, offline WPE 6.54 dB)."""
import ctypes
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_stream_cases as sc  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ILLEGAL = (("taps", 0), ("taps", 33), ("taps", -1), ("delay", 0), ("delay", 9), ("forget", 0.94), ("forget", 1.001), ("forget", 0.0),
           ("forget", float("nan")), ("loading", 0.5), ("loading", 0.0), ("loading", 2e6), ("loading", float("nan")),
           ("loading", float("inf")), ("power_floor", 0.0), ("power_floor", -1e-3), ("power_floor", 1.01), ("power_floor", float("nan")),
           ("smooth", -0.1), ("smooth", 1.0), ("smooth", float("nan")))
LEGAL = (("taps", 1), ("taps", 32), ("delay", 1), ("delay", 8), ("forget", 0.95), ("forget", 1.0), ("loading", 1.0), ("loading", 1e6),
         ("power_floor", 1.0), ("power_floor", 1e-12), ("smooth", 0.0), ("smooth", 0.999))


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)


# ---- the Python face and the C ABI -----------------------------------------------------------------------------------------------
def test_params_refuse_every_out_of_range_value_and_nan():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeStreamParams
    p = WpeStreamParams()
    assert dataclasses.asdict(p) == ds.DEFAULTS and tuple(f.name for f in dataclasses.fields(p)) == ds.FIELDS
    s = p.to_struct()
    assert isinstance(s, _lib.WpeStreamParamsStruct) and ctypes.sizeof(s) == 24 and [n for n, _ in s._fields_] == list(ds.FIELDS)
    assert (s.taps, s.delay) == (20, 3) and s.forget == np.float32(0.99) and s.loading == 300.0
    assert s.power_floor == np.float32(0.01) and s.smooth == np.float32(0.9)
    for name, value in ILLEGAL:
        with pytest.raises(ValueError, match=name):
            WpeStreamParams(**{name: value})
        with pytest.raises(ValueError, match=name):
            ds.check_params({**ds.DEFAULTS, name: value})
    for name, value in (("taps", 2.0), ("delay", True), ("taps", "3")):
        with pytest.raises(ValueError, match=name):
            WpeStreamParams(**{name: value})
    for name, value in LEGAL:
        WpeStreamParams(**{name: value})
        ds.check_params({**ds.DEFAULTS, name: value})


def test_python_defaults_equal_the_headers_and_the_pointer_replaces_the_gap():
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    m = re.search(r"taps K (\d+), delay D (\d+), forget alpha ([\d.]+), loading delta ([\d.]+),\s*\*?\s*power_floor rho ([\d.]+), "
                  r"smooth beta ([\d.]+)\.", header)
    assert m, "the defaults sentence of the dereverb stream section"
    assert [float(v) for v in m.groups()] == [float(ds.DEFAULTS[k]) for k in ds.FIELDS]
    assert re.search(r"typedef struct adn_wpe_stream_params \{ int taps, delay; float forget, loading, power_floor, smooth; \} "
                     r"adn_wpe_stream_params;", header)
    api = open(os.path.join(ROOT, "audiodenoiser_amd", "csrc", "adn_api.hip")).read()
    m = re.search(r"adn_wpe_stream_params defaults = \{([^}]*)\}", api)
    assert [float(v.strip().rstrip("f")) for v in m.group(1).split(",")] == [float(ds.DEFAULTS[k]) for k in ds.FIELDS]
    # the section states that it has no counterpart and is unpinned, and the three "not here" sentences now point at it
    section = header[header.index("---- dereverb stream:"):]
    section = section[:section.index("typedef struct adn_wpe_stream_params")]
    for phrase in ("No reference counterpart", "UNPINNED", "Hermitian update is part of the DEFINITION", "STARTS FRESH"):
        assert phrase in section, phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    module = open(os.path.join(ROOT, "audiodenoiser_amd", "dereverb.py")).read()
    for text in (header, readme, module):
        assert not re.search(r"(NOT|Not) here:\s+online / recursive WPE", text)
        assert "dereverb stream" in text
    from audiodenoiser_amd import StreamDenoiser, StreamPool, dereverb
    import audiodenoiser_amd as pkg
    assert issubclass(dereverb.StreamDereverberator, StreamDenoiser) and issubclass(dereverb.DereverbStreamPool, StreamPool)
    for name in ("WpeStreamParams", "wpe_online", "StreamDereverberator", "DereverbStreamPool"):
        assert getattr(pkg, name) is getattr(dereverb, name) and name in pkg.__all__ and name in dereverb.__all__
    for cls in (dereverb.StreamDereverberator, dereverb.DereverbStreamPool):
        assert {k for k, v in vars(cls).items() if callable(v)} == {"__init__", "reset", "network", "_net"}


def test_symbols_are_declared_exported_and_loadable():
    from audiodenoiser_amd import _lib
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    L = _lib.load()
    for name in ("adn_wpe_stream_state_bytes", "adn_wpe_online", "adn_wpe_stream", "adn_wpe_stream_pool"):
        assert re.search(r"ADN_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name


def _state_bytes(L, n_slots, n_bins, params=None, bytes_=True):
    need = ctypes.c_size_t(12345)
    return L.adn_wpe_stream_state_bytes(n_slots, n_bins, params, ctypes.byref(need) if bytes_ else None), need.value


def test_state_bytes_is_monotone_in_slots_bins_and_taps():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeStreamParams, wpe_stream_state_bytes
    L = _lib.load()
    rc, base = _state_bytes(L, 1, 257)
    assert rc == 0 and base >= 257 * 4 * (2 * 20 + 2 * 20 * 21 // 2 + 1 + 2 * 22)           # g, a triangle of P, s, D + K - 1 frames
    assert base % 8 == 0 and base == wpe_stream_state_bytes(1, 257)
    last = 0
    for taps in range(1, 33):
        need = wpe_stream_state_bytes(3, 33, WpeStreamParams(taps=taps))
        assert need > last
        last = need
    for delay in range(1, 8):
        assert wpe_stream_state_bytes(1, 33, WpeStreamParams(delay=delay + 1)) >= wpe_stream_state_bytes(1, 33, WpeStreamParams(delay=delay))
    assert [wpe_stream_state_bytes(n, 257) for n in (1, 2, 3, 64)] == [base * n for n in (1, 2, 3, 64)]
    sizes = [wpe_stream_state_bytes(2, f) for f in (1, 33, 257, 2049)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    for kw, word in ((dict(bytes_=False), b"null"), (dict(n_slots=0), b"n_slots"), (dict(n_bins=0), b"n_bins"), (dict(n_slots=-1), b"n_slots")):
        args = dict(n_slots=1, n_bins=8)
        args.update(kw)
        rc, need = _state_bytes(L, **args)
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_stream_state_bytes:") and word in msg, (kw, msg)


def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeStreamParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)               # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    q, st, mg = p + 4096, p + 8192, p + 16384
    big = 1 << 40                                            # "bytes" of the state: no call gets as far as touching it

    def online(params=None, spec=p, n=1, t=4, f=8, first=0, state=st, state_bytes=big, slots=1, out=q, mag=mg, width=4, col0=0):
        return L.adn_wpe_online(spec, n, t, f, first, params, state, state_bytes, slots, out, mag, width, col0, None)

    plan = (512, 128, 16, 4, 0)

    def stream(params=None, sstate=p, sbytes=big, y=q, n=1, first=0, steps=1, final=-1, plan=plan, max_steps=4, wstate=st, wbytes=big):
        return L.adn_wpe_stream(sstate, sbytes, y, n, first, steps, final, *plan, max_steps, params, wstate, wbytes, None)

    ring = 8192
    rows1 = (_lib.StreamPoolRow * 1)(_lib.StreamPoolRow(0, 0, -1))

    def pool(params=None, pstate=p, pbytes=big, slots=4, plan=plan, ring=ring, rows=rows1, n_rows=1, y=q, wstate=st, wbytes=big):
        return L.adn_wpe_stream_pool(pstate, pbytes, slots, *plan, ring, rows, n_rows, y, params, wstate, wbytes, None)

    for name, value in ILLEGAL:
        s = WpeStreamParams().to_struct()
        setattr(s, name, value)
        for call, who in ((online, b"adn_wpe_online:"), (stream, b"adn_wpe_stream:"), (pool, b"adn_wpe_stream_pool:")):
            assert call(ctypes.byref(s)) == 1, (name, value, who)
            msg = L.adn_last_error()
            assert msg.startswith(who) and name.encode() in msg, (name, value, msg)
        rc, need = _state_bytes(L, 1, 8, ctypes.byref(s))
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_stream_state_bytes:") and name.encode() in msg, (name, value, msg)
    for name, value in LEGAL:
        s = WpeStreamParams(**{name: value}).to_struct()
        assert _state_bytes(L, 1, 8, ctypes.byref(s))[0] == 0, (name, value)

    need = _state_bytes(L, 1, 8)[1]
    for kw, word, status in ((dict(spec=None), b"null", 1), (dict(out=None), b"null", 1), (dict(state=None), b"null", 1),
                             (dict(n=0), b"n_rows", 1), (dict(t=0), b"n_frames", 1), (dict(f=0), b"n_bins", 1), (dict(n=-1), b"n_rows", 1),
                             (dict(first=-1), b"first_frame", 1), (dict(first=(1 << 31) - 2), b"first_frame", 1),
                             (dict(slots=0), b"n_slots", 1), (dict(n=2, slots=1, state_bytes=big), b"n_slots", 1),
                             (dict(width=3), b"width", 1), (dict(col0=1), b"col0", 1), (dict(col0=-1, width=9), b"col0", 1),
                             (dict(spec=p + 4), b"aligned", 1), (dict(out=q + 4), b"aligned", 1), (dict(mag=mg + 2), b"aligned", 1),
                             (dict(state=st + 4), b"aligned", 1), (dict(out=p), b"overlap", 1), (dict(out=p + 8 * 8 * 3), b"overlap", 1),
                             (dict(state_bytes=need - 1), b"adn_wpe_stream_state_bytes", 3), (dict(state_bytes=0), b"state", 3)):
        assert online(**kw) == status, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_online:") and word in msg, (kw, msg)

    sbytes = ctypes.c_size_t()
    assert L.adn_stream_state_bytes(1, *plan, 4, ctypes.byref(sbytes)) == 0
    wneed = _state_bytes(L, 1, 257)[1]
    for kw, word, status in ((dict(sstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(wstate=None), b"null", 1),
                             (dict(plan=(512, 128, 16, 4, 1)), b"lookahead", 1), (dict(plan=(500, 128, 16, 4, 0)), b"n_fft", 1),
                             (dict(n=0), b"n_streams", 1), (dict(first=-1), b"first_step", 1), (dict(steps=0), b"n_steps", 1),
                             (dict(steps=5), b"max_steps", 1), (dict(final=0), b"final_length", 1), (dict(y=q + 2), b"aligned", 1),
                             (dict(wstate=st + 4), b"aligned", 1), (dict(sstate=p + 4), b"aligned", 1),
                             (dict(final=1000, first=9), b"past the last step", 1),
                             (dict(sbytes=sbytes.value - 1), b"adn_stream_state_bytes", 3), (dict(wbytes=wneed - 1), b"adn_wpe_stream_state_bytes", 3)):
        assert stream(**kw) == status, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_stream:") and word in msg, (kw, msg)

    pbytes = ctypes.c_size_t()
    assert L.adn_stream_pool_state_bytes(4, *plan, ring, ctypes.byref(pbytes)) == 0
    twice = (_lib.StreamPoolRow * 2)(_lib.StreamPoolRow(1, 0, -1), _lib.StreamPoolRow(1, 3, -1))
    outside = (_lib.StreamPoolRow * 1)(_lib.StreamPoolRow(4, 0, -1))
    many = (_lib.StreamPoolRow * 257)(*[_lib.StreamPoolRow(i, 0, -1) for i in range(257)])
    for kw, word, status in ((dict(pstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(wstate=None), b"null", 1), (dict(rows=None), b"null", 1),
                             (dict(plan=(512, 128, 16, 4, 2)), b"lookahead", 1), (dict(n_rows=0), b"n_rows", 1),
                             (dict(rows=many, n_rows=257, slots=300), b"ADN_STREAM_POOL_MAX_ROWS", 1), (dict(rows=twice, n_rows=2), b"twice", 1),
                             (dict(rows=outside), b"outside", 1), (dict(y=q + 2), b"aligned", 1), (dict(wstate=st + 4), b"aligned", 1),
                             (dict(ring=100), b"ring_samples", 1), (dict(pbytes=pbytes.value - 1), b"adn_stream_pool_state_bytes", 3),
                             (dict(wbytes=4 * wneed - 1), b"adn_wpe_stream_state_bytes", 3)):
        assert pool(**kw) == status, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_stream_pool:") and word in msg, (kw, msg)


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (1.0, 0.98))
def test_the_recursion_is_exact_rls(alpha):
    """With the lam_t it produced, g_T solves (alpha^T delta I + sum alpha^(T-1-t) x~ x~^H / lam_t) g = sum alpha^(T-1-t) x~ conj(X_t) / lam_t;
    at alpha = 1 that is the growing-window solution.  delta here is 1 / P_0, and P_0 is the fp32 value of 1 / loading (the header)."""
    T, F, K, D = 40, 3, 6, 2
    x = _noise((T, F), 3)
    d, state, lam = ds.wpe_online(x, dict(taps=K, delay=D, forget=alpha), with_state=True, with_lam=True)
    a = float(np.float32(alpha))
    delta = 1.0 / float(np.float32(1.0) / np.float32(ds.DEFAULTS["loading"]))
    worst = 0.0
    for f in range(F):
        A, b = (a ** T) * delta * np.eye(K, dtype=complex), np.zeros(K, complex)
        for t in range(T):
            xt = np.array([x[t - D - j, f] if t - D - j >= 0 else 0.0 for j in range(K)])
            w = a ** (T - 1 - t) / lam[t, f]
            A += w * np.outer(xt, xt.conj())
            b += w * xt * np.conj(x[t, f])
        g = np.linalg.solve(A, b)
        worst = max(worst, float(np.abs(g - state["g"][f]).max() / np.abs(g).max()))
        # and d_t is the a-priori error: with the taps BEFORE frame t -- checked for the last frame through a run one frame shorter
    print(f"alpha {alpha}: max |g - g_batch| / max |g_batch| = {worst:.3g} (bound 1e-9)")
    assert worst <= 1e-9
    _, before = ds.wpe_online(x[:-1], dict(taps=K, delay=D, forget=alpha), with_state=True)
    xt = np.stack([x[T - 1 - D - j] for j in range(K)], axis=1)
    assert np.allclose(d[-1], x[-1] - np.einsum("fj,fj->f", np.conj(before["g"]), xt), rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_the_first_frames_pass_through_exactly_and_a_zero_row_gives_zeros(dtype):
    ct = np.complex64 if dtype is np.float32 else np.complex128
    x = _noise((60, 9), 5).astype(np.complex64)
    for delay in (1, 3, 8):
        d = ds.wpe_online(x, dict(delay=delay), dtype=dtype)
        assert d.dtype == ct and np.array_equal(d[:delay], x[:delay].astype(ct)) and not np.array_equal(d[delay:], x[delay:].astype(ct))
    for n_frames in (1, 2, 3):
        assert np.array_equal(ds.wpe_online(x[:n_frames], dtype=dtype), x[:n_frames].astype(ct))
    z = x.copy()
    z[:, 3] = 0
    d = ds.wpe_online(z, dtype=dtype)
    assert np.all(d[:, 3] == 0) and np.isfinite(d).all()
    assert np.all(ds.wpe_online(np.zeros((40, 5), np.complex64), dtype=dtype) == 0)


def test_a_row_is_independent_of_its_neighbours_and_a_nan_stays_in_its_row():
    x = _noise((70, 12), 7).astype(np.complex64)
    for dtype in (np.float32, np.float64):
        whole = ds.wpe_online(x, dtype=dtype)
        assert np.array_equal(ds.wpe_online(x[:, 4:7], dtype=dtype), whole[:, 4:7])
        bad = x.copy()
        bad[20, 5] = np.nan
        got = ds.wpe_online(bad, dtype=dtype)
        keep = np.arange(12) != 5
        assert np.array_equal(got[:, keep], whole[:, keep])
        assert np.array_equal(got[:20, 5], whole[:20, 5]) and np.isnan(got[20:, 5]).all()      # poisoned from that frame on


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_cutting_the_frames_into_calls_changes_nothing(dtype):
    x = _noise((50, 6), 8).astype(np.complex64)
    for kw in (None, dict(taps=32, delay=8, forget=0.95), dict(taps=1, delay=1)):
        whole = ds.wpe_online(x, kw, dtype=dtype)
        for cuts in ((1,) * 50, (4,) * 12 + (2,), (7, 1, 30, 12)):
            parts, state, at = [], None, 0
            for n in cuts:
                d, state = ds.wpe_online(x[at:at + n], kw, dtype=dtype, state=state, first_frame=at, with_state=True)
                parts.append(d)
                at += n
            assert at == 50 and np.array_equal(np.concatenate(parts), whole), (kw, cuts)
        # a call at frame 0 ignores the state it is given
        _, state = ds.wpe_online(x, kw, dtype=dtype, with_state=True)
        assert np.array_equal(ds.wpe_online(x, kw, dtype=dtype, state=state, first_frame=0), whole)


@pytest.mark.parametrize("index", range(len(sc.LONG_PARAMS)), ids=sc.LONG_IDS)
def test_float32_stays_finite_and_bounded_over_3750_frames(index):
    """The defaults and the corners of the legal ranges: finite, and the per-quarter error does not grow by more than 4 x from the
    second quarter to the fourth.  A corner that failed would narrow the legal range, not this test."""
    finite, q = sc.long_run(index)
    print(f"{sc.LONG_IDS[index]}: finite {finite}, max|d32 - d64| / max|d64| per quarter " + ", ".join(f"{v:.3g}" for v in q)
          + f"; Q4 / Q2 = {q[3] / q[1]:.2f} (bound 4)")
    assert sc.long_spec().shape == (3750, len(sc.LONG_BINS))
    assert finite
    assert q[3] <= 4.0 * q[1]


def test_float32_is_carried_out_in_float32_and_the_floors_are_recorded():
    """FLOOR and FLOOR_AUDIO are what `python tests/dereverb_stream_cases.py` measured; here some of its cases stay under them."""
    import denoise_ref
    assert 0 < ds.FLOOR < 1e-3 and 0 < ds.FLOOR_AUDIO < 1e-3
    spec = _noise((40, 5), 9).astype(np.complex64)
    d32 = ds.wpe_online(spec, dtype=np.float32)
    assert d32.dtype == np.complex64 and not np.array_equal(d32, ds.wpe_online(spec).astype(np.complex64))
    for n_fft, n_frames, params in ((64, 23, None), (64, 97, sc.PARITY_PARAMS[2]), (512, 40, sc.PARITY_PARAMS[1])):
        x = sc.parity_audio(n_fft, n_frames)[1]
        f = sc.floor_of(denoise_ref.stft(x, n_fft, n_fft // 4).astype(np.complex64), params)
        print(f"n_fft {n_fft} T {n_frames} {params}: {f:.3g} (FLOOR {ds.FLOOR:.3g})")
        assert f <= ds.FLOOR * 1.05                              # FLOOR is written with two digits
    x = sc.parity_audio(64, sc.E2E_FRAMES)[0]
    a64 = sc.e2e_want(64, True, 0)
    a32 = ds.stream_dereverb(x, 64, 16, gain=True, dtype=np.float32)
    f = float(np.abs(a32 - a64).max() / np.abs(a64).max())
    print(f"end to end n_fft 64 with the gain, row 0: {f:.3g} (FLOOR_AUDIO {ds.FLOOR_AUDIO:.3g})")
    assert a32.dtype == np.float32 and f <= ds.FLOOR_AUDIO * 1.05
    # the float32 transforms are transforms
    s32, s64 = ds.stft32(x, 64, 16), denoise_ref.stft(x, 64, 16)
    assert s32.dtype == np.complex64 and np.abs(s32 - s64).max() <= 1e-6 * np.abs(s64).max()
    assert np.abs(ds.istft32(s64, 16, len(x)) - x).max() <= 1e-6 * np.abs(x).max()


def test_the_restatement_improves_si_sdr_on_the_quality_clip():
    wet, stream, cascade, offline = sc.restatement_si_sdr()
    print(f"SI-SDR: input {wet:.2f}, stream form {stream:.2f}, stream form then gain {cascade:.2f}, offline WPE {offline:.2f} dB")
    assert stream > wet
    assert cascade > stream
