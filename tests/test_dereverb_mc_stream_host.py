"""Streaming multichannel dereverberation without a device: the restatement's own properties
(tests/dereverb_mc_stream_ref.py), the Python face (audiodenoiser_amd/dereverb.py) and the argument checks of
adn_wpe_mc_stream_state_bytes / adn_wpe_mc_online / adn_wpe_mc_stream, which refuse before anything is launched.
Measured on the host (python tests/dereverb_mc_stream_cases.py; profiles/bench_dereverb_mc_stream.md has the tables): the batch
identity holds to 1e-13 or better at T = 50; the float32 restatement stays finite over 3750 frames at N = 32 at forget 0.99 and
at 0.984375, its per-quarter error 1e-5 ... 1e-3 of the maximum with no growth from the second quarter to the fourth; SI-SDR of
the two-microphone recording 3.33 / 3.36 dB in, 6.17 / 6.12 dB out at (2, 16)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_mc_stream_cases as msc  # noqa: E402
import dereverb_mc_stream_ref as ms  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402
from test_dereverb_stream_host import ILLEGAL, LEGAL  # noqa: E402  (the parent's ranges: they hold here unchanged)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("adn_wpe_mc_stream_state_bytes", "adn_wpe_mc_online", "adn_wpe_mc_stream")


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", (None, dict(taps=1, delay=1), dict(taps=32, delay=8, forget=0.95)))
def test_one_channel_is_the_single_channel_restatement_exactly(params):
    x = _noise((40, 5), 1)
    kw = dict(params or {})
    kw.setdefault("taps", 20)                                    # the parent's default, not 32 // 1
    want, want_state = ds.wpe_online(x, params, with_state=True)
    got, got_state = ms.wpe_mc_online(x[None], kw, with_state=True)
    assert got.dtype == np.complex128 and np.array_equal(got[0], want)
    assert np.array_equal(got_state["G"][:, 0], want_state["g"]) and np.array_equal(got_state["P"], want_state["P"])
    assert np.array_equal(got_state["s"], want_state["s"]) and np.array_equal(got_state["past"][:, 0], want_state["past"])


@pytest.mark.parametrize("ck", ((2, 3), (3, 2), (4, 8)))
def test_the_recursion_is_exact_rls_on_the_stacked_vector(ck):
    """With the lam_t it produced and alpha = 1, G after T frames solves the stacked normal equations
    (delta I + sum_t x~_t x~_t^H / lam_t) G_c = sum_t x~_t conj(X_{t,c}) / lam_t, x~[c K + j] = X_{t-D-j, c}."""
    C, K = ck
    T, F, D, N = 50, 3, 2, C * K
    x = _noise((C, T, F), 3)
    d, state, lam = ms.wpe_mc_online(x, dict(taps=K, delay=D, forget=1.0), with_state=True, with_lam=True)
    delta = 1.0 / float(np.float32(1.0) / np.float32(ds.DEFAULTS["loading"]))
    worst = 0.0
    for f in range(F):
        A, B = delta * np.eye(N, dtype=complex), np.zeros((N, C), complex)
        for t in range(T):
            xt = np.array([x[c, t - D - j, f] if t - D - j >= 0 else 0.0 for c in range(C) for j in range(K)])
            A += np.outer(xt, xt.conj()) / lam[t, f]
            B += np.outer(xt, np.conj(x[:, t, f])) / lam[t, f]
        G = np.linalg.solve(A, B)                                # (N, C)
        worst = max(worst, float(np.abs(G - state["G"][f].T).max() / np.abs(G).max()))
    print(f"(C, K) {ck}: max |G - G_batch| / max |G_batch| = {worst:.3g} (bound 1e-9)")
    assert worst <= 1e-9
    # lam is the channels' mean a-priori error power, floored
    assert np.all(lam >= (np.abs(d) ** 2).mean(axis=0) * (1 - 1e-12))


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_p_stays_exactly_hermitian_and_a_cut_into_calls_is_exact(dtype):
    C, K, T = 3, 4, 60
    x = _noise((C, T, 4), 5).astype(np.complex64)
    params = dict(taps=K, delay=2, forget=0.99)
    full, full_state = ms.wpe_mc_online(x, params, dtype=dtype, with_state=True)
    P = full_state["P"]
    assert np.array_equal(P, np.conj(np.swapaxes(P, 1, 2))) and not P[:, np.arange(C * K), np.arange(C * K)].imag.any()
    for cuts in ((1,) * T, (7, 1, 30, 22), (59, 1)):
        parts, state, at = [], None, 0
        for n in cuts:
            part, state = ms.wpe_mc_online(x[:, at:at + n], params, dtype=dtype, state=state, first_frame=at, with_state=True)
            parts.append(part)
            at += n
        assert at == T and np.array_equal(np.concatenate(parts, axis=1), full), cuts
        for name in ("G", "P", "s", "past"):
            assert np.array_equal(state[name], full_state[name]), (cuts, name)
    # a first_frame = 0 call starts fresh whatever the state holds
    junk = {k: np.full_like(v, np.nan) for k, v in full_state.items()}
    assert np.array_equal(ms.wpe_mc_online(x, params, dtype=dtype, state=junk), full)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_the_first_frames_pass_through_exactly_and_a_zero_group_gives_zeros(dtype):
    x = _noise((2, 30, 4), 7).astype(np.complex64)
    for delay in (1, 3, 8):
        d = ms.wpe_mc_online(x, dict(taps=5, delay=delay), dtype=dtype)
        assert np.array_equal(d[:, :delay], x[:, :delay].astype(d.dtype)) and not np.array_equal(d[:, delay:], x[:, delay:].astype(d.dtype))
    z = ms.wpe_mc_online(np.zeros((2, 30, 4), np.complex64), dtype=dtype)
    assert not z.any() and np.isfinite(z).all()
    # a non-finite value poisons all channels of its bin from then on and nothing else
    bad = x.copy()
    bad[1, 10, 2] = complex(np.nan, 0.25)
    clean, got = ms.wpe_mc_online(x, dtype=dtype), ms.wpe_mc_online(bad, dtype=dtype)
    keep = np.ones(4, bool)
    keep[2] = False
    assert np.array_equal(got[:, :, keep], clean[:, :, keep]) and np.array_equal(got[:, :10, 2], clean[:, :10, 2])
    assert np.isnan(got[0, -1, 2]) and np.isnan(got[1, -1, 2])


@pytest.mark.parametrize("index", range(len(msc.LONG_RUNS)), ids=[f"C{c}K{k}-forget{f:g}" for (c, k), f in msc.LONG_RUNS])
def test_the_float32_restatement_stays_finite_for_a_minute_at_the_stacked_size_32(index):
    (channels, taps), forget = msc.LONG_RUNS[index]
    assert channels * taps == 32 and 2.0 * 32 * (1.0 - float(np.float32(forget))) <= 1.0
    finite, _ = msc.long_run(index)
    assert finite, msc.LONG_RUNS[index]


def test_the_forget_rule_of_the_restatement():
    assert ms.lowest_forget(32) == 0.984375 and ms.lowest_forget(16) == 0.96875
    for n in (10, 20, 21, 32):
        f = np.float32(ms.lowest_forget(n))
        assert 2.0 * n * (1.0 - float(f)) <= 1.0 < 2.0 * n * (1.0 - float(np.nextafter(f, np.float32(0))))
    ms.check_params(dict(ms.defaults(2), forget=0.984375), 2)
    ms.check_params(dict(ms.defaults(1), forget=0.95), 1)                               # the rule does not apply to one channel
    for params, channels, word in ((dict(ms.defaults(2), forget=0.98), 2, "forget"), (dict(ms.defaults(2), taps=17), 2, r"channels \* taps"),
                                   (ms.defaults(2), 9, "channels"), (ms.defaults(2), 0, "channels"), (dict(ms.defaults(8), taps=5), 8, "taps")):
        with pytest.raises(ValueError, match=word):
            ms.check_params(params, channels)
    assert [ms.defaults(c)["taps"] for c in range(1, 9)] == [32, 16, 10, 8, 6, 5, 4, 4]


def test_the_floors_are_the_cases_script_s_and_the_cases_are_the_issue_s():
    assert 1e-7 < ms.FLOOR < 1e-3 and 1e-7 < ms.FLOOR_AUDIO < 1e-3
    doc = open(os.path.join(ROOT, "profiles", "bench_dereverb_mc_stream.md")).read()
    host = doc[doc.index("<!-- host:begin -->"):doc.index("<!-- host:end -->")]
    assert f"**{ms.FLOOR:.1e}**" in host and f"**{ms.FLOOR_AUDIO:.1e}**" in host
    cases = list(msc.parity_cases())
    assert {(t, ck) for n_fft, t, ck, extra in cases if n_fft == 64 and extra is None} == \
        {(t, ck) for t in (1, 3, 4, 23, 97) for ck in ((2, 5), (3, 7), (2, 16), (4, 8), (8, 4))}
    assert msc.WIDE_CASE in cases and msc.WIDE_CASE[0] == 512 and msc.WIDE_CASE[2] == (2, 10)
    assert msc.FORGET_CASE in cases and msc.FORGET_CASE[3] == dict(forget=0.984375) and msc.FORGET_CASE[2][0] * msc.FORGET_CASE[2][1] == 32
    assert msc.DELAY_CASE in cases and msc.DELAY_CASE[3] == dict(delay=8)
    assert msc.PARITY_GROUPS == (1, 3)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_loadable():
    from audiodenoiser_amd import _lib
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"ADN_API int " + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    section = header[header.index("---- dereverb stream multichannel:"):]
    section = section[:section.index("ADN_API int adn_wpe_mc_stream_state_bytes")]
    for phrase in ("No reference counterpart", "UNPINNED", "Hermitian update is part of the DEFINITION", "2 N (1 - forget) <= 1",
                   "fewer frames than twice the N unknowns", "starts fresh", "Not here: the stream pool"):
        assert phrase in section, phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    module = open(os.path.join(ROOT, "audiodenoiser_amd", "dereverb.py")).read()
    for text in (header, readme, module):
        assert "dereverb stream multichannel" in text
        assert "streaming or online multichannel WPE" not in text and "Not here: more than one channel;" not in text
    assert "the streaming form is single-channel" not in module


def _state_bytes(L, n_slots=1, channels=2, n_bins=8, params=None, bytes_=True):
    need = ctypes.c_size_t(12345)
    return L.adn_wpe_mc_stream_state_bytes(n_slots, channels, n_bins, params, ctypes.byref(need) if bytes_ else None), need.value


def test_state_bytes_validates_every_parameter_and_names_the_field():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeStreamParams, wpe_stream_state_bytes, wpe_stream_state_bytes_joint
    L = _lib.load()
    # the record: P (N^2), G (N C), the rings (C (D + K)) as float2, s and a pad
    for channels, taps, delay in ((2, 16, 3), (4, 8, 3), (8, 4, 8), (3, 7, 1), (2, 5, 3)):
        n = channels * taps
        want = 4 * (2 * n * n + 2 * n * channels + 2 * channels * (delay + taps) + 2)
        assert wpe_stream_state_bytes_joint(1, channels, 1, WpeStreamParams(taps=taps, delay=delay)) == want
        assert wpe_stream_state_bytes_joint(3, channels, 33, WpeStreamParams(taps=taps, delay=delay)) == 99 * want and want % 8 == 0
    assert wpe_stream_state_bytes_joint(2, 2, 33) == wpe_stream_state_bytes_joint(2, 2, 33, WpeStreamParams(taps=16))  # NULL: 32 / C
    assert wpe_stream_state_bytes_joint(2, 8, 33) == wpe_stream_state_bytes_joint(2, 8, 33, WpeStreamParams(taps=4))
    for taps in (1, 20, 32):                                    # one channel: the single-channel state
        p = WpeStreamParams(taps=taps)
        assert wpe_stream_state_bytes_joint(3, 1, 33, p) == wpe_stream_state_bytes(3, 33, p)
    assert wpe_stream_state_bytes_joint(3, 1, 33) == wpe_stream_state_bytes(3, 33, WpeStreamParams(taps=32))
    for name, value in ILLEGAL:                                  # the parent's ranges, through this function
        s = WpeStreamParams(taps=4).to_struct()
        setattr(s, name, value)
        rc, need = _state_bytes(L, params=ctypes.byref(s))
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_mc_stream_state_bytes:") and name.encode() in msg, (name, value, msg)
    for name, value in LEGAL:
        if name in ("taps", "forget"):
            continue
        assert _state_bytes(L, params=ctypes.byref(WpeStreamParams(taps=4, **{name: value}).to_struct()))[0] == 0, (name, value)
    for kw, word in ((dict(channels=0), b"channels"), (dict(channels=9), b"channels"), (dict(channels=-1), b"channels"),
                     (dict(channels=2, params=WpeStreamParams(taps=17)), b"channels * taps"),
                     (dict(channels=8, params=WpeStreamParams(taps=5)), b"channels * taps"),
                     (dict(channels=3, params=WpeStreamParams(taps=11)), b"channels * taps"),
                     (dict(channels=2, params=WpeStreamParams(taps=16, forget=0.98)), b"forget"),
                     (dict(channels=2, params=WpeStreamParams(taps=16, forget=float(np.nextafter(np.float32(0.984375), np.float32(0))))), b"forget"),
                     (dict(channels=8, params=WpeStreamParams(taps=4, forget=0.97)), b"forget"),
                     (dict(channels=2, params=WpeStreamParams(taps=8, forget=0.96)), b"forget"),
                     (dict(bytes_=False), b"null"), (dict(n_slots=0), b"n_slots"), (dict(n_bins=0), b"n_bins")):
        kw = dict(kw)
        if isinstance(kw.get("params"), WpeStreamParams):
            kw["params"] = ctypes.byref(kw["params"].to_struct())
        rc, need = _state_bytes(L, **kw)
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_mc_stream_state_bytes:") and word in msg, (kw, msg)
    for channels, taps, forget in ((2, 16, 0.984375), (8, 4, 0.984375), (2, 8, 0.96875), (2, 5, 0.951), (2, 10, 0.975), (1, 32, 0.95),
                                   (4, 8, 1.0)):
        assert _state_bytes(L, channels=channels, params=ctypes.byref(WpeStreamParams(taps=taps, forget=forget).to_struct()))[0] == 0


def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeStreamParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)               # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    q, st, mg = p + 4096, p + 8192, p + 16384
    big = 1 << 40

    def online(params=None, spec=p, n=1, c=2, t=4, f=8, first=0, state=st, state_bytes=big, slots=1, out=q, mag=mg, width=4, col0=0):
        return L.adn_wpe_mc_online(spec, n, c, t, f, first, params, state, state_bytes, slots, out, mag, width, col0, None)

    plan = (512, 128, 16, 4, 0)

    def stream(params=None, sstate=p, sbytes=big, y=q, n=2, c=2, first=0, steps=1, final=-1, plan=plan, max_steps=4, wstate=st, wbytes=big):
        return L.adn_wpe_mc_stream(sstate, sbytes, y, n, c, first, steps, final, *plan, max_steps, params, wstate, wbytes, None)

    bad_params = [(name, value, WpeStreamParams(taps=4).to_struct()) for name, value in ILLEGAL]
    for name, value, s in bad_params:
        setattr(s, name, value)
    bad_params += [("channels * taps", None, WpeStreamParams(taps=17).to_struct()), ("forget", None, WpeStreamParams(taps=16, forget=0.98).to_struct())]
    for name, value, s in bad_params:
        for call, who in ((online, b"adn_wpe_mc_online:"), (stream, b"adn_wpe_mc_stream:")):
            assert call(ctypes.byref(s)) == 1, (name, value, who)
            msg = L.adn_last_error()
            assert msg.startswith(who) and name.encode() in msg, (name, value, msg)

    need = _state_bytes(L, 1, 2, 8)[1]
    for kw, word, status in ((dict(spec=None), b"null", 1), (dict(out=None), b"null", 1), (dict(state=None), b"null", 1),
                             (dict(n=0), b"n_groups", 1), (dict(t=0), b"n_frames", 1), (dict(f=0), b"n_bins", 1), (dict(n=-1), b"n_groups", 1),
                             (dict(c=0), b"channels", 1), (dict(c=9), b"channels", 1),
                             (dict(first=-1), b"first_frame", 1), (dict(first=(1 << 31) - 2), b"first_frame", 1),
                             (dict(slots=0), b"n_slots", 1), (dict(n=2, slots=1), b"n_slots", 1),
                             (dict(width=3), b"width", 1), (dict(col0=1), b"col0", 1), (dict(col0=-1, width=9), b"col0", 1),
                             (dict(spec=p + 4), b"aligned", 1), (dict(out=q + 4), b"aligned", 1), (dict(mag=mg + 2), b"aligned", 1),
                             (dict(state=st + 4), b"aligned", 1), (dict(out=p), b"overlap", 1), (dict(out=p + 8 * 8 * 7), b"overlap", 1),
                             (dict(state_bytes=need - 1), b"adn_wpe_mc_stream_state_bytes", 3), (dict(state_bytes=0), b"state", 3)):
        assert online(**kw) == status, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_mc_online:") and word in msg, (kw, msg)

    sbytes = ctypes.c_size_t()
    assert L.adn_stream_state_bytes(2, *plan, 4, ctypes.byref(sbytes)) == 0
    wneed = _state_bytes(L, 1, 2, 257)[1]
    for kw, word, status in ((dict(sstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(wstate=None), b"null", 1),
                             (dict(plan=(512, 128, 16, 4, 1)), b"lookahead", 1), (dict(plan=(500, 128, 16, 4, 0)), b"n_fft", 1),
                             (dict(n=0), b"n_streams", 1), (dict(n=3), b"multiple of channels", 1), (dict(n=4, c=3), b"multiple of channels", 1),
                             (dict(c=0), b"channels", 1), (dict(c=9), b"channels", 1),
                             (dict(first=-1), b"first_step", 1), (dict(steps=0), b"n_steps", 1),
                             (dict(steps=5), b"max_steps", 1), (dict(final=0), b"final_length", 1), (dict(y=q + 2), b"aligned", 1),
                             (dict(wstate=st + 4), b"aligned", 1), (dict(sstate=p + 4), b"aligned", 1),
                             (dict(final=1000, first=9), b"past the last step", 1),
                             (dict(sbytes=sbytes.value - 1), b"adn_stream_state_bytes", 3),
                             (dict(wbytes=wneed - 1), b"adn_wpe_mc_stream_state_bytes", 3)):
        assert stream(**kw) == status, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_mc_stream:") and word in msg, (kw, msg)


# ---- the Python face ------------------------------------------------------------------------------------------------------------
def test_python_argument_checks_that_need_no_device():
    import inspect
    import torch
    from audiodenoiser_amd import dereverb
    from audiodenoiser_amd.dereverb import StreamDereverberator, WpeStreamParams, wpe_online_joint, wpe_stream_state_bytes_joint
    for name in ("wpe_online_joint", "wpe_stream_state_bytes_joint"):
        assert name in dereverb.__all__
    sig = inspect.signature(StreamDereverberator.__init__)
    assert sig.parameters["channels"].default == 1 and list(sig.parameters)[-1] == "channels"
    assert list(inspect.signature(wpe_online_joint).parameters) == ["spec", "channels", "state", "first_frame", "params", "mag_out", "col0"]
    assert list(inspect.signature(wpe_stream_state_bytes_joint).parameters) == ["n_slots", "channels", "n_bins", "params"]
    # the multichannel rules are checked where the channel count is known; WpeStreamParams keeps its ranges
    assert WpeStreamParams(taps=32, forget=0.95).taps == 32
    spec = torch.zeros((4, 3, 8), dtype=torch.complex64)
    for kw, word in ((dict(channels=0), "channels"), (dict(channels=9), "channels"), (dict(channels=True), "channels"),
                     (dict(channels=2.0), "channels"), (dict(channels=2, params=WpeStreamParams(taps=17)), r"channels \* taps"),
                     (dict(channels=2, params=WpeStreamParams(taps=16, forget=0.98)), "forget"),
                     (dict(channels=3), "multiple of channels")):
        with pytest.raises(ValueError, match=word):
            wpe_online_joint(spec, **kw)
    with pytest.raises(TypeError):
        wpe_online_joint(spec, 2, params=dict(taps=4))
    with pytest.raises(ValueError, match="ROCm"):
        wpe_online_joint(spec, 2)                                # a CPU tensor: refused after the parameter checks
    # the constructor refuses what breaks the rules before it looks at a device
    for kw, word in ((dict(n_streams=3, channels=2), "multiple of channels"), (dict(n_streams=2, channels=0), "channels"),
                     (dict(n_streams=9, channels=9), "channels"), (dict(n_streams=2, channels=2, params=WpeStreamParams()), r"channels \* taps"),
                     (dict(n_streams=2, channels=2, params=WpeStreamParams(taps=16, forget=0.97)), "forget"),
                     (dict(n_streams=4, channels=4, params=WpeStreamParams(taps=8, forget=0.98)), "forget")):
        with pytest.raises(ValueError, match=word):
            StreamDereverberator(torch.device("cuda", 0), **kw)
    assert dereverb._joint_stream_params("x", None, 4) == WpeStreamParams(taps=8)
    assert dereverb._joint_stream_params("x", None, 8).taps == 4 and dereverb._joint_stream_params("x", None, 3).taps == 10
