"""The multi-reference echo canceller on the host: the float64 restatement (tests/echo_mr_ref.py) against the single-reference one
it must equal at refs = 1 and against the consequences include/adn_call.h states for "echo stream multireference"; the floors of
the parity cases; the quality figures; every refusal of the three entry points of libadn_call.so and of the Python face.  No test
here needs a device: adn_aec_mr_state_bytes is host-only and every other call is refused before a launch, on pointers that are never
dereferenced.

Quality (measured on the host, float64 restatement on the complex64 spectra, tests/echo_mr_cases.py; ERLE over the single-talk
frames 40 ... 119, SI-SDR against the near-end spectrum over frames 130 ... end):
    Q = 2   one reference (channel 0) 9.72 dB, 5.31 dB; (mean) 11.75 dB, 10.78 dB; two references 2 x 8   18.05 dB, 17.52 dB
    Q = 4   one reference (channel 0) 4.03 dB, 1.87 dB; (mean)  4.97 dB,  3.65 dB; four references 4 x 4  17.09 dB, 15.29 dB
The asserted bounds are 10 dB each, and 3 dB above the better single-reference form (measured margins 6.3 / 6.7 and 12.1 / 11.6 dB).
The largest float32 floor of a parity case is 2.3e-5 (2 x 3, D = 1, forget 0.95, 97 frames), the cap 1e-4.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import echo_cases as ec  # noqa: E402
import echo_mr_cases as mc  # noqa: E402
import echo_mr_ref as mr  # noqa: E402
import echo_ref as er  # noqa: E402
import recursive_bounds as rb  # noqa: E402
from test_echo_host import ILLEGAL, WINDOW  # noqa: E402  (the illegal parameter values of adn_echo.h: one list)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- 1. one reference is the parent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,arithmetic", ((np.float64, "plain"), (np.float32, "plain"), (np.float32, "fma")))
@pytest.mark.parametrize("params", (None, dict(taps=5, delay=2), dict(taps=32, delay=8, forget=0.984375)), ids=str)
def test_one_reference_is_the_single_reference_restatement_bit_for_bit(params, dtype, arithmetic):
    mic, far = _noise((45, 6), 1).astype(np.complex64), _noise((45, 6), 2).astype(np.complex64)
    far[20:30] = 0                                                               # some gated frames too
    kw = dict(dtype=dtype, arithmetic=arithmetic, with_state=True)
    want, want_state = er.aec_online(mic, far, params, **kw)
    got, got_state = mr.aec_mr_online(mic, far[None], params, **kw)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))
    for name in ("h", "P"):
        assert np.array_equal(_bits(got_state[name]), _bits(want_state[name])), name
    assert got_state["past"].shape[0] == 1 and np.array_equal(_bits(got_state["past"][0]), _bits(want_state["past"]))
    # ... and a cut through the state too
    head, state = mr.aec_mr_online(mic[:17], far[None, :17], params, **kw)
    tail = mr.aec_mr_online(mic[17:], far[None, 17:], params, dtype=dtype, arithmetic=arithmetic, state=state, first_frame=17)
    assert np.array_equal(_bits(np.concatenate([head, tail])), _bits(want))
    assert mr.defaults(1) == er.DEFAULTS and mr.FIELDS == er.FIELDS


def test_the_default_taps_do_not_fill_the_stack():
    assert [mr.defaults(q)["taps"] for q in range(1, 9)] == [8, 8, 5, 4, 3, 2, 2, 2]
    for q in range(2, 9):
        assert {k: v for k, v in mr.defaults(q).items() if k != "taps"} == {k: v for k, v in er.DEFAULTS.items() if k != "taps"}
        mr.check_params(q, mr.defaults(q))


# ---- 2. the consequences of the header ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refs,params", ((2, dict(taps=4)), (3, dict(taps=3, delay=2)), (8, dict(taps=1)), (2, dict(taps=6, delay=1, loading=0.5))),
                         ids=str)
def test_forget_one_solves_the_stacked_normal_equations(refs, params):
    p = dict(params, forget=1.0, quiet=0.0)
    mic, far = _noise((60, 5), 1), _noise((refs, 60, 5), 2)
    _, state = mr.aec_mr_online(mic, far, p, with_state=True)
    want = mr.normal_equations(mic, far, p)
    err = np.abs(state["h"] - want).max() / np.abs(want).max()
    print(f"refs {refs} {params}: h against the stacked normal equations {err:.3g}")
    assert err <= 1e-9                                                           # test_echo_host.py's tolerance for the parent's statement


def test_the_stack_is_channel_major_with_the_lag_ascending():
    """An exact filter of the stacked vector, h_r at r = q K + j on R_{t-D-j, q}, is found tap by tap in that order."""
    refs, taps, delay, T, F = 3, 2, 1, 70, 4
    far, h = 1e3 * _noise((refs, T, F), 3), _noise((F, refs * taps), 4)
    pad = np.concatenate([np.zeros((refs, delay + taps, F), complex), far], axis=1)
    mic = np.stack([sum(np.conj(h[:, q * taps + j]) * pad[q, delay + taps + t - delay - j] for q in range(refs) for j in range(taps))
                    for t in range(T)])
    e, state = mr.aec_mr_online(mic, far, dict(taps=taps, delay=delay, forget=1.0, loading=1e-3), with_state=True)
    assert np.abs(e[4 * refs * taps:]).max() <= 1e-6 * np.abs(mic).max()
    assert np.abs(state["h"] - h).max() <= 1e-6 * np.abs(h).max()


def test_zero_inputs_a_non_finite_value_and_the_gate_on_the_stacked_power():
    mic, far = _noise((40, 7), 6).astype(np.complex64), _noise((2, 40, 7), 7).astype(np.complex64)
    for dtype, arithmetics in ((np.float64, ("plain",)), (np.float32, mr.ARITHMETICS)):
        for a in arithmetics:
            e = mr.aec_mr_online(mic, np.zeros_like(far), None, dtype=dtype, arithmetic=a)
            assert np.array_equal(e, mic.astype(e.dtype))                        # all references zero: the output is Y
            e = mr.aec_mr_online(np.zeros_like(mic), far, None, dtype=dtype, arithmetic=a)
            assert not e.any()                                                   # Y = 0: zero
    clean = mr.aec_mr_online(mic, far)
    bad = far.copy()
    bad[1, 5, 3] = np.nan
    e = mr.aec_mr_online(mic, bad)
    keep = [b for b in range(7) if b != 3]
    assert np.array_equal(e[:, keep], clean[:, keep]) and np.array_equal(e[:5, 3], clean[:5, 3]) and np.isnan(e[-1, 3])
    # the gate: both channels silent freezes P and h bit for bit; ONE silent channel does not (the header's stated limit)
    p = dict(taps=3, delay=1)
    kw = dict(dtype=np.float32, arithmetic="fma", with_state=True)
    both = far.copy()
    both[:, 12:30] = 0                                                           # the stack is silent from frame 12 + K + D - 1 = 15 on
    _, before = mr.aec_mr_online(mic[:16], both[:, :16], p, **kw)
    _, after = mr.aec_mr_online(mic[:30], both[:, :30], p, **kw)
    assert all(np.array_equal(_bits(before[n]), _bits(after[n])) for n in ("h", "P"))
    mic, one = _noise((80, 7), 8).astype(np.complex64), _noise((2, 80, 7), 9).astype(np.complex64)
    one[1, 12:] = 0
    p = dict(taps=3, delay=1, forget=0.95)
    _, before = mr.aec_mr_online(mic[:20], one[:, :20], p, **kw)
    _, after = mr.aec_mr_online(mic, one, p, **kw)
    grown = np.abs(np.diagonal(after["P"][:, 3:, 3:], axis1=1, axis2=2)).min() / np.abs(np.diagonal(before["P"][:, 3:, 3:], axis1=1, axis2=2)).max()
    print(f"one silent channel: its block of P grew {grown:.3g} x over 60 adapted frames (0.95^-60 = {0.95 ** -60:.3g})")
    assert grown > 5.0                                                           # channel 1's block grows by about 1 / alpha a frame


def test_a_minute_with_a_silent_far_end_stays_finite_in_float32():
    mic, far = mc.long_spec(2)
    first, last = mc.LONG_SILENCE
    e, state = mr.aec_mr_online(mic, far, None, dtype=np.float32, arithmetic="plain", with_state=True)
    _, held = mr.aec_mr_online(mic[:first + 8], far[:, :first + 8], None, dtype=np.float32, arithmetic="plain", with_state=True)
    _, still = mr.aec_mr_online(mic[:last], far[:, :last], None, dtype=np.float32, arithmetic="plain", with_state=True)
    print(f"2 x 8: max |P| after the silence {np.abs(still['P']).max():.3g}, at its start {np.abs(held['P']).max():.3g}, at the end {np.abs(state['P']).max():.3g}")
    assert state["P"].shape[1:] == (16, 16)
    assert np.isfinite(e).all() and np.isfinite(state["P"]).all() and np.isfinite(state["h"]).all()
    assert np.array_equal(_bits(held["P"]), _bits(still["P"])) and np.array_equal(_bits(held["h"]), _bits(still["h"]))


# ---- 3. the cases ------------------------------------------------------------------------------------------------------------------
def test_every_parity_floor_is_under_the_cap():
    worst = ("", 0.0)
    for n_fft, n_frames, refs, kw in mc.cases():
        b = mc.aec_mr_bounds(*mc.parity_spec(n_fft, n_frames, refs), kw)
        rb.assert_cap(mc.label(n_fft, n_frames, refs, kw), b)
        worst = max(worst, (mc.label(n_fft, n_frames, refs, kw), b.floor), key=lambda v: v[1])
    for n_frames in mc.SHORT_FRAMES:                       # the short cases with an active far end: the update runs
        for refs, kw in mc.LAYOUTS:
            b = mc.aec_mr_bounds(*mc.short_spec(n_frames, refs), kw)
            rb.assert_cap(mc.label(64, n_frames, refs, kw, "short"), b)
            assert n_frames == 1 or max(b.by_arithmetic.values()) > 0.0, (n_frames, refs, kw)
            worst = max(worst, (mc.label(64, n_frames, refs, kw, "short"), b.floor), key=lambda v: v[1])
    for refs, kw in mc.TILTED_PARAMS:
        mic, far = mc.parity_spec(64, mc.TILTED_FRAMES, refs)
        b = mc.aec_mr_bounds(mc.tilted(mic), mc.tilted(far), kw)
        rb.assert_cap(mc.label(64, mc.TILTED_FRAMES, refs, kw, "tilted"), b)
    print(f"largest floor {worst[1]:.3g} ({worst[0]})")
    # one set per lane layout and edge, as (Q, K, D), and every set legal
    assert [(q,) + mc.taps_delay(q, kw) for q, kw in mc.PARAMS] == [(8, 1, 0), (2, 4, 0), (2, 3, 1), (3, 5, 2), (2, 8, 0), (4, 4, 0),
                                                                     (2, 9, 0), (5, 6, 1), (2, 16, 8), (8, 4, 0)]
    assert [mc.lanes(q, kw) for q, kw in mc.PARAMS] == [8, 8, 8, 16, 16, 16, 32, 32, 32, 32]
    for q, kw in mc.PARAMS:
        mr.check_params(q, dict(mr.defaults(q), **(kw or {})))


@pytest.mark.parametrize("refs,params", mc.QUALITY, ids=("2x8", "4x4"))
def test_quality_of_the_restatement_and_its_margin_over_one_reference(refs, params):
    erle, sdr_in, sdr_out = mc.quality_restatement(refs, params)
    singles = {which: mc.quality_single(refs, which) for which in ("first", "mean")}
    for which, (s_erle, _, s_sdr) in singles.items():
        print(f"Q = {refs}, one reference ({which}): ERLE {s_erle:.2f} dB; SI-SDR {sdr_in:.2f} -> {s_sdr:.2f} dB")
    print(f"Q = {refs}, {refs} references at the default: ERLE {erle:.2f} dB; SI-SDR {sdr_in:.2f} -> {sdr_out:.2f} dB")
    assert mc.taps_delay(refs, params) == ({2: 8, 4: 4}[refs], 0)
    assert erle >= 10.0 and sdr_out >= 10.0
    assert erle >= max(s[0] for s in singles.values()) + 3.0
    assert sdr_out >= max(s[2] for s in singles.values()) + 3.0


def test_the_quality_recipe_with_one_loudspeaker_is_the_parents():
    for got, want in zip(mc.quality_audio(1), ec.quality_audio()):
        assert np.array_equal(np.squeeze(got), want)


# ---- 4. the ranges and the refusals ------------------------------------------------------------------------------------------------
MR_ILLEGAL = ((0, None, b"refs"), (9, None, b"refs"), (-1, None, b"refs"), (2, dict(taps=17), b"taps"), (8, dict(taps=5), b"taps"),
              (3, dict(taps=11), b"refs"), (2, dict(taps=16, forget=0.98), b"forget"), (4, dict(taps=4, forget=0.96), b"forget"),
              (8, dict(taps=4, forget=0.984), b"forget"))
MR_LEGAL = ((1, None), (2, None), (8, None), (2, dict(taps=16, forget=0.984375)), (8, dict(taps=4, delay=8)), (3, dict(taps=10, forget=0.99)),
            (4, dict(taps=4, forget=0.96875)))


def _struct(kw):
    from audiodenoiser_amd.echo import AecParams
    return None if kw is None else ctypes.byref(AecParams(**kw).to_struct())


def test_ranges_of_the_restatement_the_python_face_and_the_library():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.echo import AecParams, aec_mr_state_bytes, aec_stream_state_bytes, mr_default_taps
    L = _lib.load_call()
    need = ctypes.c_size_t(0)
    who = b"adn_aec_mr_state_bytes:"
    for refs, kw in MR_LEGAL:
        mr.check_params(refs, dict(mr.defaults(refs), **(kw or {})))
        assert mr_default_taps(refs) == mr.defaults(refs)["taps"]
        want = 3 * 33 * 4 * mc.record_floats(refs, kw)
        assert aec_mr_state_bytes(3, 33, refs, None if kw is None else AecParams(**kw)) == want, (refs, kw)
        assert L.adn_aec_mr_state_bytes(3, 33, refs, _struct(kw), ctypes.byref(need)) == 0 and need.value == want
    for kw in (None, dict(taps=32, delay=8, forget=0.984375), dict(taps=3, delay=2)):     # one reference: the parent's record
        p = None if kw is None else AecParams(**kw)
        assert aec_mr_state_bytes(2, 257, 1, p) == aec_stream_state_bytes(2, 257, p)
    for refs, kw, word in MR_ILLEGAL:
        with pytest.raises(ValueError):
            mr.check_params(refs, dict(mr.defaults(max(1, min(refs, 8))), **(kw or {})))
        with pytest.raises(ValueError, match=word.decode()):
            aec_mr_state_bytes(1, 33, refs, None if kw is None else AecParams(**kw))
        assert L.adn_aec_mr_state_bytes(1, 33, refs, _struct(kw), ctypes.byref(need)) == 1, (refs, kw)
        msg = L.adn_call_last_error()
        assert msg.startswith(who) and word in msg, (refs, kw, msg)
    for name, value in ILLEGAL:                              # the parent's ranges, by the parent's code
        s = AecParams().to_struct()
        setattr(s, name, value)
        assert L.adn_aec_mr_state_bytes(1, 33, 2, ctypes.byref(s), ctypes.byref(need)) == 1
        assert L.adn_call_last_error().startswith(who) and name.encode() in L.adn_call_last_error()
    for kw in WINDOW:
        s = AecParams().to_struct()
        s.taps, s.forget = kw["taps"], kw["forget"]
        assert L.adn_aec_mr_state_bytes(1, 33, 1, ctypes.byref(s), ctypes.byref(need)) == 1
        assert b"forget" in L.adn_call_last_error() and b"taps" in L.adn_call_last_error()
    for args, word in (((0, 33), b"n_slots"), (((1 << 20) + 1, 33), b"n_slots"), ((1, 0), b"n_bins")):
        assert L.adn_aec_mr_state_bytes(*args, 2, None, ctypes.byref(need)) == 1 and word in L.adn_call_last_error()
    assert L.adn_aec_mr_state_bytes(1, 33, 2, None, None) == 1 and b"null" in L.adn_call_last_error()
    for value in (True, 2.0, "2"):
        with pytest.raises(ValueError, match="refs"):
            aec_mr_state_bytes(1, 33, value)
    with pytest.raises(TypeError, match="AecParams"):
        aec_mr_state_bytes(1, 33, 2, dict(taps=4))
    header = open(os.path.join(ROOT, "include", "adn_call.h")).read()
    section = header[header.index("echo stream multireference:"):]
    for name in ("adn_aec_mr_state_bytes", "adn_aec_mr_online", "adn_aec_mr_stream"):
        assert name in _lib.CALL_EXPORTED_SYMBOLS and f"ADN_API int {name}(" in section and hasattr(L, name)
    for words in ("#define ADN_CALL_MAX_REFS 8", "NOT guarded", "not tuned by ear", "Not here:", "channel-major"):
        assert words in section, words
    for other in ("adn_echo.h",):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "more than one reference channel (" in text and "adn_call.h" in text[text.index("Not here:"):] and "adn_aec_mr" not in text


def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.echo import AecParams
    L, E, M = _lib.load_call(), _lib.load_echo(), _lib.load()
    need = ctypes.c_size_t(0)
    E.adn_aec_stream_state_bytes(0, 33, None, ctypes.byref(need))                # a refusal of the echo library ...
    e_before = E.adn_aec_last_error()
    buf = ctypes.create_string_buffer(1 << 17)               # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16 + 4096
    far, q, qm, st = p + 8192, p + 16384, p + 24576, p + 32768      # a spectrogram 1 x 4 x 8 x 8 = 256 bytes; far_spec two of them
    rec = 4 * mc.record_floats(2, None)                            # the record of a (slot, bin) at refs = 2 and its defaults

    def call(params=None, refs=2, mic=p, far=far, n=1, t=4, f=8, first=0, state=st, state_bytes=8 * rec, slots=1, out=q, mag_out=qm, width=5,
             col0=1):
        return L.adn_aec_mr_online(mic, far, n, refs, t, f, first, params, state, state_bytes, slots, out, mag_out, width, col0, None)

    who = b"adn_aec_mr_online:"
    for kw, word, code in ((dict(mic=None), b"null", 1), (dict(far=None), b"null", 1), (dict(out=None), b"null", 1),
                           (dict(state=None), b"null", 1), (dict(n=0), b"n_rows", 1), (dict(t=0), b"n_frames", 1),
                           (dict(f=0), b"n_bins", 1), (dict(f=(1 << 20) + 1, state_bytes=1 << 40), b"n_bins", 1),
                           (dict(slots=(1 << 20) + 1, state_bytes=1 << 40), b"n_slots", 1),
                           (dict(first=-1), b"first_frame", 1), (dict(first=(1 << 31) - 4), b"first_frame", 1),
                           (dict(col0=-1), b"col0", 1), (dict(col0=2), b"col0", 1), (dict(width=4), b"col0", 1),
                           (dict(n=2, slots=1, state_bytes=1 << 16), b"n_slots", 1), (dict(state_bytes=8 * rec - 1), b"state", 3),
                           (dict(state=st + 4), b"aligned", 1), (dict(mic=p + 4), b"aligned", 1), (dict(far=far + 4), b"aligned", 1),
                           (dict(out=q + 4), b"aligned", 1), (dict(mag_out=qm + 2), b"aligned", 1), (dict(out=p), b"overlap", 1),
                           (dict(out=far), b"overlap", 1), (dict(out=far + 256), b"overlap", 1),         # the SECOND reference's spectrogram
                           (dict(out=far + 504), b"overlap", 1), (dict(out=p - 248), b"overlap", 1),
                           (dict(refs=0), b"refs", 1), (dict(refs=9), b"refs", 1)):
        rc = call(**kw)
        msg = L.adn_call_last_error()
        assert rc == code, (kw, rc, msg)
        assert msg.startswith(who) and word in msg, (kw, msg)
    # a state sized for the parent's default record is too small for two references at their default (N = 16)
    assert call(state_bytes=8 * (8 * 64 + 16 * 8)) == 3 and b"adn_aec_mr_state_bytes" in L.adn_call_last_error()
    for refs, kw, word in MR_ILLEGAL:
        assert call(_struct(kw), refs=refs, state_bytes=1 << 30) == 1, (refs, kw)
        msg = L.adn_call_last_error()
        assert msg.startswith(who) and word in msg, (refs, kw, msg)
    for name, value in ILLEGAL:
        s = AecParams().to_struct()
        setattr(s, name, value)
        assert call(ctypes.byref(s)) == 1
        assert L.adn_call_last_error().startswith(who) and name.encode() in L.adn_call_last_error()

    plan = (64, 16, 16, 4, 0)
    assert M.adn_stream_state_bytes(6, *plan, 2, ctypes.byref(need)) == 0
    big = ctypes.create_string_buffer(need.value + 64)
    sp = ctypes.addressof(big) + (-ctypes.addressof(big)) % 16

    def stream(params=None, refs=2, sstate=sp, sbytes=need.value, y=p, n=6, first=0, steps=1, final=-1, plan=plan, max_steps=2, state=st,
               state_bytes=2 * 33 * rec):
        return L.adn_aec_mr_stream(sstate, sbytes, y, n, refs, first, steps, final, *plan, max_steps, params, state, state_bytes, None)

    who = b"adn_aec_mr_stream:"
    for kw, word, code in ((dict(sstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(state=None), b"null", 1),
                           (dict(plan=(64, 16, 16, 4, 1), sbytes=1 << 30), b"lookahead", 1),
                           (dict(n=5, sbytes=1 << 30), b"multiple of refs + 1", 1), (dict(n=4, sbytes=1 << 30), b"multiple of refs + 1", 1),
                           (dict(refs=3, sbytes=1 << 30, state_bytes=1 << 30), b"multiple of refs + 1", 1),
                           (dict(refs=1, n=5, sbytes=1 << 30), b"multiple of refs + 1", 1),
                           (dict(refs=0), b"refs", 1), (dict(refs=9), b"refs", 1),
                           (dict(steps=3), b"", 1), (dict(y=p + 2), b"aligned", 1), (dict(state=st + 4), b"aligned", 1),
                           (dict(state_bytes=2 * 33 * rec - 1), b"state", 3), (dict(sbytes=need.value - 1), b"", None)):
        rc = stream(**kw)
        msg = L.adn_call_last_error()
        assert rc != 0 and (code is None or rc == code), (kw, rc, msg)
        assert msg.startswith(who) and word in msg, (kw, msg)
    for refs, kw, word in MR_ILLEGAL:
        assert stream(_struct(kw), refs=refs, sbytes=1 << 30, state_bytes=1 << 30) == 1, (refs, kw)
        msg = L.adn_call_last_error()
        assert msg.startswith(who) and word in msg, (refs, kw, msg)
    s = AecParams().to_struct()
    s.taps = 40
    assert stream(ctypes.byref(s)) == 1 and b"taps" in L.adn_call_last_error()
    assert E.adn_aec_last_error() == e_before                # ... stayed what it was through all of it


def test_python_face_refuses_before_it_looks_at_a_device():
    import torch
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd import echo
    from audiodenoiser_amd.echo import AecParams
    for name in ("aec_mr_online", "aec_mr_state_bytes"):
        assert name in echo.__all__ and name in pkg.__all__ and getattr(pkg, name) is getattr(echo, name)
    mic, far = torch.zeros((2, 5, 9), dtype=torch.complex64), torch.zeros((2, 2, 5, 9), dtype=torch.complex64)
    with pytest.raises(ValueError, match="ROCm device"):
        echo.aec_mr_online(mic, far, 2)
    with pytest.raises(ValueError, match="refs"):
        echo.aec_mr_online(mic, far, 0)
    with pytest.raises(ValueError, match="refs \\* taps"):
        echo.aec_mr_online(mic, far, 2, params=AecParams(taps=17))
    with pytest.raises(ValueError, match="forget"):
        echo.aec_mr_online(mic, far, 2, params=AecParams(taps=16, forget=0.98))
    with pytest.raises(TypeError, match="AecParams"):
        echo.aec_mr_online(mic, far, 2, params=dict(taps=4))
    for cls in (echo.EchoCanceller, echo.StreamEchoCanceller):
        for kw, word in ((dict(refs=0), "refs"), (dict(refs=9), "refs"), (dict(refs=True), "refs"), (dict(refs=2.0), "refs"),
                         (dict(refs=4, params=AecParams(taps=9)), "refs \\* taps"),
                         (dict(refs=8, params=AecParams(taps=4, forget=0.98)), "forget")):
            with pytest.raises(ValueError, match=word):
                cls(**kw)
        with pytest.raises(TypeError, match="AecParams"):
            cls(refs=2, params=dict(taps=4))
    with pytest.raises(ValueError, match="pairs"):
        echo.StreamEchoCanceller(pairs=0, refs=2)
    for argv in (["mic.wav", "far.wav", "out.wav", "--refs", "9"], ["mic.wav", "far.wav", "out.wav", "--refs", "4", "--taps", "9"],
                 ["mic.wav", "far.wav", "--refs", "2"]):
        with pytest.raises(SystemExit):
            echo.main(argv)
