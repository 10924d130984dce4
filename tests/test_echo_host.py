"""The echo canceller on the host: the float64 restatement (tests/echo_ref.py) against the consequences include/adn_echo.h states for
"echo stream", the parameter ranges of the three places that hold them, the floors of the parity cases and the quality figures.
No test here needs a device: adn_aec_stream_state_bytes is host-only and every other call is refused before a launch.

Quality (measured on the host, float64 restatement on the complex64 spectra, defaults, tests/echo_cases.py): ERLE over the
single-talk frames 40 ... 119 16.28 dB; SI-SDR against the near-end spectrum over frames 130 ... end 3.57 -> 19.79 dB.  The asserted
bounds are 10 dB each.
"""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import echo_cases as ec  # noqa: E402
import echo_ref as er  # noqa: E402
import recursive_bounds as rb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- the consequences of the header --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", (dict(taps=8), dict(taps=3, delay=2), dict(taps=1), dict(taps=12, delay=1, loading=0.5)), ids=str)
def test_forget_one_solves_the_normal_equations(params):
    p = dict(params, forget=1.0, quiet=0.0)
    mic, far = _noise((60, 5), 1), _noise((60, 5), 2)
    _, state = er.aec_online(mic, far, p, with_state=True)
    want = er.normal_equations(mic, far, p)
    err = np.abs(state["h"] - want).max() / np.abs(want).max()
    print(f"{params}: h against the normal equations {err:.3g}")
    assert err <= 1e-9


@pytest.mark.parametrize("taps,delay", ((1, 0), (4, 0), (8, 3)))
def test_an_exact_filter_of_the_far_end_is_found_and_cancelled(taps, delay):
    T, F = 4 * taps + 40, 6
    far, h = 1e3 * _noise((T, F), 3), _noise((F, taps), 4)     # loud: the smallest legal loading, 1e-3, is then 1e-9 of a frame's power
    full = np.concatenate([np.zeros((delay + taps - 1, F), complex), far])
    H = delay + taps - 1
    mic = np.stack([sum(np.conj(h[:, j]) * full[H + t - delay - j] for j in range(taps)) for t in range(T)])
    p = dict(taps=taps, delay=delay, forget=1.0, loading=1e-3)
    e, state = er.aec_online(mic, far, p, with_state=True)
    level = np.abs(mic).max()
    print(f"K {taps} D {delay}: residual after 4 K frames {np.abs(e[4 * taps:]).max() / level:.3g}, h {np.abs(state['h'] - h).max():.3g}")
    assert np.abs(e[4 * taps:]).max() <= 1e-6 * level
    assert np.abs(state["h"] - h).max() <= 1e-6 * np.abs(h).max()


def test_a_single_echo_shrinks_and_does_not_double():
    far = _noise((80, 4), 5)
    mic = (0.7 - 0.2j) * far                                                     # one tap, no delay
    e = er.aec_online(mic, far, dict(taps=1, loading=1e-3))
    assert np.abs(e[-20:]).max() < 1e-3 * np.abs(mic).max()
    late = np.concatenate([np.zeros((2, 4), complex), mic[:-2]])                # ... at x~_1 = R_{t-2} of D = 1
    e = er.aec_online(late, far, dict(taps=2, delay=1, loading=1e-3))
    assert np.abs(e[-20:]).max() < 1e-3 * np.abs(mic).max()


def test_zero_inputs():
    mic, far = _noise((30, 7), 6).astype(np.complex64), _noise((30, 7), 7).astype(np.complex64)
    for dtype, arithmetics in ((np.float64, ("plain",)), (np.float32, er.ARITHMETICS)):
        for a in arithmetics:
            e = er.aec_online(mic, np.zeros_like(far), None, dtype=dtype, arithmetic=a)
            assert np.array_equal(e, mic.astype(e.dtype))                        # R = 0: the output is Y
            e = er.aec_online(np.zeros_like(mic), far, None, dtype=dtype, arithmetic=a)
            assert not e.any()                                                   # Y = 0: zero


def test_a_non_finite_value_stays_in_its_bin():
    mic, far = _noise((30, 7), 8), _noise((30, 7), 9)
    clean = er.aec_online(mic, far)
    far[5, 3] = np.nan
    e = er.aec_online(mic, far)
    keep = [b for b in range(7) if b != 3]
    assert np.array_equal(e[:, keep], clean[:, keep]) and np.array_equal(e[:5, 3], clean[:5, 3]) and np.isnan(e[-1, 3])


@pytest.mark.parametrize("dtype,arithmetic", ((np.float64, "plain"), (np.float32, "plain"), (np.float32, "fma")))
def test_the_gate_leaves_the_filter_bit_for_bit(dtype, arithmetic):
    mic, far = _noise((60, 5), 10).astype(np.complex64), _noise((60, 5), 11).astype(np.complex64)
    far[20:45] = 0                                                               # frames 20 + K - 1 ... 44 see a silent stack
    p = dict(taps=4, delay=1)
    kw = dict(dtype=dtype, arithmetic=arithmetic, with_state=True)
    _, before = er.aec_online(mic[:26], far[:26], p, **kw)                       # after frame 25: x~ = R_24 ... R_21 = 0 from 25 on
    _, after = er.aec_online(mic[:45], far[:45], p, **kw)
    for name in ("h", "P"):
        assert np.array_equal(_bits(before[name]), _bits(after[name])), name
    _, later = er.aec_online(mic[:48], far[:48], p, **kw)
    assert not np.array_equal(later["h"], after["h"])
    # a cut through the state is exact, the gated stretch included
    full = er.aec_online(mic, far, p, dtype=dtype, arithmetic=arithmetic)
    head, state = er.aec_online(mic[:30], far[:30], p, **kw)
    tail = er.aec_online(mic[30:], far[30:], p, dtype=dtype, arithmetic=arithmetic, state=state, first_frame=30)
    assert np.array_equal(_bits(np.concatenate([head, tail])), _bits(full))


def test_a_minute_with_a_silent_far_end_stays_finite_in_float32_and_not_without_the_gate():
    mic, far = ec.long_spec()
    first, last = ec.LONG_SILENCE
    e, state = er.aec_online(mic, far, None, dtype=np.float32, arithmetic="fma", with_state=True)
    _, held = er.aec_online(mic[:first + 8], far[:first + 8], None, dtype=np.float32, arithmetic="fma", with_state=True)
    _, still = er.aec_online(mic[:last], far[:last], None, dtype=np.float32, arithmetic="fma", with_state=True)
    print(f"max |P| after the silence {np.abs(still['P']).max():.3g}, at its start {np.abs(held['P']).max():.3g}, at the end {np.abs(state['P']).max():.3g}")
    assert np.isfinite(e).all() and np.isfinite(state["P"]).all()
    # bounded: over the 2000 silent frames P does not move at all (ungated it grows by alpha^-1992 = 2.2e4), and h with it
    assert np.array_equal(_bits(held["P"]), _bits(still["P"])) and np.array_equal(_bits(held["h"]), _bits(still["h"]))
    # without the gate (quiet = 0 gates exact zeros too, so the restatement's gate is taken out: a floor of noise far below quiet)
    rng = np.random.default_rng(0)
    dust = far + (1e-12 * (rng.standard_normal(far.shape) + 1j * rng.standard_normal(far.shape))).astype(np.complex64)
    _, loose = er.aec_online(mic[:last], dust[:last], dict(quiet=0.0), dtype=np.float32, arithmetic="fma", with_state=True)
    print(f"without the gate: max |P| {np.abs(loose['P']).max():.3g}")
    assert np.abs(loose["P"]).max() > 1e3 * np.abs(still["P"]).max()


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_every_parity_floor_is_under_the_cap():
    worst = 0.0
    for n_fft, n_frames, kw in ec.parity_cases():
        b = ec.aec_bounds(*ec.parity_spec(n_fft, n_frames), kw)
        rb.assert_cap(ec.label(n_fft, n_frames, kw), b)
        worst = max(worst, b.floor)
    for n_frames in ec.SHORT_FRAMES:                       # the short cases with an active far end: floors above 2^-23, the update runs
        for kw in ec.SHORT_PARAMS:
            b = ec.aec_bounds(*ec.short_spec(n_frames), kw)
            rb.assert_cap(ec.label(64, n_frames, kw, "short"), b)
            assert n_frames == 1 or max(b.by_arithmetic.values()) > 0.0, (n_frames, kw)
            worst = max(worst, b.floor)
    for n_fft, n_frames in ((64, ec.TILTED_FRAMES), (512, 40)):
        mic, far = ec.parity_spec(n_fft, n_frames)
        for kw in ec.TILTED_PARAMS:
            b = ec.aec_bounds(ec.tilted(mic), ec.tilted(far), kw)
            rb.assert_cap(ec.label(n_fft, n_frames, kw, "tilted"), b)
            worst = max(worst, b.floor)
    print(f"largest floor {worst:.3g}")
    # the layouts' edges are in the grid: G = 8 at 1 and 8 taps, G = 16 at 9 and 16, G = 32 at 17 and 32
    assert sorted((kw or er.DEFAULTS)["taps"] for kw in ec.PARITY_PARAMS) == [1, 8, 9, 16, 17, 32]


def test_quality_of_the_restatement():
    erle, sdr_in, sdr_out = ec.quality_restatement()
    print(f"ERLE {erle:.2f} dB; SI-SDR {sdr_in:.2f} -> {sdr_out:.2f} dB")
    assert erle >= 10.0 and sdr_out >= sdr_in + 10.0


# ---- the ranges, in the three places that hold them ------------------------------------------------------------------------------------
LEGAL = (dict(), dict(taps=1), dict(taps=32, forget=0.984375), dict(delay=8), dict(forget=1.0), dict(loading=1e-3), dict(loading=1e6),
         dict(quiet=0.0), dict(quiet=1.0), dict(taps=9, forget=0.95))
ILLEGAL = (("taps", 0), ("taps", 33), ("delay", -1), ("delay", 9), ("forget", 0.94), ("forget", 1.01), ("forget", float("nan")),
           ("loading", 5e-4), ("loading", 2e6), ("loading", float("nan")), ("quiet", -1e-9), ("quiet", 1.5), ("quiet", float("nan")))
# 2 K (1 - forget) > 1; at taps 10 on the fp32 value of 0.95, which lies below it
WINDOW = (dict(taps=11, forget=0.95), dict(taps=32, forget=0.98), dict(taps=10, forget=0.95))


def test_ranges_of_the_restatement_the_dataclass_and_the_library():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.echo import AecParams, aec_stream_state_bytes
    L = _lib.load_echo()
    need = ctypes.c_size_t(0)
    assert dataclasses.asdict(AecParams()) == er.DEFAULTS and tuple(f.name for f in dataclasses.fields(AecParams)) == er.FIELDS
    for kw in LEGAL:
        p = dict(er.DEFAULTS, **kw)
        er.check_params(p)
        k, d = p["taps"], p["delay"]
        assert aec_stream_state_bytes(3, 33, AecParams(**kw)) == 3 * 33 * (8 * k * k + 16 * k + 8 * d)
    assert aec_stream_state_bytes(2, 257) == 2 * 257 * (8 * 64 + 16 * 8)
    for name, value in ILLEGAL:
        with pytest.raises(ValueError, match=name):
            er.check_params(dict(er.DEFAULTS, **{name: value}))
        with pytest.raises(ValueError, match=name):
            AecParams(**{name: value})
        s = AecParams().to_struct()
        setattr(s, name, value)
        assert L.adn_aec_stream_state_bytes(1, 33, ctypes.byref(s), ctypes.byref(need)) == 1
        msg = L.adn_aec_last_error()
        assert msg.startswith(b"adn_aec_stream_state_bytes:") and name.encode() in msg, msg
    for kw in WINDOW:
        with pytest.raises(ValueError, match="forget"):
            er.check_params(dict(er.DEFAULTS, **kw))
        with pytest.raises(ValueError, match="forget"):
            AecParams(**kw)
        s = AecParams().to_struct()
        s.taps, s.forget = kw["taps"], kw["forget"]
        assert L.adn_aec_stream_state_bytes(1, 33, ctypes.byref(s), ctypes.byref(need)) == 1
        assert b"forget" in L.adn_aec_last_error() and b"taps" in L.adn_aec_last_error()
    for value in (True, 2.0, "8"):
        with pytest.raises(ValueError, match="taps"):
            AecParams(taps=value)
    with pytest.raises(dataclasses.FrozenInstanceError):
        AecParams().forget = 0.99
    for args, word in (((0, 33), b"n_slots"), (((1 << 20) + 1, 33), b"n_slots"), ((1, 0), b"n_bins")):
        assert L.adn_aec_stream_state_bytes(*args, None, ctypes.byref(need)) == 1 and word in L.adn_aec_last_error()
    assert L.adn_aec_stream_state_bytes(1, 33, None, None) == 1 and b"null" in L.adn_aec_last_error()
    header = open(os.path.join(ROOT, "include", "adn_echo.h")).read()
    for name in ("adn_aec_stream_state_bytes", "adn_aec_online", "adn_aec_stream"):
        assert name in _lib.ECHO_EXPORTED_SYMBOLS and f"ADN_API int {name}(" in header and hasattr(L, name)
    for words in ("NOT scale invariant", "not tuned by ear", "Not here:"):
        assert words in header[header.index("echo stream:"):]


def test_the_echo_library_exports_its_header_and_libadn_none_of_it():
    """libadn_echo.so's dynamic symbol table is adn_echo.h's four functions and nothing else, although it is linked from every
    object of libadn.so; libadn.so, whose table is adn.h's, has none of them; each library keeps its own error message."""
    import re
    import subprocess
    from audiodenoiser_amd import _lib
    L, M = _lib.load_echo(), _lib.load()
    header = open(os.path.join(ROOT, "include", "adn_echo.h")).read()
    declared = set(re.findall(r"\b(adn_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.ECHO_EXPORTED_SYMBOLS) and len(declared) == 4

    def table(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split() and ln.split()[-2] in "TWVBDR"}

    assert table(L) == declared
    assert not any(name.startswith("adn_aec") for name in table(M)) and not set(_lib.EXPORTED_SYMBOLS) & declared
    assert "adn_aec" not in open(os.path.join(ROOT, "include", "adn.h")).read().replace("adn_aec_* ", "")
    need = ctypes.c_size_t(0)
    M.adn_stream_state_bytes(0, 64, 16, 16, 4, 0, 2, ctypes.byref(need))         # a refusal of libadn.so ...
    before = M.adn_last_error()
    assert L.adn_aec_stream_state_bytes(0, 33, None, ctypes.byref(need)) == 1
    assert L.adn_aec_last_error().startswith(b"adn_aec_stream_state_bytes:") and M.adn_last_error() == before   # ... is not overwritten


def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.echo import AecParams
    L = _lib.load_echo()
    buf = ctypes.create_string_buffer(1 << 17)               # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16 + 4096
    far, q, qm, st = p + 8192, p + 16384, p + 24576, p + 32768      # a spectrogram 1 x 4 x 8 x 8 = 256 bytes
    rec = 8 * 64 + 16 * 8                                          # the record of a (slot, bin) at the defaults

    def call(params=None, mic=p, far=far, n=1, t=4, f=8, first=0, state=st, state_bytes=8 * rec, slots=1, out=q, mag_out=qm, width=5, col0=1):
        return L.adn_aec_online(mic, far, n, t, f, first, params, state, state_bytes, slots, out, mag_out, width, col0, None)

    for kw, word, code in ((dict(mic=None), b"null", 1), (dict(far=None), b"null", 1), (dict(out=None), b"null", 1),
                           (dict(state=None), b"null", 1), (dict(n=0), b"n_rows", 1), (dict(t=0), b"n_frames", 1),
                           (dict(f=0), b"n_bins", 1), (dict(f=(1 << 20) + 1, state_bytes=1 << 40), b"n_bins", 1),
                           (dict(slots=(1 << 20) + 1, state_bytes=1 << 40), b"n_slots", 1),
                           (dict(first=-1), b"first_frame", 1), (dict(first=(1 << 31) - 4), b"first_frame", 1),
                           (dict(col0=-1), b"col0", 1), (dict(col0=2), b"col0", 1), (dict(width=4), b"col0", 1),
                           (dict(n=2, slots=1, state_bytes=1 << 16), b"n_slots", 1), (dict(state_bytes=8 * rec - 1), b"state", 3),
                           (dict(state=st + 4), b"aligned", 1), (dict(mic=p + 4), b"aligned", 1), (dict(far=far + 4), b"aligned", 1),
                           (dict(out=q + 4), b"aligned", 1), (dict(mag_out=qm + 2), b"aligned", 1), (dict(out=p), b"overlap", 1),
                           (dict(out=far), b"overlap", 1), (dict(out=far + 248), b"overlap", 1), (dict(out=p - 248), b"overlap", 1)):
        assert call(**kw) == code, (kw, L.adn_aec_last_error())
        msg = L.adn_aec_last_error()
        assert msg.startswith(b"adn_aec_online:") and word in msg, (kw, msg)
    for name, value in ILLEGAL:
        s = AecParams().to_struct()
        setattr(s, name, value)
        assert call(ctypes.byref(s)) == 1
        assert L.adn_aec_last_error().startswith(b"adn_aec_online:") and name.encode() in L.adn_aec_last_error()

    need = ctypes.c_size_t(0)
    plan = (64, 16, 16, 4, 0)
    assert _lib.load().adn_stream_state_bytes(4, *plan, 2, ctypes.byref(need)) == 0
    big = ctypes.create_string_buffer(need.value + 64)
    sp = ctypes.addressof(big) + (-ctypes.addressof(big)) % 16

    def stream(params=None, sstate=sp, sbytes=need.value, y=p, n=4, first=0, steps=1, final=-1, plan=plan, max_steps=2, state=st,
               state_bytes=2 * 33 * rec):
        return L.adn_aec_stream(sstate, sbytes, y, n, first, steps, final, *plan, max_steps, params, state, state_bytes, None)

    for kw, word, code in ((dict(sstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(state=None), b"null", 1),
                           (dict(plan=(64, 16, 16, 4, 1), sbytes=1 << 30), b"lookahead", 1), (dict(n=3, sbytes=1 << 30), b"even", 1),
                           (dict(steps=3), b"", 1), (dict(y=p + 2), b"aligned", 1), (dict(state=st + 4), b"aligned", 1),
                           (dict(state_bytes=2 * 33 * rec - 1), b"state", 3), (dict(sbytes=need.value - 1), b"", None)):
        rc = stream(**kw)
        assert rc != 0 and (code is None or rc == code), (kw, rc, L.adn_aec_last_error())
        msg = L.adn_aec_last_error()
        assert msg.startswith(b"adn_aec_stream:") and word in msg, (kw, msg)
    s = AecParams().to_struct()
    s.taps = 40
    assert stream(ctypes.byref(s)) == 1 and b"taps" in L.adn_aec_last_error()


def test_python_face_refuses_before_it_looks_at_a_device():
    import torch
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd import echo
    for name in echo.__all__:
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(echo, name)
    spec = torch.zeros((2, 5, 9), dtype=torch.complex64)
    with pytest.raises(ValueError, match="ROCm device"):
        echo.aec_online(spec, spec)
    with pytest.raises(TypeError, match="AecParams"):
        echo.aec_stream_state_bytes(1, 9, dict(taps=4))
    with pytest.raises(TypeError, match="AecParams"):
        echo.EchoCanceller(params=dict(taps=4))
    with pytest.raises(ValueError, match="pairs"):
        echo.StreamEchoCanceller(pairs=0)
    with pytest.raises(TypeError, match="AecParams"):
        echo.StreamEchoCanceller(pairs=1, params=(8, 0))
    with pytest.raises(SystemExit):
        echo.main(["mic.wav", "far.wav"])
