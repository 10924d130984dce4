"""The streaming beamformer on the host: the float64 restatement (tests/beamform_stream_ref.py) against the consequences
include/adn.h states for "beamform stream", the parameter ranges of the three places that hold them, and the quality table.  No test
here needs a device: adn_mvdr_stream_state_bytes is host-only.

Quality (measured on the host, float64 restatements, defaults; profiles/bench_beamform_stream.md): SI-SDR after the first second,
microphone 0 -> streaming MVDR: 1.50 -> 5.08 dB at C = 2, 1.50 -> 7.59 at C = 4, 1.50 -> 7.22 at C = 8 (offline MVDR with the same
mask: 4.61, 7.72, 9.09).  Every row's margin is above 1 dB, so every row is asserted.
"""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_ref as bf  # noqa: E402
import beamform_stream_cases as bsc  # noqa: E402
import beamform_stream_ref as bs  # noqa: E402
import dereverb_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _group(n_frames, channels, g=0):
    spec, mags = bsc.host_inputs(n_frames, channels)
    return spec[g * channels:(g + 1) * channels], mags[g * channels:(g + 1) * channels]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the consequences of the header --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", (1, 3, 8))
@pytest.mark.parametrize("n_frames", (2, 23))
def test_forget_one_refresh_one_ends_where_the_offline_beamformer_does(n_frames, channels):
    specs, mags = _group(n_frames, channels)
    for ref in bc.refs_of(channels):
        y, _ = bs.mvdr_stream(specs, mags, dict(forget=1.0, ref_channel=ref))
        for t in (n_frames - 1, n_frames // 2):                                    # ... and every prefix ends where ITS offline run does
            want = bf.mvdr(specs[:, :t + 1], mags[:, :, :t + 1], dict(ref_channel=ref), order="sequential")
            err = np.abs(y[t] - want[t]).max() / np.abs(want).max()
            print(f"T {n_frames} C {channels} ref {ref} frame {t}: {err:.3g} of the maximum")
            assert err <= 1e-9


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_causal_and_cuts_through_the_state_are_exact(dtype):
    specs, mags = _group(23, 3)
    p = dict(refresh=4, ref_channel=1)
    full, state = bs.mvdr_stream(specs, mags, p, dtype=dtype)
    later, later_mags = specs.copy(), mags.copy()
    later[:, 10:] *= -0.5j                                                       # frames > 9 changed: frames 0 ... 9 do not move
    later_mags[:, :, 10:] = 0.25
    moved, _ = bs.mvdr_stream(later, later_mags, p, dtype=dtype)
    assert np.array_equal(_bits(moved[:10]), _bits(full[:10])) and not np.array_equal(moved[10:], full[10:])
    for cuts in ((1, 8, 23), (7, 23), (4, 5, 6, 22, 23)):                        # at, before and after a refresh frame
        parts, st, lo = [], None, 0
        for hi in cuts:
            y, st = bs.mvdr_stream(specs[:, lo:hi], mags[:, :, lo:hi], p, dtype=dtype, state=st, first_frame=lo)
            parts.append(y)
            lo = hi
        assert np.array_equal(_bits(np.concatenate(parts)), _bits(full)), cuts
        for k in state:
            assert np.array_equal(_bits(st[k]), _bits(state[k])), (cuts, k)
    # frame 0 starts fresh whatever the state holds
    junk = {k: np.full_like(v, np.nan) for k, v in state.items()}
    again, _ = bs.mvdr_stream(specs, mags, p, dtype=dtype, state=junk, first_frame=0)
    assert np.array_equal(_bits(again), _bits(full))
    with pytest.raises(ValueError):
        bs.mvdr_stream(specs, mags, p, first_frame=3)


@pytest.mark.parametrize("channels", (2, 5))
def test_refresh_frames_equal_the_refresh_one_run(channels):
    specs, mags = _group(23, channels)
    every, _ = bs.mvdr_stream(specs, mags, dict(refresh=1))
    fourth, _ = bs.mvdr_stream(specs, mags, dict(refresh=4))
    assert np.array_equal(_bits(fourth[::4]), _bits(every[::4]))
    assert not np.array_equal(fourth[1::4], every[1::4])


def test_one_channel_zero_groups_and_a_nan():
    specs, mags = _group(23, 1)
    for dtype in (np.float64, np.float32):
        y, _ = bs.mvdr_stream(specs, mags, dtype=dtype)
        assert np.array_equal(y, specs[0].astype(y.dtype))                       # C = 1: w = G / G = 1, as values
    specs, mags = _group(23, 3)
    y, st = bs.mvdr_stream(np.zeros_like(specs), np.zeros_like(mags))
    assert not y.any() and not st["w"].any()
    clean, _ = bs.mvdr_stream(specs, mags)
    bad = specs.copy()
    bad[2, 5, 13] = complex(np.nan, 0.25)
    got, _ = bs.mvdr_stream(bad, mags)
    keep = np.ones(bsc.N_BINS, bool)
    keep[13] = False
    assert np.array_equal(_bits(got[:, keep]), _bits(clean[:, keep]))
    assert np.array_equal(_bits(got[:5]), _bits(clean[:5])) and np.isnan(got[5:, 13]).all()    # poisoned from then on


def test_no_wind_up_through_silence():
    """Covariances decay and nothing that is carried grows: a silent stretch scales Phi by alpha^n and the filter goes on."""
    specs, mags = _group(65, 3)
    quiet, quiet_mags = specs.copy(), mags.copy()
    quiet[:, 20:50] = 0
    quiet_mags[:, :, 20:50] = 0
    y, st = bs.mvdr_stream(quiet, quiet_mags, dtype=np.float32)
    _, before = bs.mvdr_stream(quiet[:, :20], quiet_mags[:, :, :20], dtype=np.float32)
    _, after = bs.mvdr_stream(quiet[:, :50], quiet_mags[:, :, :50], dtype=np.float32)
    assert np.isfinite(y).all() and not y[20:50].any()
    for k in ("phi_s", "phi_n"):
        assert np.abs(after[k]).max() <= np.abs(before[k]).max()
    plain, _ = bs.mvdr_stream(specs, mags, dtype=np.float32)
    assert np.abs(y[50:]).max() <= 4.0 * np.abs(plain[50:]).max()


def test_the_restated_solve_is_dereverb_refs():
    rng = np.random.default_rng(0)
    for dtype in (np.complex128, np.complex64):
        b = (rng.standard_normal((7, 5, 5)) + 1j * rng.standard_normal((7, 5, 5))).astype(dtype)
        a = (b @ np.conj(b.transpose(0, 2, 1)) + np.eye(5)).astype(dtype)
        a[:, np.arange(5), np.arange(5)] = a[:, np.arange(5), np.arange(5)].real
        p = (rng.standard_normal((7, 5, 3)) + 1j * rng.standard_normal((7, 5, 3))).astype(dtype)
        g = bs.cholesky_solve_columns(a, p)
        for c in range(3):
            assert np.array_equal(_bits(g[:, :, c]), _bits(dr._cholesky_solve(a, np.ascontiguousarray(p[:, :, c]))))


# ---- the three places that hold the ranges -------------------------------------------------------------------------------------------
RANGE_PROBES = (("ref_channel", (-1, 0, 1, 2, 7, 8)), ("refresh", (0, 1, 4, 64, 65)),
                ("forget", (0.89, 0.9, 0.95, 0.99, 1.0, 1.0001, float("nan"))), ("loading", (0.0, 9e-7, 1e-6, 1e-3, 1.0, 1.5, float("nan"))),
                ("mask_floor", (0.0, 9e-7, 1e-6, 1e-3, 0.25, 0.26, float("nan"))))


def test_parameter_ranges_agree_between_python_the_restatement_and_the_library():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.beamform import MvdrStreamParams, mvdr_stream_state_bytes
    assert dataclasses.asdict(MvdrStreamParams()) == bs.DEFAULTS
    assert tuple(f.name for f in dataclasses.fields(MvdrStreamParams)) == bs.FIELDS
    assert ctypes.sizeof(_lib.MvdrStreamParamsStruct) == 20
    L = _lib.load()
    channels = 2
    for name, values in RANGE_PROBES:
        for v in values:
            p = dict(bs.DEFAULTS, **{name: v})
            try:
                bs.check_params(p, channels)
                ref_ok = True
            except ValueError as exc:
                ref_ok = False
                assert str(exc) == name
            s = MvdrStreamParams().to_struct()
            setattr(s, name, v)
            need = ctypes.c_size_t(12345)
            rc = L.adn_mvdr_stream_state_bytes(3, channels, 33, ctypes.byref(s), ctypes.byref(need))
            assert (rc == 0) == ref_ok, (name, v, L.adn_last_error())
            if ref_ok:
                assert need.value == 3 * 33 * 2 * (channels * (channels + 1) + channels) * 4
            else:
                msg = L.adn_last_error()
                assert rc == 1 and need.value == 12345 and msg.startswith(b"adn_mvdr_stream_state_bytes:") and name.encode() in msg, msg
            try:
                made = MvdrStreamParams(**{name: v})
                py_ok = made.ref_channel < channels                              # ref_channel < channels is the call's rule
            except ValueError as exc:
                py_ok = False
                assert name in str(exc)
            assert py_ok == ref_ok, (name, v)
    for kw in (dict(refresh=2.0), dict(refresh=True), dict(ref_channel=1.0)):
        with pytest.raises(ValueError):
            MvdrStreamParams(**kw)
    with pytest.raises(dataclasses.FrozenInstanceError):
        MvdrStreamParams().forget = 0.5
    # NULL is the defaults, for every channel count; the shape arguments are refused by name
    for c in range(1, 9):
        assert mvdr_stream_state_bytes(2, c, 257) == 2 * 257 * 2 * (c * (c + 1) + c) * 4
    need = ctypes.c_size_t(0)
    for args, word in (((0, 2, 33), b"n_slots"), ((1, 0, 33), b"channels"), ((1, 9, 33), b"channels"), ((1, 2, 0), b"n_bins")):
        assert L.adn_mvdr_stream_state_bytes(*args, None, ctypes.byref(need)) == 1 and word in L.adn_last_error()
    assert L.adn_mvdr_stream_state_bytes(1, 2, 33, None, None) == 1 and b"null" in L.adn_last_error()
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    for name in ("adn_mvdr_stream_state_bytes", "adn_mvdr_online", "adn_mvdr_stream"):
        assert name in _lib.EXPORTED_SYMBOLS and f"ADN_API int {name}(" in header and hasattr(L, name)


def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    L = _lib.load()
    buf = ctypes.create_string_buffer(65536)                 # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    m, q, qm, st = p + 8192, p + 16384, p + 24576, p + 32768  # spec 2 x 4 x 8 x 8 = 512 bytes, mag 2 x 8 x 6 x 4 = 384, state 8 x 64

    def call(params=None, spec=p, mag=m, mag_width=6, mag_col0=2, n=1, c=2, t=4, f=8, first=0, state=st, state_bytes=8 * 64, slots=1,
             out=q, mag_out=qm, width=5, col0=1):
        return L.adn_mvdr_online(spec, mag, mag_width, mag_col0, n, c, t, f, first, params, state, state_bytes, slots, out, mag_out,
                                 width, col0, None)

    for kw, word, code in ((dict(spec=None), b"null", 1), (dict(mag=None), b"null", 1), (dict(out=None), b"null", 1),
                           (dict(state=None), b"null", 1), (dict(n=0), b"n_groups", 1), (dict(t=0), b"n_frames", 1),
                           (dict(f=0), b"n_bins", 1), (dict(c=0), b"channels", 1), (dict(c=9), b"channels", 1),
                           (dict(first=-1), b"first_frame", 1), (dict(first=(1 << 31) - 4), b"first_frame", 1),
                           (dict(mag_col0=-1), b"mag_col0", 1), (dict(mag_col0=3), b"mag_col0", 1), (dict(mag_width=5), b"mag_col0", 1),
                           (dict(col0=-1), b"col0", 1), (dict(col0=2), b"col0", 1), (dict(width=4), b"col0", 1),
                           (dict(n=2, slots=1, state_bytes=1 << 12), b"n_slots", 1), (dict(state_bytes=8 * 64 - 1), b"state", 3),
                           (dict(state=st + 4), b"aligned", 1), (dict(spec=p + 4), b"aligned", 1), (dict(out=q + 4), b"aligned", 1),
                           (dict(mag=m + 2), b"aligned", 1), (dict(mag_out=qm + 2), b"aligned", 1), (dict(out=p), b"overlap", 1),
                           (dict(out=m), b"overlap", 1), (dict(out=st), b"overlap", 1), (dict(mag_out=m), b"overlap", 1),
                           (dict(mag_out=q + 8), b"overlap", 1), (dict(mag_out=st + 8), b"overlap", 1), (dict(state=p + 8), b"overlap", 1),
                           (dict(state=m + 8), b"overlap", 1)):
        assert call(**kw) == code, (kw, L.adn_last_error())
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_mvdr_online:") and word in msg, (kw, msg)
    from audiodenoiser_amd.beamform import MvdrStreamParams
    for name, value in (("ref_channel", 2), ("refresh", 0), ("forget", 0.5), ("loading", float("nan")), ("mask_floor", 0.3)):
        s = MvdrStreamParams().to_struct()
        setattr(s, name, value)
        assert call(ctypes.byref(s)) == 1
        assert L.adn_last_error().startswith(b"adn_mvdr_online:") and name.encode() in L.adn_last_error()

    # adn_mvdr_stream: everything adn_wpe_mc_stream refuses, with the MVDR state in the WPE state's place
    need = ctypes.c_size_t(0)
    plan = (64, 16, 16, 4, 0)
    assert L.adn_stream_state_bytes(4, *plan, 2, ctypes.byref(need)) == 0
    big = ctypes.create_string_buffer(need.value + 64)
    sp = ctypes.addressof(big) + (-ctypes.addressof(big)) % 16

    def stream(params=None, sstate=sp, sbytes=need.value, y=p, n=4, c=2, first=0, steps=1, final=-1, plan=plan, max_steps=2, state=st,
               state_bytes=2 * 33 * 64):
        return L.adn_mvdr_stream(sstate, sbytes, y, n, c, first, steps, final, *plan, max_steps, params, state, state_bytes, None)

    for kw, word, code in ((dict(sstate=None), b"null", 1), (dict(y=None), b"null", 1), (dict(state=None), b"null", 1),
                           (dict(plan=(64, 16, 16, 4, 1), sbytes=1 << 30), b"lookahead", 1), (dict(c=3), b"multiple of channels", 1),
                           (dict(c=0), b"channels", 1), (dict(steps=3), b"", 1), (dict(y=p + 2), b"aligned", 1),
                           (dict(state=st + 4), b"aligned", 1), (dict(state_bytes=2 * 33 * 64 - 1), b"state", 3),
                           (dict(sbytes=need.value - 1), b"", None)):
        rc = stream(**kw)
        assert rc != 0 and (code is None or rc == code), (kw, rc, L.adn_last_error())
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_mvdr_stream:") and word in msg, (kw, msg)
    s = MvdrStreamParams().to_struct()
    s.ref_channel = 2
    assert stream(ctypes.byref(s)) == 1 and b"ref_channel" in L.adn_last_error()


def test_python_face_refuses_before_it_looks_at_a_device():
    import torch
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd.beamform import MvdrStreamParams, StreamBeamformer, mvdr_online
    for name in ("MvdrStreamParams", "mvdr_stream_state_bytes", "mvdr_online", "StreamBeamformer"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.beamform, name)
    spec = torch.zeros((6, 5, 9), dtype=torch.complex64)
    mag = torch.zeros((6, 1, 9, 5))
    for channels in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="channels"):
            mvdr_online(spec, mag, channels)
    with pytest.raises(ValueError, match="multiple of channels"):
        mvdr_online(spec, mag, 4)
    with pytest.raises(ValueError, match="ref_channel"):
        mvdr_online(spec, mag, 2, params=MvdrStreamParams(ref_channel=2))
    with pytest.raises(TypeError):
        mvdr_online(spec, mag, 2, params=dict())
    with pytest.raises(ValueError, match="ROCm device"):
        mvdr_online(spec, mag, 3)
    for kw, word in ((dict(channels=0), "channels"), (dict(channels=9, n_streams=9), "channels"),
                     (dict(n_streams=5, channels=2), "multiple of channels"),
                     (dict(n_streams=2, channels=2, params=MvdrStreamParams(ref_channel=2)), "ref_channel"),
                     (dict(n_fft=500), "n_fft"), (dict(block_frames=0), "block_frames")):
        with pytest.raises(ValueError, match=word):
            StreamBeamformer(**kw)
    for kw in (dict(params=dict()), dict(wpe_params=dict()), dict(mask_params=dict()), dict(gain_params=dict())):
        with pytest.raises(TypeError):
            StreamBeamformer(**kw)


# ---- floors and quality ----------------------------------------------------------------------------------------------------------------
def test_the_float32_floor_of_every_parity_case_is_printed():
    """Frame 0 solves from one frame: both covariances have rank one and only the loading conditions the solve, so the first frames
    set every floor (1e-4 ... 4e-4 at the default loading, as the rank-deficient cases of "beamform").  At loading 1e-6 float32 cannot
    resolve that solve at all: the floor of that case is 0.26 of the bin's maximum, and E <= 4 floor bounds nothing there beyond
    finiteness -- the case stays in the grid as the issue sets it, and its later frames are what the bit pins hold."""
    worst = 0.0
    for case in bsc.parity_cases():
        n_frames, channels, params, extra = case
        b = bsc.bounds(*bsc.host_inputs(n_frames, channels), channels, params)
        print(f"{bsc.label(*case)}: float32 floor {b.floors['sequential']:.3g}")
        assert np.isfinite(b.floor) and b.floor >= 2.0 ** -23
        if "loading" not in params:
            worst = max(worst, b.floor)
    assert worst < 1e-3                                                          # at the default loading a floor is a few 1e-4


def test_streaming_beats_microphone_zero_after_the_first_second():
    print(bsc.quality_table())
    for channels in bsc.QUALITY_CHANNELS:                                        # every row's measured margin is above 1 dB
        q = bsc.quality(channels)
        assert q["stream"][1] >= q["mic0"][1] + 1.0, (channels, q)
