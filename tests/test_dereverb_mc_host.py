"""Multichannel dereverberation without a device: the restatement's own properties (tests/dereverb_mc_ref.py), the gain over the
per-channel operator that the feature exists for, the Python face (audiodenoiser_amd/dereverb.py) and the argument checks of
adn_wpe_mc / adn_wpe_mc_workspace_bytes, which refuse before anything is launched.
Measured on the host (float64 restatements, speech_like(32000, 7) heard by two microphones, SI-SDR after the inverse STFT):
input 3.33 / 3.36 dB; per channel K = 20: 6.54 / 5.17; joint (2, 10): 6.92 / 6.94; joint (2, 16): 9.95 / 10.52."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_ref as mr  # noqa: E402
import dereverb_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)).astype(np.complex64)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (None, dict(taps=20), dict(taps=7, delay=1, iterations=2, loading=1e-6)), ids=("null", "k20", "other"))
def test_one_channel_is_the_single_channel_restatement(kw):
    x = _noise((70, 11), 1)
    want = dr.wpe(x, kw if kw is not None else dict(taps=32))              # NULL at C = 1: taps = 32 / 1
    got = mr.wpe_mc(x[None], kw)
    assert got.shape == (1, 70, 11) and got.dtype == np.complex128
    err = float(np.abs(got[0] - want).max() / np.abs(want).max())
    print(f"C = 1 against dereverb_ref.wpe, {kw}: {err:.3g} of the maximum (bound 1e-12)")
    assert err <= 1e-12


def test_defaults_and_legal_ranges():
    assert [mr.defaults(c)["taps"] for c in range(1, 9)] == [32, 16, 10, 8, 6, 5, 4, 4]
    assert {k: v for k, v in mr.defaults(3).items() if k != "taps"} == {k: v for k, v in dr.DEFAULTS.items() if k != "taps"}
    for channels, taps in ((0, 1), (9, 1), (2, 17), (3, 11), (8, 5), (1, 33)):
        with pytest.raises(ValueError):
            mr.check_params(dict(dr.DEFAULTS, taps=taps), channels)
    for channels, taps in ((1, 32), (2, 16), (3, 10), (8, 4), (8, 1)):
        mr.check_params(dict(dr.DEFAULTS, taps=taps), channels)
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    section = header[header.index("dereverb multichannel: joint WPE"):header.index("dereverb stream: recursive WPE")]
    for phrase in ("32, 16, 10, 8, 6, 5, 4, 4", "not tuned by ear", "UNPINNED", "channels * taps <= 32", "1 <= channels <= 8",
                   "returns adn_wpe's bits", "under a permutation of the channels", "no atomics"):
        assert phrase in section, phrase


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_pass_through_zero_groups_and_isolation(dtype):
    ct = np.complex64 if dtype is np.float32 else np.complex128
    for n_frames in (1, 2, 3):                                                 # T <= D
        x = _noise((3, n_frames, 5), n_frames)
        assert np.array_equal(mr.wpe_mc(x, dtype=dtype), x.astype(ct))
    x = _noise((3, 40, 6), 4)
    for delay in (1, 3, 8):                                                    # the first D frames of every channel
        d = mr.wpe_mc(x, dict(taps=4, delay=delay), dtype=dtype)
        assert np.array_equal(d[:, :delay], x[:, :delay].astype(ct)) and not np.array_equal(d[:, delay:], x[:, delay:].astype(ct))
    assert np.all(mr.wpe_mc(np.zeros((2, 30, 4), np.complex64), dtype=dtype) == 0)
    whole = mr.wpe_mc(x, dtype=dtype)
    assert np.array_equal(mr.wpe_mc(x[:, :, 2:5], dtype=dtype), whole[:, :, 2:5])          # a bin does not see its neighbours
    bad = x.copy()
    bad[1, 20, 3] = np.nan
    keep = np.arange(6) != 3
    assert np.array_equal(mr.wpe_mc(bad, dtype=dtype)[:, :, keep], whole[:, :, keep])
    # one zero bin in a live group: zeros there, in every channel
    x[:, :, 1] = 0
    assert np.all(mr.wpe_mc(x, dtype=dtype)[:, :, 1] == 0)


def test_a_second_microphone_removes_an_echo_the_first_cannot_predict():
    """Two microphones, X_c = S + a_c E with E an echo that is NOT a delayed copy of S in either channel alone (it is white) but is
    seen by both: ... the sign and the conjugation of G in d = X - G^H x~ are right if the cross-channel taps shrink it."""
    n_frames, n_bins, delay = 400, 5, 2
    s, e = _noise((n_frames, n_bins), 8), _noise((n_frames, n_bins), 9)
    late = np.zeros_like(e)
    late[delay:] = e[:-delay]
    x = np.stack([s + 0.8 * late + 0.05 * e, 0.1 * s + e])                     # channel 1 hears the echo's source early
    joint = mr.wpe_mc(x, dict(taps=2, delay=delay))
    alone = dr.wpe(x[0], dict(taps=2, delay=delay))
    before = float(np.sum(np.abs(x[0] - s) ** 2))
    after_joint, after_alone = float(np.sum(np.abs(joint[0] - s) ** 2)), float(np.sum(np.abs(alone - s) ** 2))
    print(f"error energy of channel 0: {before:.1f} -> joint {after_joint:.1f}, alone {after_alone:.1f}")
    assert after_joint <= 0.5 * before and after_joint <= 0.5 * after_alone


def test_joint_beats_per_channel_on_the_two_microphone_recording():
    """The figures of the issue's table, from the restatement: joint at the same stacked size is better on both channels, and at
    the stacked size 32 by at least 2 dB on both."""
    rows = {label: mc.restatement_si_sdr(label) for label in ("input", "per channel, K = 20", "joint, C = 2, K = 10", "joint, C = 2, K = 16")}
    for label, v in rows.items():
        print(f"{label}: " + " / ".join(f"{s:.2f}" for s in v) + " dB")
    wet, dry = mc.recording(2)
    assert wet.shape == (2, 32000) and dry.shape == (32000,)
    alone, same, wide = rows["per channel, K = 20"], rows["joint, C = 2, K = 10"], rows["joint, C = 2, K = 16"]
    for c in range(2):
        assert alone[c] > rows["input"][c]
        assert same[c] > alone[c], (c, same[c], alone[c])
        assert wide[c] >= alone[c] + 2.0, (c, wide[c], alone[c])


def test_float32_is_carried_out_in_float32_and_the_floor_is_recorded():
    """The floors are what `python tests/dereverb_mc_cases.py` measured; here two of its cases stay under theirs."""
    assert 0 < mr.FLOOR_DEFAULT_LOADING < mr.FLOOR < 1e-2
    x = _noise((2, 40, 5), 9)
    d32 = mr.wpe_mc(x, dtype=np.float32)
    assert d32.dtype == np.complex64 and not np.array_equal(d32, mr.wpe_mc(x).astype(np.complex64))
    for n_fft, n_frames, ck, extra in ((64, 23, (3, 7), None), mc.LOADING_CASE):
        f = mc.floor_of(mc.group_specs(n_fft, n_frames, ck[0], 1), mc.params_of(ck, extra))
        print(f"n_fft {n_fft} T {n_frames} {ck} {extra}: {f:.3g} (its floor {mc.floor_for(extra):.3g})")
        assert f <= mc.floor_for(extra) * 1.05                   # the floors are written with two digits
    assert sum(1 for _ in mc.parity_cases()) == 6 * 7 + 2


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(16384)                 # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    q = p + 8192

    def call(params=None, spec=p, n=1, c=2, t=4, f=8, ws=None, ws_bytes=0, out=q, mag=q + 2048, width=4):
        return L.adn_wpe_mc(spec, n, c, t, f, params, ws, ws_bytes, out, mag, width, None)

    def size(params=None, n=1, c=2, t=4, f=8, bytes_=True):
        need = ctypes.c_size_t(12345)
        return L.adn_wpe_mc_workspace_bytes(n, c, t, f, params, ctypes.byref(need) if bytes_ else None), need.value

    def both(word, params=None, **kw):
        assert call(params, **kw) == 1, (word, kw)
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_mc:") and word in msg, (kw, msg)
        rc, need = size(params, **kw)
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_mc_workspace_bytes:") and word in msg, (kw, msg)

    both(b"channels", c=0)
    both(b"channels", c=9)
    both(b"channels", c=-1)
    for channels, taps in ((3, 11), (1, 33), (2, 17), (8, 5)):              # 33, 33, 34, 40
        s = WpeParams().to_struct()
        s.taps = taps
        both(b"taps", ctypes.byref(s), c=channels)
    for name, value in (("loading", float("nan")), ("loading", 0.0), ("power_floor", float("nan")), ("delay", 0), ("delay", 9),
                        ("iterations", 0), ("iterations", 9), ("taps", 0)):
        s = WpeParams(taps=4).to_struct()
        setattr(s, name, value)
        both(name.encode(), ctypes.byref(s))
    for kw, word in ((dict(n=0), b"n_groups"), (dict(t=0), b"n_frames"), (dict(f=0), b"n_bins"), (dict(n=1 << 30, c=2), b"2^31"),
                     (dict(n=1 << 29, c=2, f=33), b"grid")):
        both(word, **kw)
    for kw, word in ((dict(spec=None), b"null"), (dict(out=None), b"null"), (dict(width=3), b"width"), (dict(spec=p + 4), b"aligned"),
                     (dict(out=q + 4), b"aligned"), (dict(mag=q + 2050), b"aligned"), (dict(out=p), b"overlap"),
                     (dict(out=p + 2 * 4 * 8 * 8 - 8), b"overlap"), (dict(spec=q + 8, out=q), b"overlap")):
        assert call(**kw) == 1, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe_mc:") and word in msg, (kw, msg)
    assert size(bytes_=False)[0] == 1 and b"null" in L.adn_last_error()
    # the defaults are legal for every channel count, and so is every (C, K) of the parity cases
    for channels in range(1, 9):
        assert size(c=channels)[0] == 0, channels
        s = WpeParams(taps=32 // channels).to_struct()
        assert size(ctypes.byref(s), c=channels)[0] == 0
    for channels, taps in mc.PARITY_CK:
        assert size(ctypes.byref(WpeParams(taps=taps).to_struct()), c=channels)[0] == 0
    # a workspace below adn_wpe_mc_workspace_bytes: the size function may report 0 (everything on chip), and then no size is too small
    rc, need = size(n=3, c=2, t=188, f=257)
    assert rc == 0
    if need > 0:
        assert call(n=3, c=2, t=188, f=257, width=188, ws=p, ws_bytes=need - 1) == 3
        assert L.adn_last_error().startswith(b"adn_wpe_mc:") and b"workspace" in L.adn_last_error()
        assert call(n=3, c=2, t=188, f=257, width=188, ws=None, ws_bytes=need) == 3


# ---- the Python face ---------------------------------------------------------------------------------------------------------------
def test_python_face_refuses_before_it_looks_at_a_device():
    import torch
    from audiodenoiser_amd import dereverb
    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams, wpe_joint
    assert "wpe_joint" in dereverb.__all__
    spec = torch.zeros((6, 5, 9), dtype=torch.complex64)
    for channels in (0, 9, -2, 2.0, True, "2"):
        with pytest.raises(ValueError, match="channels"):
            wpe_joint(spec, channels)
    with pytest.raises(ValueError, match="multiple of channels"):
        wpe_joint(spec, 4)
    with pytest.raises(ValueError, match=r"channels \* taps"):
        wpe_joint(spec, 2, WpeParams())                                         # 2 x 20
    with pytest.raises(ValueError, match=r"channels \* taps"):
        wpe_joint(spec, 3, WpeParams(taps=11))
    with pytest.raises(TypeError):
        wpe_joint(spec, 2, dict(taps=4))
    with pytest.raises(ValueError, match="ROCm device"):                        # legal arguments: only the device is missing
        wpe_joint(spec, 3)
    for bad in ("both", None, 2, True):
        with pytest.raises(ValueError, match="channels must be 'separate' or 'joint'"):
            Dereverberator(channels=bad)
    # the parameters of a joint call: 32 // C by default, the caller's when they fit
    assert [dereverb._joint_params("x", None, c).taps for c in range(1, 9)] == [32, 16, 10, 8, 6, 5, 4, 4]
    assert dereverb._joint_params("x", WpeParams(taps=16, delay=2), 2) == WpeParams(taps=16, delay=2)
    with pytest.raises(ValueError, match=r"x: need channels \* taps <= 32"):
        dereverb._joint_params("x", WpeParams(), 2)


def test_wpe_params_itself_is_unchanged():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeParams
    assert dataclasses.asdict(WpeParams()) == dr.DEFAULTS and tuple(f.name for f in dataclasses.fields(WpeParams)) == dr.FIELDS
    assert ctypes.sizeof(_lib.WpeParamsStruct) == 20
    WpeParams(taps=32)                                                          # still legal on its own: the product is the call's rule
    for name in ("adn_wpe_mc_workspace_bytes", "adn_wpe_mc"):
        assert name in _lib.EXPORTED_SYMBOLS
