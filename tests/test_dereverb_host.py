"""Dereverberation baseline without a device: the restatement's own properties (tests/dereverb_ref.py), the Python face
(audiodenoiser_amd/dereverb.py) and the argument checks of adn_wpe / adn_wpe_workspace_bytes, which refuse before anything is
launched.  The quality conditions the device test relies on are evaluated here on the restatement alone.  Measured on the host:
single echo of 0.5 at D = 3 on white rows: 0.447 of the echo energy left; Freeverb'd speech_like(32000, 7): WPE +3.21 dB over the input, the
cascade +2.30 dB over the Wiener gain alone."""
import ctypes
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_cases as dc  # noqa: E402
import dereverb_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ILLEGAL = (("taps", 0), ("taps", 33), ("taps", -1), ("delay", 0), ("delay", 9), ("iterations", 0), ("iterations", 9),
           ("loading", 0.0), ("loading", 9e-7), ("loading", 1.5), ("loading", float("nan")), ("power_floor", 0.0),
           ("power_floor", -1e-3), ("power_floor", 1.01), ("power_floor", float("nan")), ("loading", float("inf")))
LEGAL = (("taps", 1), ("taps", 32), ("delay", 1), ("delay", 8), ("iterations", 1), ("iterations", 8), ("loading", 1e-6),
         ("loading", 1.0), ("power_floor", 1.0), ("power_floor", 1e-12))


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)


def test_params_refuse_every_out_of_range_value_and_nan():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeParams
    p = WpeParams()
    assert dataclasses.asdict(p) == dr.DEFAULTS and tuple(f.name for f in dataclasses.fields(p)) == dr.FIELDS
    s = p.to_struct()
    assert isinstance(s, _lib.WpeParamsStruct) and ctypes.sizeof(s) == 20 and [n for n, _ in s._fields_] == list(dr.FIELDS)
    assert (s.taps, s.delay, s.iterations) == (20, 3, 3) and s.loading == np.float32(1e-3) and s.power_floor == np.float32(1e-3)
    for name, value in ILLEGAL:
        with pytest.raises(ValueError, match=name):
            WpeParams(**{name: value})
        with pytest.raises(ValueError, match=name):
            dr.check_params({**dr.DEFAULTS, name: value})
    for name, value in (("taps", 2.0), ("delay", True), ("iterations", "3")):
        with pytest.raises(ValueError, match=name):
            WpeParams(**{name: value})
    for name, value in LEGAL:
        WpeParams(**{name: value})
        dr.check_params({**dr.DEFAULTS, name: value})


def test_python_defaults_equal_the_headers():
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    m = re.search(r"taps K (\d+), delay D (\d+), iterations I (\d+), loading delta ([\de.-]+), power_floor rho ([\de.-]+)\.", header)
    assert m, "the defaults sentence of the dereverb section"
    assert [float(v) for v in m.groups()] == [float(dr.DEFAULTS[k]) for k in dr.FIELDS]
    assert re.search(r"typedef struct adn_wpe_params \{ int taps, delay, iterations; float loading, power_floor; \} adn_wpe_params;", header)
    api = open(os.path.join(ROOT, "audiodenoiser_amd", "csrc", "adn_api.hip")).read()
    m = re.search(r"adn_wpe_params defaults = \{([^}]*)\}", api)
    assert [float(v.strip().rstrip("f")) for v in m.group(1).split(",")] == [float(dr.DEFAULTS[k]) for k in dr.FIELDS]
    for phrase in ("online / recursive WPE", "more than one channel", "tuning by ear"):
        assert phrase in header
    from audiodenoiser_amd import Denoiser, dereverb
    assert issubclass(dereverb.Dereverberator, Denoiser)
    assert {k for k, v in vars(dereverb.Dereverberator).items() if callable(v)} == {"__init__", "_core"}


def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(8192)                  # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    q = p + 4096

    def call(params=None, spec=p, n=1, t=4, f=8, ws=None, ws_bytes=0, out=q, mag=q + 1024, width=4):
        return L.adn_wpe(spec, n, t, f, params, ws, ws_bytes, out, mag, width, None)

    def size(params=None, n=1, t=4, f=8, bytes_=True):
        need = ctypes.c_size_t(12345)
        return L.adn_wpe_workspace_bytes(n, t, f, params, ctypes.byref(need) if bytes_ else None), need.value

    for name, value in ILLEGAL:
        s = WpeParams().to_struct()
        setattr(s, name, value)
        assert call(ctypes.byref(s)) == 1, (name, value)
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe:") and name.encode() in msg, (name, value, msg)
        rc, need = size(ctypes.byref(s))
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_workspace_bytes:") and name.encode() in msg, (name, value, msg)
    for name, value in LEGAL:
        s = WpeParams(**{name: value}).to_struct()
        assert size(ctypes.byref(s))[0] == 0, (name, value)
    # NULL and misaligned pointers, zero counts, width < n_frames, overlap, a grid of 2^31 workgroups
    for kw, word in ((dict(spec=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b"n_clips"), (dict(t=0), b"n_frames"),
                     (dict(f=0), b"n_bins"), (dict(n=-1), b"n_clips"), (dict(width=3), b"width"), (dict(spec=p + 4), b"aligned"),
                     (dict(out=q + 4), b"aligned"), (dict(mag=q + 1026), b"aligned"), (dict(out=p), b"overlap"),
                     (dict(out=p + 8 * 8 * 3), b"overlap"), (dict(n=1 << 30, f=33, t=1, width=1), b"grid")):
        assert call(**kw) == 1, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_wpe:") and word in msg, (kw, msg)
    for kw, word in ((dict(bytes_=False), b"null"), (dict(n=0), b"n_clips"), (dict(t=0), b"n_frames"), (dict(f=0), b"n_bins"),
                     (dict(n=1 << 30, f=33), b"grid")):
        rc, need = size(**kw)
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_wpe_workspace_bytes:") and word in msg, (kw, msg)
    # a workspace below adn_wpe_workspace_bytes: the size function may report 0 (everything on chip), and then no size is too small
    rc, need = size(n=3, t=188, f=257)
    assert rc == 0
    if need > 0:
        assert call(n=3, t=188, f=257, width=188, ws=p, ws_bytes=need - 1) == 3
        assert L.adn_last_error().startswith(b"adn_wpe:") and b"workspace" in L.adn_last_error()
        assert call(n=3, t=188, f=257, width=188, ws=None, ws_bytes=need) == 3


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_short_rows_and_the_first_frames_pass_through_exactly(dtype):
    ct = np.complex64 if dtype is np.float32 else np.complex128
    for n_frames in (1, 2, 3):                                 # T <= D
        x = _noise((n_frames, 9), n_frames).astype(np.complex64)
        d = dr.wpe(x, dtype=dtype)
        assert d.dtype == ct and np.array_equal(d, x.astype(ct))
    x = _noise((8, 5), 4).astype(np.complex64)                 # T <= D at the largest delay
    assert np.array_equal(dr.wpe(x, dict(delay=8), dtype=dtype), x.astype(ct))
    x = _noise((60, 9), 5).astype(np.complex64)
    for delay in (1, 3, 8):
        d = dr.wpe(x, dict(delay=delay), dtype=dtype)
        assert np.array_equal(d[:delay], x[:delay].astype(ct)) and not np.array_equal(d[delay:], x[delay:].astype(ct))


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_zero_row_gives_zeros(dtype):
    x = _noise((50, 7), 6).astype(np.complex64)
    x[:, 3] = 0
    d = dr.wpe(x, dtype=dtype)
    assert np.all(d[:, 3] == 0) and np.isfinite(d).all()
    assert np.all(dr.wpe(np.zeros((40, 5), np.complex64), dtype=dtype) == 0)


def test_a_row_is_independent_of_its_neighbours():
    x = _noise((70, 12), 7).astype(np.complex64)
    for dtype in (np.float32, np.float64):
        whole = dr.wpe(x, dtype=dtype)
        assert np.array_equal(dr.wpe(x[:, 4:7], dtype=dtype), whole[:, 4:7])
        assert np.array_equal(dr.wpe(x[:, 11:], dtype=dtype), whole[:, 11:])
        bad = x.copy()
        bad[20, 5] = np.nan
        got = dr.wpe(bad, dtype=dtype)
        keep = np.arange(12) != 5
        assert np.array_equal(got[:, keep], whole[:, keep])


def test_single_echo_loses_at_least_half_its_energy():
    """X_t = S_t + a S_{t-D} with white complex S: the predictable part of X_t from X_{t-D} is the echo; the sign and the
    conjugation of g in d = X - sum conj(g) X are right if the echo shrinks (a wrong one doubles it)."""
    n_frames, n_bins, delay, a = 400, 6, 3, 0.5 * np.exp(0.7j)
    s = _noise((n_frames, n_bins), 8)
    x = s.copy()
    x[delay:] += a * s[:-delay]
    d, g = dr.wpe(x.astype(np.complex64), dict(taps=4, delay=delay), with_taps=True)
    echo_in, echo_out = np.sum(np.abs(x - s) ** 2), np.sum(np.abs(d - s) ** 2)
    print(f"echo energy {echo_in:.1f} -> {echo_out:.1f} ({echo_out / echo_in:.3g}); conj(g_0) mean {np.conj(g[:, 0]).mean():.3f}, a = {a:.3f}")
    assert echo_out <= 0.5 * echo_in
    # the first tap points along the echo's coefficient (the 1 / |d|^2 weights of a Gaussian row shrink its length, not its angle)
    assert np.abs(np.angle(np.conj(g[:, 0]) / a)).max() < 0.5


def test_float32_is_carried_out_in_float32_and_the_floor_is_recorded():
    """FLOOR is what `python tests/dereverb_cases.py` measured; here two of its cases stay under it."""
    assert 0 < dr.FLOOR < 1e-2
    spec = _noise((40, 5), 9).astype(np.complex64)
    d32 = dr.wpe(spec, dtype=np.float32)
    assert d32.dtype == np.complex64 and not np.array_equal(d32, dr.wpe(spec).astype(np.complex64))
    import denoise_ref
    for n_fft, n_frames, params in ((64, 23, None), (64, dc.EXTRA_FRAMES, dc.EXTRA_PARAMS[2])):
        x = dc.parity_audio(n_fft, n_frames, 3)[1]
        f = dc.floor_of(denoise_ref.stft(x, n_fft, n_fft // 4).astype(np.complex64), params)
        print(f"n_fft {n_fft} T {n_frames} {params}: {f:.3g} (FLOOR {dr.FLOOR:.3g})")
        assert f <= dr.FLOOR * 1.05                              # FLOOR is written with two digits


def test_quality_conditions_of_the_restatement():
    wet, wpe_, wiener, cascade = dc.restatement_si_sdr()
    print(f"SI-SDR: input {wet:.2f}, WPE {wpe_:.2f}, spectral baseline {wiener:.2f}, WPE then spectral baseline {cascade:.2f} dB")
    assert dc.quality_case()[0].shape == (32000,)
    assert wpe_ - wet >= 2.0
    assert cascade - wiener >= 1.0
