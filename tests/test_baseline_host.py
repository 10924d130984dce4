"""Spectral baseline without a device: the restatement's own properties (tests/baseline_ref.py), the Python face
(audiodenoiser_amd/baseline.py) and the argument checks of adn_spectral_gain, which refuse before anything is launched."""
import ctypes
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_cases as bc  # noqa: E402
import baseline_ref as br  # noqa: E402
import denoise_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ILLEGAL = (("smooth", -0.01), ("smooth", 1.0), ("beta", -0.5), ("beta", 1.0), ("alpha", -1e-3), ("alpha", 1.0), ("gamma", 0.0),
           ("gamma", 1.0), ("gain_floor", 0.0), ("gain_floor", 1.01), ("bias", 0.0), ("bias", 100.5), ("bias", float("nan")),
           ("smooth", float("nan")), ("gamma", float("inf")))
LEGAL = (("smooth", 0.0), ("beta", 0.0), ("alpha", 0.0), ("gain_floor", 1.0), ("bias", 100.0), ("gamma", 0.5))


def _spec(n_fft=512, n_frames=188, seed=3):
    x = bc.white_mix(bc.parity_length(n_fft, n_frames), 8.0, seed)[0]
    return denoise_ref.stft(x, n_fft, n_fft // 4).astype(np.complex64)


@pytest.mark.parametrize("n_fft,n_frames", ((64, 188), (512, 97)))
def test_float32_chunk_invariance_is_exact(n_fft, n_frames):
    spec = _spec(n_fft, n_frames)
    whole, state = br.spectral_gain(spec, dtype=np.float32)
    for cuts in ((1, 8, 40), (32, 64), (n_frames - 1,)):
        parts, st, lo = [], None, 0
        for hi in cuts + (n_frames,):
            m, st = br.spectral_gain(spec[lo:hi], state=st, dtype=np.float32)
            parts.append(m)
            lo = hi
        assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(st, state)
    assert whole.dtype == np.float32 and state.dtype == np.float32 and state.shape == (3, n_fft // 2 + 1)


def test_fresh_start_sentinel_per_bin():
    spec = _spec(64, 40)
    first, st = br.spectral_gain(spec[:20])
    st[0, ::2] = -1.0                                         # every other bin starts again
    got, _ = br.spectral_gain(spec[20:], state=st)
    cont, _ = br.spectral_gain(spec[20:], state=br.spectral_gain(spec[:20])[1])
    fresh, _ = br.spectral_gain(spec[20:])
    assert np.array_equal(got[::2], fresh[::2]) and np.array_equal(got[1::2], cont[1::2])


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_zero_input_gives_zero_output(dtype):
    m, st = br.spectral_gain(np.zeros((50, 33), np.complex64), dtype=dtype)
    assert np.all(m == 0) and np.all(st == 0)


def test_non_finite_poisons_its_own_row_from_that_frame_on():
    spec = _spec(64, 40)
    clean, _ = br.spectral_gain(spec, dtype=np.float32)
    for bad in (np.nan, np.inf):
        s = spec.copy()
        s[17, 5] = bad
        m, st = br.spectral_gain(s, dtype=np.float32)
        rows = np.arange(33) != 5
        assert np.array_equal(m[rows], clean[rows]) and np.array_equal(m[5, :17], clean[5, :17])
        assert np.isnan(m[5, 17:]).all() and not np.isfinite(st[:, 5]).any()


def test_minimum_tracker_settles_on_stationary_white_noise():
    """Complex white noise of power sigma^2 per bin, 2000 frames: after 200 frames the time average of bias * Pmin of a bin lies
    within a factor of the true power.  Measured with the defaults over 129 bins: the averages range over 0.39 .. 0.48 sigma^2 and
    the mean over bins is 0.43 (a minimum tracker sits below the mean of an exponentially distributed periodogram; `bias` is there
    to lift it).  Asserted with margin: every bin within [0.3, 0.6], the mean within [0.35, 0.5]."""
    rng = np.random.default_rng(11)
    sigma2 = 0.37
    z = (rng.standard_normal((2000, 129)) + 1j * rng.standard_normal((2000, 129))) * np.sqrt(sigma2 / 2.0)
    n_est = np.empty((2000, 129))
    st = None
    for t in range(2000):
        _, st = br.spectral_gain(z[t:t + 1], state=st)
        n_est[t] = st[1]
    ratio = n_est[200:].mean(axis=0) / sigma2
    print(f"Pmin / sigma^2 per bin: {ratio.min():.3f} .. {ratio.max():.3f}, mean {ratio.mean():.3f}")
    assert 0.3 <= ratio.min() and ratio.max() <= 0.6 and 0.35 <= ratio.mean() <= 0.5


def test_restatement_improves_si_sdr_of_the_8_db_white_mix():
    noisy, clean = bc.quality_case(8.0)
    assert noisy.shape == (48000,)
    out = br.denoise(noisy.astype(np.float64), 512, 128)
    before, after = br.si_sdr(noisy, clean), br.si_sdr(out, clean)
    print(f"SI-SDR {before:.2f} -> {after:.2f} dB")
    assert abs(before - 8.0) < 0.2 and after - before >= 3.0


def test_floor_is_recorded_and_plausible():
    """FLOOR is what `python tests/baseline_cases.py` measured; here the long, cancellation-prone case alone stays under it."""
    assert 0 < br.FLOOR < 1e-4
    spec = denoise_ref.stft(bc.parity_audio(64, 188, 1)[0], 64, 16).astype(np.complex64)
    assert bc.floor_of(spec) <= br.FLOOR * 1.05             # FLOOR is written with two digits


def test_package_imports_and_params_round_trip():
    from audiodenoiser_amd import _lib, baseline
    p = baseline.SpectralParams()
    assert dataclasses.asdict(p) == br.DEFAULTS and tuple(f.name for f in dataclasses.fields(p)) == br.FIELDS
    s = p.to_struct()
    assert isinstance(s, _lib.SpectralParamsStruct) and ctypes.sizeof(s) == 24
    assert [name for name, _ in s._fields_] == list(br.FIELDS)
    back = baseline.SpectralParams.from_struct(s)
    for name in br.FIELDS:
        assert getattr(back, name) == float(np.float32(br.DEFAULTS[name]))
    q = baseline.SpectralParams(0.75, 0.9375, 0.5, 0.875, 0.25, 2.5)       # exact in fp32
    assert baseline.SpectralParams.from_struct(q.to_struct()) == q
    assert issubclass(baseline.SpectralDenoiser, __import__("audiodenoiser_amd").Denoiser)
    own = {k for k, v in vars(baseline.SpectralDenoiser).items() if callable(v)}
    assert own == {"__init__", "_core", "gain"}


def test_python_defaults_equal_the_headers():
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    m = re.search(r"smooth a_s ([\d.]+), beta b ([\d.]+), gamma g ([\d.]+), alpha ([\d.]+), gain_floor g_min\s+\*?\s*([\d.]+), bias ([\d.]+)\.",
                  header)
    assert m, "the defaults sentence of the baseline section"
    assert [float(v) for v in m.groups()] == [br.DEFAULTS[k] for k in br.FIELDS]
    assert re.search(r"typedef struct \{ float smooth, beta, gamma, alpha, gain_floor, bias; \} adn_spectral_params;", header)
    api = open(os.path.join(ROOT, "audiodenoiser_amd", "csrc", "adn_api.hip")).read()
    m = re.search(r"adn_spectral_params defaults = \{([^}]*)\}", api)
    assert [float(v.strip().rstrip("f")) for v in m.group(1).split(",")] == [br.DEFAULTS[k] for k in br.FIELDS]


def test_illegal_parameters_and_shapes_are_refused():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import SpectralParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(4096)                  # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def call(params=None, spec=p, n=1, t=4, f=8, out=p, width=4, col0=0, s_in=None, s_out=None):
        return L.adn_spectral_gain(spec, n, t, f, params, s_in, s_out, out, width, col0, None)

    for name, value in ILLEGAL:
        with pytest.raises(ValueError):
            SpectralParams(**{name: value})
        with pytest.raises(ValueError):
            br.check_params({**br.DEFAULTS, name: value})
        s = SpectralParams().to_struct()
        setattr(s, name, value)
        assert call(ctypes.byref(s)) == 1 and name.encode() in L.adn_last_error(), (name, value)
    for name, value in LEGAL:
        SpectralParams(**{name: value})
        br.check_params({**br.DEFAULTS, name: value})
    for kw in (dict(spec=None), dict(out=None), dict(n=0), dict(t=0), dict(f=0), dict(col0=-1), dict(col0=1), dict(width=3),
               dict(t=1 << 30, width=1 << 30, col0=1 << 30), dict(spec=p + 4), dict(out=p + 2), dict(s_in=p + 1), dict(s_out=p + 3),
               dict(n=1 << 30, f=65, t=1, width=1)):
        assert call(**kw) == 1 and L.adn_last_error().startswith(b"adn_spectral_gain"), kw


def _host_classes():
    """(class, the name its refusals carry, how to construct it without a device): the three classes that take a model get a CPU
    ``UNet(1, 1).eval()``, the six that take a device get ``"cpu"``."""
    from audiodenoiser_amd import Denoiser, StreamDenoiser, StreamPool, baseline, dereverb
    from audiodenoiser_amd.model import UNet
    net = UNet(1, 1).eval()
    return [(Denoiser, "Denoiser", net), (StreamDenoiser, "StreamDenoiser", net), (StreamPool, "StreamPool", net),
            (baseline.SpectralDenoiser, "SpectralDenoiser", "cpu"), (dereverb.Dereverberator, "Dereverberator", "cpu"),
            (baseline.StreamSpectralDenoiser, "StreamSpectralDenoiser", "cpu"),
            (dereverb.StreamDereverberator, "StreamDereverberator", "cpu"),
            (baseline.SpectralStreamPool, "StreamPool", "cpu"), (dereverb.DereverbStreamPool, "StreamPool", "cpu")]


def test_every_class_refuses_the_stft_plan_by_name_before_it_looks_at_the_device():
    """One check (``_host.check_stft_plan``) behind every class, the three with a model and the six without: an illegal transform is
    a ValueError that names the class (``StreamPool`` for the three pools), raised although the model / device given is a CPU one
    -- which alone would be a RuntimeError."""
    for cls, who, first in _host_classes():
        with pytest.raises(RuntimeError, match="no CPU path"):
            cls(first)                                      # legal plan: the device is what is refused
        for kw in (dict(n_fft=500), dict(n_fft=32), dict(n_fft=512, hop_length=512 // 4 + 1), dict(n_fft=64, hop_length=64 // 4 + 1),
                   dict(sample_rate=0)):
            with pytest.raises(ValueError, match=rf"^{who}: ") as exc:
                cls(first, **kw)
            word = "sample_rate" if "sample_rate" in kw else "hop_length" if "hop_length" in kw else "power of two in [64, 4096]"
            assert word in str(exc.value), (cls.__name__, kw, str(exc.value))
