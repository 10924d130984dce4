"""Host-side checks of the quality metrics: the definitions of include/adn.h ("quality") through their float64 restatement
tests/quality_ref.py -- constants, frame rules and known answers -- and the C entry points as far as they run without a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_cases as qc  # noqa: E402
import quality_ref as qr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("adn_quality_workspace_bytes", "adn_quality", "adn_stoi_workspace_bytes", "adn_stoi")


# ---- STOI: constants and frame rules ---------------------------------------------------------------------------------------------
def test_band_table_follows_from_its_definition():
    assert qr.band_table() == qr.BAND_TABLE
    assert qr.BAND_TABLE[0] == (7, 9) and qr.BAND_TABLE[-1] == (174, 219) and len(qr.BAND_TABLE) == 15
    assert all(a[1] == b[0] for a, b in zip(qr.BAND_TABLE, qr.BAND_TABLE[1:]))
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    text = " ".join(f"({lo},{hi})" for lo, hi in qr.BAND_TABLE)
    assert text in " ".join(header.replace("*", " ").split()), "adn.h states another band table"


def test_window_is_hanning_258_without_its_zeros():
    w = qr.window()
    assert w.shape == (256,) and w.min() > 0 and np.allclose(w, w[::-1], atol=1e-15)
    assert np.allclose(w, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1, 257) / 257), atol=1e-15)


@pytest.mark.parametrize("length,frames", [(256, 0), (257, 1), (384, 1), (385, 2), (256 + 128 * 7, 7), (100, 0)])
def test_frame_count_rule(length, frames):
    assert len(qr.frame_starts(length)) == frames


def test_compacted_signal_has_one_frame_less_than_kept():
    for name, est, ref in qc.stoi_cases():
        idx, tr, te = qr.stoi_parts(est, ref)
        assert tr.shape == te.shape == (15, max(len(idx) - 1, 0)), name
    idx, tr, _ = qr.stoi_parts(*[c for c in qc.stoi_cases() if c[0] == "quiet_middle"][0][1:])
    n = len(qr.frame_starts(20000))
    assert 31 <= len(idx) < n - 20, "the quiet stretch must drop frames and leave enough for a segment"
    assert np.any(np.diff(idx) > 1), "adjacent kept frames must come from non-adjacent sources"


def test_compacted_formula_equals_overlap_add():
    """Step 3 as the header writes it (two terms per sample) against the explicit overlap-add of the restatement."""
    _, est, ref = [c for c in qc.stoi_cases() if c[0] == "quiet_ends"][0]
    r = ref.astype(np.float64)
    w = qr.window()
    lev = qr.frame_levels(r)
    idx = np.nonzero(lev > lev.max() - 40.0)[0]
    K = len(idx)
    c = np.zeros(128 * (K + 1))
    for n in range(len(c)):
        for j in (n // 128 - 1, n // 128):
            if 0 <= j < K:
                c[n] += w[n - 128 * j] * r[128 * idx[j] + n - 128 * j]
    ola = np.zeros(128 * (K + 1))
    for j in range(K):
        ola[128 * j:128 * j + 256] += w * r[128 * idx[j]:128 * idx[j] + 256]
    assert np.max(np.abs(c - ola)) <= 1e-15 * np.max(np.abs(ola))


# ---- STOI: known answers -----------------------------------------------------------------------------------------------------------
def _speech(seed=3, length=12000):
    return qc._speechlike(np.random.default_rng(seed), length)


def test_stoi_known_answers():
    x = _speech()
    assert abs(qr.stoi_ref(x, x) - 1.0) <= 1e-12
    assert abs(qr.stoi_ref(-x, x) - 1.0) <= 1e-12
    assert abs(qr.stoi_ref(np.zeros_like(x), x)) <= 1e-12
    rng = np.random.default_rng(11)
    nz = rng.standard_normal(len(x))
    d = [qr.stoi_ref(x + np.sqrt(np.mean(x ** 2) / np.mean(nz ** 2)) * 10 ** (-s / 20) * nz, x) for s in (20.0, 5.0, -5.0)]
    print("STOI over white noise at 20, 5, -5 dB:", d)
    assert 1.0 > d[0] > d[1] > d[2] > 0.0


def test_stoi_is_nan_below_thirty_one_kept_frames():
    x = _speech(5, 4097)
    assert len(qr.stoi_parts(x[:4096], x[:4096])[0]) == 30 and np.isnan(qr.stoi_ref(x[:4096], x[:4096]))
    assert len(qr.stoi_parts(x, x)[0]) == 31 and abs(qr.stoi_ref(x, x) - 1.0) <= 1e-12
    assert np.isnan(qr.stoi_ref(x[:200], x[:200]))


# ---- time-domain metrics: known answers --------------------------------------------------------------------------------------------
def test_time_metric_known_answers():
    n = 8000
    t = np.arange(n) / n
    r = np.sin(2 * np.pi * 10 * t)
    q = qr.quality_ref(0.5 * r, r, 240)
    assert abs(q[0] - 20 * np.log10(2.0)) <= 1e-12 and abs(q[0] - 6.0206) < 1e-4 and q[1] == np.inf
    # an orthogonal sinusoid of a tenth of the amplitude: 20 dB in every metric (frames of whole periods)
    q = qr.quality_ref(r + 0.1 * np.cos(2 * np.pi * 10 * t), r, 800)
    assert np.max(np.abs(q - 20.0)) <= 1e-9
    # ... and scaling est leaves SI-SDR alone
    assert abs(qr.quality_ref(3.0 * (r + 0.1 * np.cos(2 * np.pi * 10 * t)), r, 800)[1] - 20.0) <= 1e-9
    with np.errstate(all="ignore"):
        assert np.array_equal(qr.quality_ref(r, r, 240), [np.inf, np.inf, 35.0])                      # upper clamp
        q = qr.quality_ref(r + 100.0, r, 240)
        assert q[2] == -10.0                                                                          # lower clamp
        q = qr.quality_ref(np.ones(500), np.zeros(500), 240)
        assert q[0] == -np.inf and np.isnan(q[1])                                                     # silent reference
        assert np.isnan(qr.quality_ref(r[:100], r[:100] * 0.9, 240)[2])                               # no whole frame
        assert np.all(np.isnan(qr.quality_ref(r[:0], r[:0], 240)))
    # only whole frames count
    e = r.copy()
    e[7900:] += 1.0                                        # inside the last whole frame [7680, 7920) and the partial one behind it
    assert qr.quality_ref(e, r, 240)[2] < 35.0 and qr.quality_ref(e[:7910], r[:7910], 240)[2] == 35.0
    e = r.copy()
    e[7920:] += 1.0                                        # the trailing partial frame alone
    assert qr.quality_ref(e, r, 240)[2] == 35.0


def test_expanded_residual_loses_the_high_sdr_case():
    """What tests/test_gpu_quality.py::test_high_sdr relies on: in float32 the two-pass form stays within the floor, the expanded
    form sum e^2 - Ser^2 / Srr is off by decibels."""
    est, ref = qc.high_sdr_case()
    for i in range(est.shape[0]):
        want = qr.quality_ref(est[i], ref[i], 240)[1]
        assert 70.0 < want < 78.0
        assert abs(qr.quality_ref(est[i], ref[i], 240, np.float32)[1] - want) <= qr.BOUND["si_sdr"]
        assert not abs(qr.si_sdr_expanded_f32(est[i], ref[i]) - want) <= 0.5


def test_fixture_threshold_margins():
    for name, est, ref in qc.stoi_cases(qc.scipy_resample):
        assert qr.threshold_margin_db(ref) > 0.1, name


# ---- C ABI without a device ----------------------------------------------------------------------------------------------------------
def test_declared_and_exported():
    from audiodenoiser_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    declared = set(re.findall(r"\b(adn_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert m_count(header) == len(_lib.EXPORTED_SYMBOLS) == len(declared)


def m_count(header):
    return int(re.search(r"The (\d+) functions below", header).group(1))


def test_size_functions_and_argument_errors():
    from audiodenoiser_amd import _lib
    L = _lib.load()
    need = ctypes.c_size_t()
    for fn in (L.adn_quality_workspace_bytes, L.adn_stoi_workspace_bytes):
        assert fn(0, 8000, ctypes.byref(need)) == 1
        assert fn(1, 0, ctypes.byref(need)) == 1
        assert fn(1, 1 << 30, ctypes.byref(need)) == 1
        assert fn(1, 8000, None) == 1 and L.adn_last_error()
        assert fn(3, 8000, ctypes.byref(need)) == 0 and need.value > 0 and need.value % 16 == 0
    # six fp64 partial sums per block of 8192 samples
    for n, length in ((1, 1), (3, 8192), (3, 8193), (60, 480000)):
        assert L.adn_quality_workspace_bytes(n, length, ctypes.byref(need)) == 0
        assert need.value == n * -(-length // 8192) * 6 * 8
    # STOI: grows with the frames of the row pitch; a pitch without a frame still has its kept counts
    assert L.adn_stoi_workspace_bytes(2, 256, ctypes.byref(need)) == 0 and need.value == 16
    sizes = []
    for length in (257, 4097, 20000):
        assert L.adn_stoi_workspace_bytes(2, length, ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] < sizes[1] < sizes[2]
    frames = len(qr.frame_starts(20000))
    assert sizes[2] >= 2 * (frames * 8 + (frames - 1) * 30 * 4)

    buf = ctypes.create_string_buffer(1 << 16)              # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    assert L.adn_quality_workspace_bytes(1, 1000, ctypes.byref(need)) == 0
    assert L.adn_quality(None, p, None, 1, 1000, 240, p, need.value, p, None) == 1
    assert L.adn_quality(p, p, None, 1, 1000, 240, p, need.value, None, None) == 1
    assert L.adn_quality(p, p, None, 0, 1000, 240, p, need.value, p, None) == 1
    assert L.adn_quality(p, p, None, 1, 0, 240, p, need.value, p, None) == 1
    for seg in (15, 8193, 0, -1):
        assert L.adn_quality(p, p, None, 1, 1000, seg, p, need.value, p, None) == 1
        assert b"seg_frame" in L.adn_last_error()
    assert L.adn_quality(p, p, None, 1, 1000, 240, p, need.value - 1, p, None) == 3
    assert L.adn_quality(p, p, None, 1, 1000, 240, None, need.value, p, None) == 3
    assert L.adn_quality(p, p, None, 1, 1000, 240, p + 4, need.value, p, None) == 1 and b"aligned" in L.adn_last_error()
    assert L.adn_stoi_workspace_bytes(1, 5000, ctypes.byref(need)) == 0
    assert L.adn_stoi(None, p, None, 1, 5000, p, need.value, p, None) == 1
    assert L.adn_stoi(p, p, None, 1, 5000, p, need.value, None, None) == 1
    assert L.adn_stoi(p, p, None, 0, 5000, p, need.value, p, None) == 1
    assert L.adn_stoi(p, p, None, 1, 5000, p, need.value - 1, p, None) == 3
    assert L.adn_stoi(p, p, None, 1, 5000, p + 8, need.value, p, None) == 1 and b"aligned" in L.adn_last_error()


def test_python_surface_without_a_device():
    import torch
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd import metrics
    for name in ("snr", "si_sdr", "seg_snr", "stoi", "evaluate"):
        assert getattr(pkg, name) is getattr(metrics, name) and name in pkg.__all__
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.evaluate(torch.zeros(100), torch.zeros(100), 8000)
    with pytest.raises(ValueError, match="frame"):
        metrics._seg_frame(8000, 15)
    assert metrics._seg_frame(8000, None) == 240 and metrics._seg_frame(44100, None) == 1323
    with pytest.raises(ValueError, match="lengths"):
        metrics._host_lengths([1, 2, 3], 2, 10, "evaluate")
    with pytest.raises(ValueError, match="lengths"):
        metrics._host_lengths([1, 11], 2, 10, "evaluate")
