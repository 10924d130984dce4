"""Streaming spectral baseline without a device: the float64 equivalence of the stream of steps with the offline restatement, the
recorded float32 floor of the magnitude form, the C ABI of adn_spectral_gain_windows (declared, exported, every refusal -- made
with host pointers that are never dereferenced) and the Python classes' argument checks."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_ref as br  # noqa: E402
import baseline_stream_cases as sc  # noqa: E402
import denoise_ref  # noqa: E402
import stream_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "adn_spectral_gain_windows"


# ---- the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", sc.BLOCKS)
@pytest.mark.parametrize("length", sc.LENGTHS)
def test_float64_stream_of_steps_equals_the_offline_restatement(length, block):
    """stream_ref.denoise with the magnitude form on the kept columns in the network's place against baseline_ref.denoise: the
    same recurrence over the same frames, m = |X| handed over in place of X -- sqrt(p)^2 against p, an ulp of float64.  Measured
    4e-16 of the maximum; asserted at 1e-12."""
    x = sc.e2e_audio(length).astype(np.float64)
    got = stream_ref.denoise(x, sc.gain_net(block), sc.N_FFT, sc.HOP, sc.window_of(block), block, 0)
    want = br.denoise(x, sc.N_FFT, sc.HOP)
    assert got.shape == want.shape == (length,)
    e = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"L {length} B {block}: {e:.3g} of the maximum")
    assert e <= 1e-12


def test_magnitude_form_is_the_operator_on_m_plus_0i():
    """In float32 the magnitude form is NOT the offline gain of the same spectrogram in the last bits (sqrtf(p)^2 != p), and it is
    within the floors of it."""
    spec = denoise_ref.stft(sc.e2e_audio(2047), sc.N_FFT, sc.HOP).astype(np.complex64)
    offline, _ = br.spectral_gain(spec, dtype=np.float32)
    m = np.abs(spec).astype(np.float32)
    windows, _ = br.spectral_gain(m.astype(np.complex64), dtype=np.float32)
    assert not np.array_equal(offline, windows)
    assert np.abs(offline.astype(np.float64) - windows).max() <= 4 * (br.FLOOR + sc.FLOOR_WINDOWS) * float(offline.max())


def test_floor_windows_is_recorded_and_reproduced():
    assert 0 < sc.FLOOR_WINDOWS < 1e-4
    measured = sc.measure_floor()
    print(f"FLOOR_WINDOWS {sc.FLOOR_WINDOWS:g}, measured {measured:.4g}")
    assert abs(measured - sc.FLOOR_WINDOWS) <= 0.05 * sc.FLOOR_WINDOWS        # written with two digits
    assert sc.FLOOR_WINDOWS <= 10.0 * br.FLOOR


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_loadable():
    from audiodenoiser_amd import _lib
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    assert f"ADN_API int {NAME}(" in header and NAME in _lib.EXPORTED_SYMBOLS
    L = _lib.load()
    fn = getattr(L, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert re.search(r"^#define ADN_SPECTRAL_MAX_ROWS 256$", header, flags=re.M)
    assert re.search(r"typedef struct adn_spectral_row \{ int slot; int fresh; \} adn_spectral_row;", header)
    assert ctypes.sizeof(_lib.SpectralRow) == 8 and [n for n, _ in _lib.SpectralRow._fields_] == ["slot", "fresh"]
    from audiodenoiser_amd import baseline
    assert baseline.SPECTRAL_MAX_ROWS == 256
    internal = open(os.path.join(ROOT, "audiodenoiser_amd", "csrc", "adn_internal.h")).read()
    assert re.search(r"constexpr int SPECTRAL_MAX_ROWS = 256;", internal)


def _rows(*pairs):
    from audiodenoiser_amd import _lib
    return (_lib.SpectralRow * len(pairs))(*[_lib.SpectralRow(*p) for p in pairs])


def test_every_refusal_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import SpectralParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(4096)                  # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def call(windows=p, y=p, n_rows=2, n_steps=3, f=8, w=16, col0=12, n_cols=4, params=None, state=p, n_slots=4, rows=None):
        return L.adn_spectral_gain_windows(windows, y, n_rows, n_steps, f, w, col0, n_cols, params, state, n_slots, rows, None)

    many = _rows(*[(i, 0) for i in range(257)])
    cases = (dict(windows=None), dict(y=None), dict(state=None),                                   # null pointers
             dict(windows=p + 2), dict(y=p + 1), dict(state=p + 3),                                # misaligned ones
             dict(n_rows=0), dict(n_steps=0), dict(f=0), dict(w=0), dict(n_cols=0), dict(n_slots=0), dict(n_rows=-1),
             dict(col0=-1), dict(col0=13), dict(col0=0, n_cols=17), dict(col0=1 << 30, n_cols=1 << 30, w=1 << 30),
             dict(n_rows=5), dict(n_rows=5, n_slots=4),                                            # more rows than slots, no table
             dict(n_rows=257, n_slots=1000, rows=many),                                            # a table of more than 256 rows
             dict(rows=_rows((0, 0), (4, 0))), dict(rows=_rows((-1, 1), (0, 0))),                  # a slot outside [0, n_slots)
             dict(rows=_rows((3, 0), (3, 1))),                                                     # a slot named twice
             dict(n_steps=1 << 16, n_cols=1 << 15, col0=0, w=1 << 15),                             # n_steps x n_cols = 2^31
             dict(n_rows=1 << 30, n_slots=1 << 30, f=65))                                          # the grid: 2^31 workgroups
    for kw in cases:
        assert call(**kw) == 1, kw
        assert L.adn_last_error().startswith(NAME.encode() + b":"), (kw, L.adn_last_error())
    for name, value in (("smooth", 1.0), ("beta", -0.5), ("alpha", 1.0), ("gamma", 0.0), ("gain_floor", 0.0), ("bias", 100.5),
                        ("bias", float("nan")), ("gamma", float("inf"))):
        s = SpectralParams().to_struct()
        setattr(s, name, value)
        assert call(params=ctypes.byref(s)) == 1
        assert L.adn_last_error().startswith(NAME.encode() + b":") and name.encode() in L.adn_last_error(), (name, value)


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def test_names_are_exported_lazily():
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd import baseline, stream
    for name in ("StreamSpectralDenoiser", "SpectralStreamPool", "spectral_gain_windows"):
        assert getattr(pkg, name) is getattr(baseline, name) and name in pkg.__all__ and name in baseline.__all__
    assert issubclass(baseline.StreamSpectralDenoiser, stream.StreamDenoiser)
    assert issubclass(baseline.SpectralStreamPool, stream.StreamPool)


def test_constructors_validate_without_a_device():
    from audiodenoiser_amd.baseline import SpectralStreamPool, StreamSpectralDenoiser
    for kw in (dict(n_streams=0), dict(n_fft=500), dict(n_fft=32), dict(hop_length=0), dict(hop_length=129), dict(block_frames=0),
               dict(block_frames=2.0), dict(sample_rate=0), dict(input_rate=0), dict(input_rate=44100.0)):
        with pytest.raises(ValueError, match="StreamSpectralDenoiser"):
            StreamSpectralDenoiser("cpu", **kw)
    for kw in (dict(max_streams=0), dict(backlog_steps=0), dict(n_fft=500), dict(hop_length=129), dict(block_frames=0),
               dict(sample_rate=0), dict(input_rates=(0,))):
        with pytest.raises(ValueError, match="StreamPool"):
            SpectralStreamPool("cpu", **kw)
    for cls in (StreamSpectralDenoiser, SpectralStreamPool):
        with pytest.raises(TypeError, match=cls.__name__):
            cls("cpu", params={"bias": 2.0})
        with pytest.raises(RuntimeError, match="no CPU path"):
            cls("cpu")


def test_spectral_gain_windows_checks_its_arguments():
    import torch
    from audiodenoiser_amd.baseline import spectral_gain_windows
    with pytest.raises(ValueError, match="spectral_gain_windows"):
        spectral_gain_windows(torch.zeros(2, 1, 33, 16), torch.zeros(2, 3, 33), 12, 4)         # not on a device
    with pytest.raises(ValueError, match="spectral_gain_windows"):
        spectral_gain_windows(np.zeros((2, 1, 33, 16), np.float32), None, 12, 4)


def test_poolbook_yields_fresh_exactly_at_step_0_after_a_slot_is_reused():
    """The pool's row table is (slot, step == 0): a stream's first step and no other one, in a slot that an earlier stream has
    left without a reset as well."""
    from audiodenoiser_amd.stream import PoolBook
    book = PoolBook(max_streams=2, backlog_steps=4, n_fft=512, hop_length=128, window_frames=16, block_frames=4, lookahead_frames=0)
    per, seen = 4 * 128, []

    def tick():
        rows = book.rows()
        seen.extend((slot, step, step == 0) for slot, step, _ in rows)
        for slot, _, _ in rows:
            book.ran(slot)
        return rows

    a = book.open()
    book.take(a, book.end_of(0) + 2 * per)                   # three steps' samples, one step per tick
    assert [tick() for _ in range(3)] == [[(a, 0, -1)], [(a, 1, -1)], [(a, 2, -1)]] and tick() == []
    b = book.open()
    book.take(b, book.end_of(0))
    assert tick() == [(b, 0, -1)]
    book.close(a)
    while tick():
        pass
    assert book.status[a] == book.FREE
    again = book.open()
    assert again == a, "the lowest free slot: the first stream's, reused without a reset"
    book.take(again, book.end_of(1))
    assert tick() == [(again, 0, -1)] and tick() == [(again, 1, -1)]
    fresh = [(slot, step) for slot, step, f in seen if f]
    assert fresh == [(a, 0), (b, 0), (a, 0)] and all(f == (step == 0) for _, step, f in seen)
