"""Host-side checks of the resampler inside a stream (no GPU): adn_resample_stream_plan / _state_bytes against the float64
restatement in tests/stream_resample_ref.py, the argument checks of adn_resample_stream, the composed plan of a StreamDenoiser
with an input rate, the Python refusals, and the restatement's own sanity."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_resample_ref as ref  # noqa: E402

ADN_ERR_INVALID, ADN_ERR_WORKSPACE = 1, 3
PAIRS = ((44100, 8000), (8000, 44100), (48000, 8000), (8000, 48000), (16000, 8000), (44100, 48000), (3, 2), (22050, 8000))


@pytest.fixture(scope="module")
def lib():
    from audiodenoiser_amd import _lib
    return _lib.load()


def _plan(lib, src, dst, received, final=0):
    e, h, lat = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    assert lib.adn_resample_stream_plan(src, dst, received, final, ctypes.byref(e), ctypes.byref(h), ctypes.byref(lat)) == 0
    return e.value, h.value, lat.value


@pytest.mark.parametrize("src,dst", PAIRS)
def test_plan_against_restatement(lib, src, dst):
    up, down = ref.ratio(src, dst)
    half = ref.half_of(up, down)
    h_want, lat_want = ref.history(src, dst), ref.latency(src, dst)
    assert h_want == 2 * (half // up) + -(-down // up) + 1 and lat_want == -(-half // up)
    prev, carried = 0, 0
    length = ctypes.c_long()
    for n in range(3001):
        e, h, lat = _plan(lib, src, dst, n)
        assert (e, h, lat) == (ref.emitted(n, src, dst), h_want, lat_want), n
        assert e >= prev and e <= -(-n * up // down)                           # never goes back, never past the finished length
        prev = e
        if e:
            assert 0 <= ref.last_input(e - 1, src, dst) < n, n                 # the last emitted output reads only i < n
        assert ref.last_input(e, src, dst) >= n, n                             # the next one reads some i >= n
        assert n * up - e * down <= half, n                                    # the latency inequality
        carried = max(carried, n - max(ref.first_input(e, src, dst), 0))       # what the next output still needs of the past
        if n:
            assert lib.adn_resample_length(n, src, dst, ctypes.byref(length)) == 0
            assert _plan(lib, src, dst, n, 1)[0] == length.value == ref.emitted(n, src, dst, True)
    assert _plan(lib, src, dst, 0, 1)[0] == 0
    assert carried <= h_want, (carried, h_want)
    # any output pointer may be NULL
    assert lib.adn_resample_stream_plan(src, dst, 100, 0, None, None, None) == 0


def test_equal_rates_are_the_identity(lib):
    for rate in (8000, 44100, 1):
        for n in (0, 1, 7, 3000):
            assert _plan(lib, rate, rate, n) == (n, 0, 0) and _plan(lib, rate, rate, n, 1) == (n, 0, 0)
    v = ctypes.c_size_t(1)
    assert lib.adn_resample_stream_state_bytes(4, 8000, 8000, ctypes.byref(v)) == 0 and v.value == 0
    from audiodenoiser_amd.resample import resample_stream_plan
    assert resample_stream_plan(123, 8000, 8000) == (123, 0, 0)
    assert resample_stream_plan(1000, 48000, 8000) == (ref.emitted(1000, 48000, 8000), 385 + 6, 192)
    assert resample_stream_plan(1000, 48000, 8000, final=True)[0] == 167


def test_state_bytes_are_linear_in_the_streams(lib):
    v = ctypes.c_size_t()
    for src, dst in PAIRS:
        assert lib.adn_resample_stream_state_bytes(1, src, dst, ctypes.byref(v)) == 0
        one = v.value
        assert one == 2 * 4 * ref.history(src, dst) and one % 8 == 0
        for n in (2, 3, 16, 256):
            assert lib.adn_resample_stream_state_bytes(n, src, dst, ctypes.byref(v)) == 0 and v.value == n * one
    # the audio pair with the longest filter stays far below the limit
    assert ref.history(192000, 8000) == 1561 <= 16384


@pytest.mark.parametrize("rate", (48000, 44100, 16000))
@pytest.mark.parametrize("plan", ((512, 128, 48, 8, 4), (512, 128, 192, 16, 0)))
def test_rate_plan_composition(rate, plan):
    from audiodenoiser_amd.resample import resample_stream_plan
    from audiodenoiser_amd.stream import stream_plan, stream_rate_plan
    n_fft, hop, w, b, a = plan
    up, down = ref.ratio(rate, 8000)
    latency = -(-(2 * ref.half_of(up, down) + ((b + a - 1) * hop + n_fft) * down) // up)
    if rate == 48000 and plan == (512, 128, 192, 16, 0):
        assert latency == 14976
    prev = 0
    for n in list(range(0, 40000, 37)) + [40000, 100000, 1 << 20]:
        e, lat = stream_rate_plan(n, rate, *plan)
        assert lat == latency
        at_work = resample_stream_plan(n, rate, 8000)[0]
        assert e == resample_stream_plan(stream_plan(at_work, *plan)[1], 8000, rate)[0]
        assert prev <= e <= n, n                                               # never goes back, never ahead of the input
        if e:
            assert n - e <= latency, (n, e)
        prev = e
    assert prev > 0


def test_bad_calls_launch_nothing(lib):
    """Every refusal below comes from the argument checks, before any HIP call: the pointers are host memory."""
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    v = ctypes.c_size_t()
    assert lib.adn_resample_stream_state_bytes(2, 48000, 8000, ctypes.byref(v)) == 0

    def call(state=ptr, nbytes=big, audio=ptr, audio_stride=0, n_streams=1, call_index=0, before=0, n_new=480, final=0, src=48000,
             dst=8000, out=ptr, out_stride=0):
        return lib.adn_resample_stream(state, nbytes, audio, audio_stride, n_streams, call_index, before, n_new, final, src, dst, out,
                                       out_stride, None)

    for kw in (dict(src=0), dict(dst=0), dict(src=-8000), dict(src=4097, dst=1), dict(src=1, dst=4097),       # adn_resample's limits
               dict(src=4096, dst=1),                                                                       # H = 266 241 > 16384
               dict(n_streams=0), dict(n_new=0), dict(n_new=-1), dict(n_new=-1, final=1), dict(final=2),
               dict(call_index=-1), dict(call_index=0, before=480), dict(call_index=1, before=0),
               dict(call_index=1, before=1 << 31), dict(call_index=1, before=(1 << 31) - 100, n_new=100),    # input positions
               dict(src=8000, dst=48000, call_index=1, before=1 << 29),                                     # output positions
               dict(state=None), dict(audio=None), dict(out=None, n_new=480),
               dict(n_streams=2, audio_stride=479, out_stride=80), dict(n_streams=2, audio_stride=480, out_stride=10),
               dict(audio_stride=-1), dict(out_stride=-1)):
        assert call(**kw) == ADN_ERR_INVALID, kw
        assert b"adn_resample_stream" in lib.adn_last_error(), kw
    assert call(src=4096, dst=1) == ADN_ERR_INVALID and b"16384" in lib.adn_last_error()
    assert call(n_streams=2, audio_stride=480, out_stride=80, nbytes=v.value - 1) == ADN_ERR_WORKSPACE
    assert b"adn_resample_stream_state_bytes" in lib.adn_last_error()
    for src, dst in ((0, 8000), (4096, 1)):
        assert lib.adn_resample_stream_plan(src, dst, 10, 0, None, None, None) == ADN_ERR_INVALID
        assert lib.adn_resample_stream_state_bytes(1, src, dst, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_resample_stream_plan(48000, 8000, -1, 0, None, None, None) == ADN_ERR_INVALID
    assert lib.adn_resample_stream_plan(48000, 8000, 10, 2, None, None, None) == ADN_ERR_INVALID
    assert lib.adn_resample_stream_state_bytes(0, 48000, 8000, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_resample_stream_state_bytes(1, 48000, 8000, None) == ADN_ERR_INVALID
    # 1:4096 upsamples with a short filter per output: it can be streamed
    assert lib.adn_resample_stream_state_bytes(1, 1, 4096, ctypes.byref(v)) == 0 and v.value == 2 * 4 * 66


def test_python_refusals():
    """Checked before any device is touched."""
    import torch
    from audiodenoiser_amd import StreamDenoiser, StreamResampler
    from audiodenoiser_amd.model import UNet
    for args in ((0, 8000), (8000, 0), (-1, 8000), (48000.0, 8000)):
        with pytest.raises(ValueError, match="rates"):
            StreamResampler(*args)
    with pytest.raises(ValueError, match="n_streams"):
        StreamResampler(48000, 8000, n_streams=0)
    rs = StreamResampler(48000, 8000, n_streams=2)
    assert rs.latency_samples == 192 and rs.received == 0 and rs.emitted == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        rs.push(torch.zeros((2, 480)))
    cpu = UNet(1, 1).eval()
    for bad in (0, -8000, 48000.0):
        with pytest.raises(ValueError, match="input_rate"):
            StreamDenoiser(cpu, input_rate=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        StreamDenoiser(cpu, input_rate=48000)


def test_restatement_sanity():
    """For every pair and a dozen split patterns the concatenated pushes equal resample_ref of the whole to 1e-12."""
    assert len(ref.split_patterns(1501, 0)) >= 12
    assert ref.sanity() <= 1e-12


def test_restatement_streams_shorter_than_the_latency():
    for src, dst in ((48000, 8000), (44100, 8000)):
        for length in (1, 100):
            x = np.random.default_rng([src, dst, length]).uniform(-1.0, 1.0, length)
            s = ref.StreamRef(src, dst)
            first = s.push(x)
            assert len(first) == ref.emitted(length, src, dst) == 0            # shorter than the latency: all comes from flush
            got = s.flush()
            want = ref.resample_ref.resample_ref(x, src, dst)[0]
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
