"""Streaming denoiser, the parts that need no device: adn_stream_plan / adn_stream_state_bytes against tests/stream_ref.py, the
argument checks of the adn_stream_* entry points, the constructor refusals of StreamDenoiser and the restatement's own sanity."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref  # noqa: E402
import stream_ref as ref  # noqa: E402

PLANS = ((512, 128, 192, 16, 0), (512, 128, 48, 8, 4), (256, 64, 32, 16, 16), (64, 16, 16, 1, 0), (256, 32, 40, 3, 5),
         (512, 128, 32, 32, 0))        # n_fft, hop, W, B, A
ADN_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from audiodenoiser_amd import _lib
    return _lib.load()


def _plan(lib, n_fft, hop, w, b, a, received):
    s, e, lat = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    assert lib.adn_stream_plan(n_fft, hop, w, b, a, received, ctypes.byref(s), ctypes.byref(e), ctypes.byref(lat)) == 0
    return s.value, e.value, lat.value


@pytest.mark.parametrize("n_fft,hop,w,b,a", PLANS)
def test_plan_equals_restatement(lib, n_fft, hop, w, b, a):
    prev = 0
    for m in range(0, 3 * (b + a) * hop + 2 * n_fft + 1):
        steps, out, lat = _plan(lib, n_fft, hop, w, b, a, m)
        assert steps == ref.steps_done(m, n_fft, hop, b, a), m
        assert out == ref.emitted(m, n_fft, hop, b, a), m
        assert lat == ref.latency(n_fft, hop, b, a) == (b + a - 1) * hop + n_fft
        assert out >= prev, m                                   # emitted never goes back
        prev = out
        if steps:
            assert m - out <= lat, m                            # a sample waits at most `latency` samples once a step has run
        assert out <= m
    # the first step runs exactly when frame B + A - 1 is complete
    first = (b + a - 1) * hop + n_fft // 2
    assert _plan(lib, n_fft, hop, w, b, a, first - 1)[0] == 0 and _plan(lib, n_fft, hop, w, b, a, first)[0] == 1


def test_plan_outputs_are_optional(lib):
    s = ctypes.c_long()
    assert lib.adn_stream_plan(512, 128, 192, 16, 0, 100000, ctypes.byref(s), None, None) == 0
    assert s.value == ref.steps_done(100000, 512, 128, 16, 0)


@pytest.mark.parametrize("n_fft,hop,w,b,a", PLANS)
def test_state_bytes(lib, n_fft, hop, w, b, a):
    def size(n_streams, max_steps):
        v = ctypes.c_size_t()
        assert lib.adn_stream_state_bytes(n_streams, n_fft, hop, w, b, a, max_steps, ctypes.byref(v)) == 0
        return v.value
    one = size(1, 4)
    assert one > 0
    for n in (2, 3, 16, 256):
        assert size(n, 4) == n * one                            # linear in the number of streams
    sizes = [size(3, s) for s in (1, 2, 3, 8, 64)]
    assert all(x <= y for x, y in zip(sizes, sizes[1:]))        # non-decreasing in max_steps
    # at least the magnitudes of the last W frames and the n_fft - hop shared samples
    assert size(1, 1) >= 4 * (w * (n_fft // 2 + 1) + n_fft - hop)


BAD_PLANS = {
    "B + A > W": (512, 128, 32, 24, 9),
    "hop > n_fft / 4": (512, 129, 192, 16, 0),
    "hop < 1": (512, 0, 192, 16, 0),
    "n_fft not a power of two": (500, 100, 192, 16, 0),
    "n_fft too large": (8192, 128, 192, 16, 0),
    "window < 16": (512, 128, 15, 8, 0),
    "block < 1": (512, 128, 192, 0, 0),
    "lookahead < 0": (512, 128, 192, 16, -1),
}


@pytest.mark.parametrize("why", sorted(BAD_PLANS))
def test_bad_plans_are_refused_everywhere(lib, why):
    p = BAD_PLANS[why]
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    v, s = ctypes.c_size_t(), ctypes.c_long()
    calls = (lambda: lib.adn_stream_plan(*p, 1000, ctypes.byref(s), None, None),
             lambda: lib.adn_stream_state_bytes(1, *p, 4, ctypes.byref(v)),
             lambda: lib.adn_stream_reset(ptr, 1 << 40, 1, *p, 4, None),
             lambda: lib.adn_stream_analyze(ptr, 1 << 40, ptr, 0, 1, 0, 1, -1, *p, 4, ptr, None),
             lambda: lib.adn_stream_emit(ptr, 1 << 40, ptr, 1, 0, 1, -1, *p, 4, ptr, 0, None))
    for call in calls:
        assert call() == ADN_ERR_INVALID, why
        assert b"adn_stream_" in lib.adn_last_error() and b"block + lookahead <= window" in lib.adn_last_error()


def test_bad_calls_launch_nothing(lib):
    """Every refusal below comes from the argument checks, before any HIP call: the pointers are host memory."""
    good = (512, 128, 192, 16, 0)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    v = ctypes.c_size_t()
    assert lib.adn_stream_state_bytes(1, *good, 4, ctypes.byref(v)) == 0
    big = 1 << 40

    def analyze(first=0, n_steps=1, final=-1, max_steps=4, n_streams=1, state=ptr, audio=ptr, out=ptr, nbytes=big):
        return lib.adn_stream_analyze(state, nbytes, audio, 0, n_streams, first, n_steps, final, *good, max_steps, out, None)

    def emit(first=0, n_steps=1, final=-1, max_steps=4, n_streams=1, state=ptr, y=ptr, nbytes=big):
        return lib.adn_stream_emit(state, nbytes, y, n_streams, first, n_steps, final, *good, max_steps, ptr, 0, None)

    for call in (analyze, emit):
        assert call(n_steps=5) == ADN_ERR_INVALID and b"max_steps" in lib.adn_last_error()            # n_steps > max_steps
        assert call(n_steps=0) == ADN_ERR_INVALID
        assert call(first=-1) == ADN_ERR_INVALID
        assert call(max_steps=0) == ADN_ERR_INVALID
        assert call(max_steps=1 << 17) == ADN_ERR_INVALID
        assert call(n_streams=0) == ADN_ERR_INVALID
        assert call(state=None) == ADN_ERR_INVALID and b"null" in lib.adn_last_error()
        # 32-bit positions inside the kernels: steps that reach sample 2^30, and step counts beyond any stream
        assert call(first=(1 << 30) // (16 * 128)) == ADN_ERR_INVALID and b"2^30" in lib.adn_last_error()
        assert call(first=1 << 40) == ADN_ERR_INVALID
        assert call(final=0) == ADN_ERR_INVALID and b"final_length" in lib.adn_last_error()
        assert call(final=-2) == ADN_ERR_INVALID
        assert call(final=1 << 30) == ADN_ERR_INVALID
        # a stream of 1000 samples has T = 8 frames, K = 1 step: step 1 does not exist
        assert call(first=1, final=1000) == ADN_ERR_INVALID and b"last step" in lib.adn_last_error()
        assert call(nbytes=v.value - 1) == 3 and b"adn_stream_state_bytes" in lib.adn_last_error()     # ADN_ERR_WORKSPACE
    assert analyze(audio=None) == ADN_ERR_INVALID and analyze(out=None) == ADN_ERR_INVALID
    assert emit(y=None) == ADN_ERR_INVALID
    assert lib.adn_stream_reset(None, big, 1, *good, 4, None) == ADN_ERR_INVALID
    assert lib.adn_stream_reset(ptr, 16, 1, *good, 4, None) == 3
    assert lib.adn_stream_state_bytes(0, *good, 4, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_stream_state_bytes(1, *good, 0, ctypes.byref(v)) == ADN_ERR_INVALID
    assert lib.adn_stream_state_bytes(1, *good, 4, None) == ADN_ERR_INVALID
    assert lib.adn_stream_plan(*good, -1, None, None, None) == ADN_ERR_INVALID


def test_constructor_refusals():
    """Checked before any device is touched: a model on the CPU stands in for one on the device."""
    import torch  # noqa: F401
    from audiodenoiser_amd import StreamDenoiser
    from audiodenoiser_amd.model import UNet
    cpu = UNet(1, 1).eval()
    for kw in (dict(n_fft=500), dict(n_fft=32), dict(hop_length=129), dict(hop_length=0), dict(window_frames=15),
               dict(block_frames=0), dict(lookahead_frames=-1), dict(window_frames=32, block_frames=24, lookahead_frames=9),
               dict(n_streams=0), dict(batch_windows=0), dict(sample_rate=0)):
        with pytest.raises(ValueError):
            StreamDenoiser(cpu, **kw)
    with pytest.raises(ValueError, match="UNet"):
        StreamDenoiser(object())
    with pytest.raises(ValueError, match="UNet"):
        StreamDenoiser(UNet(2, 1).eval())
    with pytest.raises(RuntimeError, match="train mode"):
        StreamDenoiser(UNet(1, 1).train())
    with pytest.raises(RuntimeError, match="no CPU path"):
        StreamDenoiser(cpu)


@pytest.mark.parametrize("n_fft,hop,w,b,a", PLANS)
@pytest.mark.parametrize("length", (10007, 1, 300))
def test_restatement_identity_network(n_fft, hop, w, b, a, length):
    """The windows hand every frame to exactly one step; with the network replaced by the identity the input comes back."""
    x = np.random.default_rng([n_fft, w, length]).uniform(-1.0, 1.0, length)
    seen = []

    def net(win):
        seen.append(win.shape)
        return win
    y = ref.denoise(x, net, n_fft, hop, w, b, a)
    n_frames = 1 + length // hop
    assert seen == [(-(-n_frames // b), n_fft // 2 + 1, w)]
    assert y.shape == (length,)
    assert np.abs(y - x).max() <= 1e-12
    # the join is the inverse of the windows on the frames a step keeps
    mag = np.abs(denoise_ref.stft(x, n_fft, hop))
    assert np.array_equal(ref.join(ref.windows(mag, w, b, a), n_frames, w, b, a, clamp=False), mag.T)
