"""Streaming denoiser on the device (csrc/stream_kernels.hip, audiodenoiser_amd/stream.py) against the float64 restatement in
tests/stream_ref.py.

Bounds (the tree's own, none tuned here):
* windows: the tree's transform tolerance TOL = 1e-4 of max |ref| against the restatement applied to denoise_ref.stft of the whole
  signal (test_gpu_denoise / test_istft_and_complex_stft_match_oracle); padded frames, before 0 and from T on, exactly zero.
* round trip with the analysis windows in place of the network's output: the tree's round-trip figures on uniform [-1, 1] audio,
  1e-5 absolute, and 6e-5 over the last `hop` samples where the window sum-of-squares falls from 1.5 to as little as 0.26
  (test_gpu_denoise.test_resynth).
* end to end: TOL of max |ref| in fp32 with the same device network as the restatement's callable; 1e-2 in fp16 against the
  fp32 device network (the U-Net's fp16 bound, test_gpu_parity.py).
* split invariance, stream independence, reuse: bit for bit with model.set_batch_invariant(True); without it the U-Net's
  documented per-batch-size bound, 2e-5 of the maximum in fp32 (UNet.set_batch_invariant).
Measured on the MI355X, worst over all cases: windows 2.1e-7 of the maximum, round trip 3.6e-7 (body) / 2.4e-7 (last hop samples)
absolute, end to end 4.6e-6 (fp32) / 2.0e-3 (fp16) of the maximum, splits without batch invariance 2.0e-6 of the maximum.
The plans here are n_fft 64, 256 and 512 at hop = n_fft / 4; the other sizes, a hop that does not divide n_fft and bounds per frame
and per sample (not of the maximum) are tests/test_gpu_spectral_grid.py's.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref  # noqa: E402
import stream_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
PLANS = ((512, 128, 64, 16, 0), (512, 128, 48, 8, 4), (256, 64, 32, 16, 16), (64, 16, 16, 1, 0))     # n_fft, hop, W, B, A
N_STREAMS = 3


def lengths(hop, block):
    return (10007, 24000, block * hop, hop - 1, 1)


CASES = [p + (length,) for p in PLANS for length in lengths(p[1], p[3])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _net(weights_np, dev, dtype="f32"):
    from audiodenoiser_amd.model import UNet
    m = UNet(1, 1)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights_np.items()}, strict=True)
    return m.to(dev).eval().set_compute_dtype(dtype)


@pytest.fixture(scope="module")
def net(weights_np, dev):
    m = _net(weights_np, dev)
    yield m
    m._workspace = None


@pytest.fixture(scope="module")
def net16(weights_np, dev):
    m = _net(weights_np, dev, "f16")
    yield m
    m._workspace = None


def _sd(net, plan, n_streams=N_STREAMS, **kw):
    from audiodenoiser_amd import StreamDenoiser
    n_fft, hop, w, b, a = plan
    return StreamDenoiser(net, n_streams=n_streams, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b,
                          lookahead_frames=a, **kw)


_AUDIO = {}


def _audio(dev, plan, length, n_streams=N_STREAMS):
    """Uniform [-1, 1] audio seeded from the parameters, made once per case and left unchanged."""
    key = plan + (length, n_streams)
    if key not in _AUDIO:
        x = np.random.default_rng(list(plan) + [length]).uniform(-1.0, 1.0, (n_streams, length)).astype(np.float32)
        x.setflags(write=False)
        _AUDIO[key] = x
    return _AUDIO[key], torch.from_numpy(_AUDIO[key].copy()).to(dev)


def _drive(sd, xd, fn, chunks=(1, 3, 8, 2)):
    """Every step of a finished stream through adn_stream_analyze / adn_stream_emit themselves, `fn` in the network's place, in
    calls of changing size: the steps the arrived samples allow while the stream runs, the rest with the final length.
    -> windows (n_streams, K, F, W), audio (n_streams, L)."""
    n_fft, hop, w, b, a = sd.n_fft, sd.hop_length, sd.window_frames, sd.block_frames, sd.lookahead_frames
    n, length = xd.shape
    running = ref.steps_done(length, n_fft, hop, b, a)
    total = ref.n_steps(1 + length // hop, b)
    assert running <= total
    sd.reset()
    wins, outs, k, i = [], [], 0, 0
    while k < total:
        final = -1 if k < running else length
        m = min(chunks[i % len(chunks)], sd.max_steps, (running if k < running else total) - k)
        base = 0 if k == 0 else (k * b + a - 1) * hop + n_fft // 2        # e(k - 1): where the call's new samples start
        src = xd[:, base:] if base < length else xd
        win = sd.analyze(src, length, k, m, final)
        assert win.shape == (n * m, 1, n_fft // 2 + 1, w)
        wins.append(win.view(n, m, n_fft // 2 + 1, w))
        out = sd.emit(fn(win), k, m, final)
        assert out.shape == (n, sd.emit_count(k, m, final))
        outs.append(out)
        k, i = k + m, i + 1
    sd.reset()
    return torch.cat(wins, dim=1), torch.cat(outs, dim=1)


_DRIVEN = {}


def _driven(dev, net, plan, length):
    """The identity drive of a case, computed once and shared by the windows and the round-trip test."""
    key = plan + (length,)
    if key not in _DRIVEN:
        _, xd = _audio(dev, plan, length)
        win, out = _drive(_sd(net, plan, batch_windows=24), xd, lambda t: t)
        _DRIVEN[key] = (win.cpu().numpy(), out.cpu().numpy())
    return _DRIVEN[key]


@pytest.mark.parametrize("n_fft,hop,w,b,a,length", CASES)
def test_windows_against_restatement(dev, net, n_fft, hop, w, b, a, length):
    plan = (n_fft, hop, w, b, a)
    x, _ = _audio(dev, plan, length)
    got, _ = _driven(dev, net, plan, length)
    n_frames = 1 + length // hop
    k = ref.n_steps(n_frames, b)
    assert got.shape == (N_STREAMS, k, n_fft // 2 + 1, w) and got.dtype == np.float32
    first = np.arange(k)[:, None] * b + b + a - w + np.arange(w)[None, :]            # frame of (step, local frame)
    pad = (first < 0) | (first >= n_frames)
    worst = 0.0
    for c in range(N_STREAMS):
        want = ref.windows(np.abs(denoise_ref.stft(x[c], n_fft, hop)), w, b, a)
        e = float(np.abs(got[c] - want).max() / np.abs(want).max())
        worst = max(worst, e)
        assert e <= TOL, (c, e)
        assert np.all(got[c].transpose(0, 2, 1)[pad] == 0.0)
    print(f"windows n_fft {n_fft} W {w} B {b} A {a} L {length}: K {k}, {int(pad.sum())} padded frames, error {worst:.3g} of the maximum")


@pytest.mark.parametrize("n_fft,hop,w,b,a,length", CASES)
def test_round_trip_without_the_network(dev, net, n_fft, hop, w, b, a, length):
    plan = (n_fft, hop, w, b, a)
    x, _ = _audio(dev, plan, length)
    _, back = _driven(dev, net, plan, length)
    assert back.shape == (N_STREAMS, length) and back.dtype == np.float32
    err = np.abs(back.astype(np.float64) - x)
    body, tail = err[:, :max(length - hop, 0)], err[:, max(length - hop, 0):]
    e_body, e_tail = float(body.max()) if body.size else 0.0, float(tail.max())
    print(f"round trip n_fft {n_fft} W {w} B {b} A {a} L {length}: body {e_body:.3g} tail {e_tail:.3g}")
    assert e_body <= 1e-5 and e_tail <= 6e-5


def _device_net(model, dev):
    """The device network as the restatement's callable: (K, F, W) float64 -> (K, F, W) float64, 64 windows at a time."""
    def call(win):
        x = torch.from_numpy(win.astype(np.float32)).to(dev)[:, None]
        with torch.no_grad():
            y = torch.cat([model(x[i:i + 64]) for i in range(0, x.shape[0], 64)])
        return y[:, 0].cpu().numpy().astype(np.float64)
    return call


@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("n_fft,hop,w,b,a,length", CASES)
def test_end_to_end(dev, net, net16, dtype, n_fft, hop, w, b, a, length):
    plan = (n_fft, hop, w, b, a)
    x, xd = _audio(dev, plan, length)
    sd = _sd(net if dtype == "f32" else net16, plan)
    assert sd.latency_samples == ref.latency(n_fft, hop, b, a)
    first = sd.push(xd)
    assert first.is_cuda and first.shape == (N_STREAMS, ref.emitted(length, n_fft, hop, b, a))
    assert sd.received == length and sd.emitted == first.shape[1]
    rest = sd.flush()
    assert sd.received == 0 and sd.emitted == 0
    got = torch.cat([first, rest], dim=1)
    assert got.shape == (N_STREAMS, length) and torch.isfinite(got).all()
    got = got.cpu().numpy().astype(np.float64)
    call = _device_net(net, dev)                                 # the fp32 device network in both cases
    tol = TOL if dtype == "f32" else 1e-2
    worst = 0.0
    for c in range(N_STREAMS):
        want = ref.denoise(x[c].astype(np.float64), call, n_fft, hop, w, b, a)
        e = float(np.abs(got[c] - want).max() / np.abs(want).max())
        worst = max(worst, e)
        assert e <= tol, (c, e)
    print(f"end to end {dtype} n_fft {n_fft} W {w} B {b} A {a} L {length}: {worst:.3g} of the maximum (allowed {tol:g})")


def _pushes(sd, xd, sizes):
    """Push `xd` in blocks of the given sizes (the last one cut), flush; check the count of every push.
    -> audio, the number of steps each push completed."""
    plan = (sd.n_fft, sd.hop_length, sd.block_frames, sd.lookahead_frames)
    length, pos, outs, steps = xd.shape[1], 0, [], []
    for size in sizes:
        if pos >= length:
            break
        size = min(size, length - pos)
        before = ref.emitted(pos, *plan)
        out = sd.push(xd[:, pos:pos + size])
        steps.append(ref.steps_done(pos + size, *plan) - ref.steps_done(pos, *plan))
        pos += size
        assert out.shape == (xd.shape[0], ref.emitted(pos, *plan) - before), (pos, size)
        assert sd.received == pos and sd.emitted == ref.emitted(pos, *plan)
        outs.append(out)
    assert pos == length
    outs.append(sd.flush())
    out = torch.cat(outs, dim=1)
    assert out.shape == xd.shape
    return out, steps


def _random_sizes(plan, length):
    """Seeded blocks of 1 ... 3000 samples, every third one of 1 ... 7: pushes that complete no step and pushes that complete several."""
    rng = np.random.default_rng(list(plan) + [length, 77])
    sizes = []
    while sum(sizes) < length:
        sizes.append(int(rng.integers(1, 8)) if len(sizes) % 3 == 1 else int(rng.integers(1, 3001)))
    return sizes


@pytest.mark.parametrize("n_fft,hop,w,b,a", PLANS)
def test_split_invariance(dev, net, n_fft, hop, w, b, a):
    plan, length = (n_fft, hop, w, b, a), 10007
    _, xd = _audio(dev, plan, length)
    sd = _sd(net, plan)
    net.set_batch_invariant(True)
    try:
        whole, s1 = _pushes(sd, xd, [length])
        by_1000, s2 = _pushes(sd, xd, [1000] * 11)
        rand, s3 = _pushes(sd, xd, _random_sizes(plan, length))
        steps = s1 + s2 + s3
        assert min(steps) == 0 and max(steps) >= 2 and min(s3) == 0, steps     # pushes that complete no step, pushes that complete several
        assert torch.equal(whole, by_1000) and torch.equal(whole, rand)
        assert torch.isfinite(whole).all()
        # a push of nothing returns nothing and changes nothing
        assert sd.push(xd[:, :0]).shape == (N_STREAMS, 0) and sd.received == 0
    finally:
        net.set_batch_invariant(False)
    loose_whole, _ = _pushes(sd, xd, [length])
    loose_rand, _ = _pushes(sd, xd, _random_sizes(plan, length))
    e = float((loose_rand - loose_whole).abs().max() / loose_whole.abs().max())
    print(f"split n_fft {n_fft} W {w} B {b} A {a}: without batch invariance {e:.3g} of the maximum (allowed 2e-5)")
    assert e <= 2e-5


@pytest.mark.parametrize("n_fft,hop,w,b,a", PLANS[1:3])
def test_stream_independence_and_reuse(dev, net, n_fft, hop, w, b, a):
    plan, length = (n_fft, hop, w, b, a), 10007
    x, xd = _audio(dev, plan, length)
    net.set_batch_invariant(True)
    try:
        sd = _sd(net, plan)
        whole, _ = _pushes(sd, xd, [length])
        # stream 0 alone in a batch of one: the same bits
        alone, _ = _pushes(_sd(net, plan, n_streams=1), xd[:1].clone(), [3000] * 4)
        assert torch.equal(alone[0], whole[0])
        # a stream holding a NaN sample leaves its neighbours alone
        bad = xd.clone()
        bad[1, 5000] = float("nan")
        with_nan, _ = _pushes(sd, bad, [4096] * 3)
        assert torch.isnan(with_nan[1]).any()
        assert torch.equal(with_nan[0], whole[0]) and torch.equal(with_nan[2], whole[2])
        # reuse: nothing of the poisoned stream is left after flush(); reset() in the middle of a stream does the same
        again, _ = _pushes(sd, xd, [1000] * 11)
        assert torch.equal(again, whole)
        sd.push(bad[:, :7000])
        sd.reset()
        assert sd.received == 0 and sd.emitted == 0
        after_reset, _ = _pushes(sd, xd, [length])
        assert torch.equal(after_reset, whole)
        # numpy in -> numpy out; (m,) for one stream
        one = _sd(net, plan, n_streams=1)
        out = np.concatenate([one.push(x[0, :6000]), one.push(x[0, 6000:]), one.flush()], axis=1)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(out[0], whole[0].cpu().numpy())
        with pytest.raises(ValueError, match="n_streams"):
            sd.push(x[:2])
    finally:
        net.set_batch_invariant(False)


def test_command_line_feeds_a_file_in_chunks(dev, net, weights_np, tmp_path):
    """main() in this process (no second interpreter): a stereo 8 kHz file, every channel a stream, equals push / flush by hand."""
    from audiodenoiser_amd import stream
    from audiodenoiser_amd.wav import read_wav, write_wav
    x, _ = _audio(dev, (512, 128, 48, 8, 4), 10007, 2)
    src, dst, ckpt = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "ckpt.pth")
    write_wav(src, np.ascontiguousarray(0.5 * x.T), 8000, "FLOAT")
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in weights_np.items()}, ckpt)
    assert stream.main(["--model", ckpt, "--window", "48", "--block", "8", "--lookahead", "4", "--chunk", "1000", src, dst]) == 0
    got, rate = read_wav(dst, mono=False)
    assert rate == 8000 and got.shape == (10007, 2)
    samples, _ = read_wav(src, mono=False)
    sd = _sd(net, (512, 128, 48, 8, 4), n_streams=2)
    xd = torch.from_numpy(np.ascontiguousarray(samples.T)).to(dev)
    want, _ = _pushes(sd, xd, [1000] * 11)
    want = (np.clip(np.rint(want.cpu().numpy() * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)     # write_wav's PCM_16 rounding
    assert np.array_equal(got.T, want)
