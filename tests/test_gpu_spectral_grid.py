"""Every spectral entry point at all seven n_fft and every hop class against the float64 definitions of include/adn.h, with LOCAL
bounds: tests/spectral_ref.py holds the cases, the references, the scales and the float32 host floors.

Bound, everywhere it is not stated otherwise:  |device - ref64| <= 4 floor(entry, n_fft) scale, element by element, and exactly
zero where the scale is zero (silent frames, padded frames of the windows, samples whose only window tap is w[0] = 0 at
hop = n_fft).  floor is the worst error of two float32 host forms of the same operation over the same cases in units of the same
scale, 4 the project's margin over a host floor (tests/quality_ref.py::BOUND); nothing here is sized from device output.  Inputs
change level from frame to frame by up to 2^-12, so a quiet frame that picks up a loud neighbour's values (a stale LDS slot, a
frame index off by one at a pass or span boundary, a gather from the wrong frame) misses its own bound by orders of magnitude where
the tree's global 1e-4 of max |ref| would pass it.

Departures from 4 floor scale:
* Griffin-Lim with 1 and 3 iterations: the tree's 1e-4 of max |ref| per clip (test_gpu_parity); no local bound is derived for
  the projection loop.  Iteration 0 is under the inverse bound.
* Denoiser.stitch: test_gpu_denoise's derived 4 eps sum_k a_k |y_k| (a weight, two products and a sum, one rounding each).
* stft_magnitude_fit, repeated calls, a clip alone against the clip in its batch, pushes against calls, the pool against the solo
  stream: bit equality.

Every test walks all cases of its (entry, n_fft), prints the largest share of the bound it saw (profiles/spectral_grid.md) and
asserts at the end, naming every case that missed with its worst element.  test_gpu_denoise.py and test_gpu_stream.py keep the
network, the fp16 path and the command lines; this file has the sizes and hops they leave out, with an elementwise map in the
network's place.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dref  # noqa: E402
import spectral_ref as sp  # noqa: E402
import stream_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TOL = 1e-4
N = sp.N_CLIPS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    """Denoiser, StreamDenoiser and StreamPool ask for a network; the elementwise map runs in its place."""
    from audiodenoiser_amd.model import UNet
    return UNet(1, 1).eval().to(dev)


def _to(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)


def _h(t):
    t = t.cpu().numpy()
    return t.astype(np.complex128 if np.iscomplexobj(t) else np.float64)


_MAP = {}


def _fn(x):
    """y = x * gain + offset on the device, (.., F, width) with spectral_ref.gain_offset's float32 values."""
    key = (x.shape[-2], x.shape[-1], x.device)
    if key not in _MAP:
        g, o = sp.gain_offset(x.shape[-2], x.shape[-1])
        _MAP[key] = (torch.from_numpy(g).to(x.device), torch.from_numpy(o).to(x.device))
    g, o = _MAP[key]
    return x * g + o


def _done(entry, n_fft, worst, failures):
    print(f"share {entry} n_fft {n_fft}: {worst:.3f} of the bound (floor {sp.floor(entry, n_fft):.3g})")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_stft_magnitude(dev, n_fft):
    from audiodenoiser_amd.stft import stft_magnitude
    worst, failures = 0.0, []
    for center in (True, False):
        for hop, length, t in sp.forward_cases(n_fft, center):
            x = sp.audio(n_fft, hop, length)
            got = stft_magnitude(_to(dev, x), n_fft, hop, center)
            assert got.shape == (N, n_fft // 2 + 1, t) and got.dtype == torch.float32
            got = _h(got).transpose(0, 2, 1)
            for c in range(N):
                ref, scale = np.abs(sp.stft64(x[c], n_fft, hop, center)), sp.forward_scale(x[c], n_fft, hop, center)[:, None]
                worst = max(worst, sp.check(got[c], ref, scale, "stft_magnitude", n_fft, f"center {center} hop {hop} L {length} clip {c}", failures))
    _done("stft_magnitude", n_fft, worst, failures)


@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_stft_complex(dev, n_fft):
    from audiodenoiser_amd.griffin_lim import stft_complex
    worst, failures = 0.0, []
    for hop, length, t in sp.forward_cases(n_fft, True):
        x = sp.audio(n_fft, hop, length)
        got = stft_complex(_to(dev, x), n_fft, hop)
        assert got.shape == (N, t, n_fft // 2 + 1) and got.dtype == torch.complex64
        got = _h(got)
        for c in range(N):
            ref, scale = sp.stft64(x[c], n_fft, hop), sp.forward_scale(x[c], n_fft, hop)[:, None]
            worst = max(worst, sp.check(got[c], ref, scale, "stft_complex", n_fft, f"hop {hop} L {length} clip {c}", failures))
    _done("stft_complex", n_fft, worst, failures)


@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_stft_magnitude_fit_is_the_two_step_form(dev, n_fft):
    """On the clips of test_stft_magnitude: bit-equal to quantize_pad_on_device(stft_magnitude(...)), a window larger than the
    spectrogram in one direction or both and a window that crops."""
    from audiodenoiser_amd.data_loader import quantize_pad_on_device
    from audiodenoiser_amd.stft import stft_magnitude, stft_magnitude_fit
    bad = []
    for center in (True, False):
        for hop, length, _ in sp.forward_cases(n_fft, center):
            xd = _to(dev, sp.audio(n_fft, hop, length))
            mag = stft_magnitude(xd, n_fft, hop, center)
            for target in ((n_fft // 2 + 1, 32), (n_fft // 2 - 3, 12)):
                if not torch.equal(stft_magnitude_fit(xd, target, n_fft, hop, center), quantize_pad_on_device(mag, target)):
                    bad.append((center, hop, length, target))
    assert not bad, bad


@pytest.mark.parametrize("n_fft", sorted(sp.MAX_HOP))
def test_hop_limit(dev, n_fft):
    """stft_mag_kernel stages the audio span of a batch of frames in LDS (spectral_ref.MAX_HOP re-derives the limit from launch_m):
    the largest hop that fits matches the reference (it is one of test_stft_magnitude's cases too), the next one is refused with
    AdnError (no kernel is launched), and the device goes on working."""
    from audiodenoiser_amd._lib import AdnError
    from audiodenoiser_amd.stft import stft_magnitude, stft_magnitude_fit
    hop = sp.MAX_HOP[n_fft]
    worst, failures = 0.0, []
    for center in (True, False):
        (length, t), = [(length, t) for h, length, t in sp.forward_cases(n_fft, center) if h == hop]
        x = sp.audio(n_fft, hop, length)
        xd = _to(dev, x)
        before = stft_magnitude(xd, n_fft, hop, center)
        with pytest.raises(AdnError, match="hop too large"):
            stft_magnitude(xd, n_fft, hop + 1, center)
        with pytest.raises(AdnError, match="hop too large"):
            stft_magnitude_fit(xd, (n_fft // 2 + 1, 32), n_fft, hop + 1, center)
        after = stft_magnitude(xd, n_fft, hop, center)
        torch.cuda.synchronize(dev)
        assert torch.equal(before, after) and after.shape == (N, n_fft // 2 + 1, t)
        got = _h(after).transpose(0, 2, 1)
        for c in range(N):
            ref, scale = np.abs(sp.stft64(x[c], n_fft, hop, center)), sp.forward_scale(x[c], n_fft, hop, center)[:, None]
            worst = max(worst, sp.check(got[c], ref, scale, "stft_magnitude", n_fft, f"center {center} hop {hop} L {length} clip {c}", failures))
    _done("stft_magnitude", n_fft, worst, failures)


# ---------------------------------------------------------------------------------------------------------------------- inverse
@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_istft(dev, n_fft):
    from audiodenoiser_amd.griffin_lim import istft
    worst, failures = 0.0, []
    for hop, t in sp.istft_cases(n_fft):
        z = sp.spectra(n_fft, hop, t)
        got = istft(_to(dev, z), hop)
        assert got.shape == (N, hop * (t - 1)) and got.dtype == torch.float32
        got = _h(got)
        for c in range(N):
            z64 = z[c].astype(np.complex128)
            worst = max(worst, sp.check(got[c], sp.istft64(z64, hop), sp.inverse_scale(z64, hop, hop * (t - 1)), "istft", n_fft,
                                        f"hop {hop} T {t} clip {c}", failures))
    _done("istft", n_fft, worst, failures)


@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_griffin_lim(dev, n_fft):
    from audiodenoiser_amd.griffin_lim import griffin_lim_reconstruction
    worst, worst_loop, failures = 0.0, 0.0, []
    for hop, t in sp.gl_cases(n_fft):
        mag, rnd = sp.gl_input(n_fft, hop, t)
        magd, rndd = _to(dev, mag), _to(dev, rnd)
        for iterations in sp.GL_ITERATIONS:
            got = griffin_lim_reconstruction(magd, n_fft, hop, iterations, rand=rndd)
            assert got.shape == (N, hop * (t - 1)) and got.dtype == torch.float32
            got = _h(got)
            for c in range(N):
                what = f"hop {hop} T {t} iterations {iterations} clip {c}"
                if iterations == 0:
                    hat = sp.polar64(mag[c], rnd[c])
                    worst = max(worst, sp.check(got[c], sp.istft64(hat, hop), sp.inverse_scale(hat, hop, hop * (t - 1)), "griffin_lim", n_fft,
                                                what, failures))
                else:
                    ref = sp.griffin_lim64(mag[c], rnd[c], n_fft, hop, iterations)
                    e = float(np.abs(got[c] - ref).max() / np.abs(ref).max())
                    worst_loop = max(worst_loop, e)
                    if not e <= TOL:
                        failures.append(f"griffin_lim n_fft {n_fft} {what}: {e:.3g} of the maximum (allowed {TOL:g})")
    print(f"griffin_lim n_fft {n_fft}: 1 and 3 iterations {worst_loop:.3g} of the maximum (allowed {TOL:g})")
    _done("griffin_lim", n_fft, worst, failures)


# ---------------------------------------------------------------------------------------------------------------------- denoiser
@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_denoiser(dev, model, n_fft):
    """windows: the forward bound, against the restatement applied to the downloaded device spectrum as in test_gpu_denoise.py and
    against the float64 STFT of the audio (which is what checks the transform at these hops); stitch (clamped): 4 eps sum_k a_k
    |y_k|; resynth: the inverse bound against denoise_ref.resynth fed the device's y and the device's spectrum."""
    from audiodenoiser_amd import Denoiser
    from audiodenoiser_amd.griffin_lim import stft_complex
    n_bins = n_fft // 2 + 1
    w_win, w_stitch, w_out, failures = 0.0, 0.0, 0.0, []
    for w, v, hop, length in sp.denoise_cases(n_fft):
        dn = Denoiser(model, n_fft=n_fft, hop_length=hop, window_frames=w, overlap_frames=v)
        x = sp.audio(n_fft, hop, length)
        spec = stft_complex(_to(dev, x), n_fft, hop)
        t = 1 + length // hop
        k, width = dref.plan(t, w, v)
        win = dn.windows(spec)
        assert win.shape == (N * k, 1, n_bins, width)
        y = _fn(win)
        out = dn.resynth(y, spec, length)
        assert out.shape == (N, length) and out.dtype == torch.float32
        assert torch.equal(out, dn.resynth(y, spec, length)), (w, v, hop, length)
        alone = dn.resynth(y[k:2 * k].clone(), spec[1:2].clone(), length)
        assert torch.equal(alone[0], out[1]), (w, v, hop, length)
        stitched = _h(dn.stitch(y, N, t, True))
        spec_h, win_h, out_h = _h(spec), _h(win).reshape(N, k, n_bins, width), _h(out)
        y_h = _h(y).reshape(N, k, n_bins, width)
        first = sp.denoise_first(t, w, v)
        for c in range(N):
            what = f"W {w} V {v} hop {hop} L {length} clip {c}"
            wscale = sp.windows_scale(sp.forward_scale(x[c], n_fft, hop), (k, n_bins, width), first)
            w_win = max(w_win, sp.check(win_h[c], dref.windows(np.abs(spec_h[c]), w, v), wscale, "denoise_windows", n_fft, what + " (device spectrum)", failures),
                        sp.check(win_h[c], dref.windows(np.abs(dref.stft(x[c], n_fft, hop)), w, v), wscale, "denoise_windows", n_fft, what, failures))
            want, sum_abs = dref.stitch(y_h[c], t, w, v, clamp=True, with_sum_abs=True)
            share = float((np.abs(stitched[c] - want) / np.maximum(4.0 * EPS * sum_abs, 1e-300)).max())
            w_stitch = max(w_stitch, share)
            if not share <= 1.0:
                failures.append(f"denoise_stitch n_fft {n_fft} {what}: {share:.3f} of 4 eps sum a |y|")
            hat = dref.rephase(want, spec_h[c])
            w_out = max(w_out, sp.check(out_h[c], dref.resynth(y_h[c], spec_h[c], length, hop, w, v), sp.inverse_scale(hat, hop, length),
                                        "denoise_resynth", n_fft, what, failures))
    print(f"share denoise_stitch n_fft {n_fft}: {w_stitch:.3f} of 4 eps sum a |y|")
    print(f"share denoise_windows n_fft {n_fft}: {w_win:.3f} of the bound (floor {sp.floor('denoise_windows', n_fft):.3g})")
    _done("denoise_resynth", n_fft, w_out, failures)


# ---------------------------------------------------------------------------------------------------------------------- stream
def _drive(sd, xd, chunks=(1, 3, 8, 2)):
    """test_gpu_stream.py's scheme: every step of a finished stream through adn_stream_analyze / adn_stream_emit themselves, the map
    in the network's place, in calls of 1, 3, 8 and 2 steps: the steps the arrived samples allow while the stream runs, the rest
    with the final length.  -> windows (n, K, F, W), y (n, K, F, W), audio (n, L)."""
    n_fft, hop, w, b, a = sd.n_fft, sd.hop_length, sd.window_frames, sd.block_frames, sd.lookahead_frames
    n, length = xd.shape
    running = sref.steps_done(length, n_fft, hop, b, a)
    total = sref.n_steps(1 + length // hop, b)
    assert running <= total
    sd.reset()
    wins, ys, outs, k, i = [], [], [], 0, 0
    while k < total:
        final = -1 if k < running else length
        m = min(chunks[i % len(chunks)], sd.max_steps, (running if k < running else total) - k)
        base = 0 if k == 0 else (k * b + a - 1) * hop + n_fft // 2        # e(k - 1): where the call's new samples start
        src = xd[:, base:] if base < length else xd
        win = sd.analyze(src, length, k, m, final)
        assert win.shape == (n * m, 1, n_fft // 2 + 1, w)
        y = _fn(win)
        out = sd.emit(y, k, m, final)
        assert out.shape == (n, sd.emit_count(k, m, final))
        wins.append(win.view(n, m, n_fft // 2 + 1, w))
        ys.append(y.view(n, m, n_fft // 2 + 1, w))
        outs.append(out)
        k, i = k + m, i + 1
    sd.reset()
    return torch.cat(wins, dim=1), torch.cat(ys, dim=1), torch.cat(outs, dim=1)


@pytest.mark.parametrize("n_fft", sp.N_FFTS)
def test_stream(dev, model, n_fft):
    """windows under the forward bound and audio under the inverse bound against stream_ref fed the float64 STFT of the signal and
    the device's y; the same signal through push() in uneven pieces and flush() gives the same bits."""
    from audiodenoiser_amd import StreamDenoiser
    w_win, w_out, failures = 0.0, 0.0, []
    for w, b, a, hop, length in sp.stream_cases(n_fft):
        sd = StreamDenoiser(model, n_streams=N, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a,
                            batch_windows=24)
        assert sd.max_steps == 8
        x = sp.audio(n_fft, hop, length)
        xd = _to(dev, x)
        win, y, out = _drive(sd, xd)
        t = 1 + length // hop
        assert out.shape == (N, length) and win.shape == (N, sref.n_steps(t, b), n_fft // 2 + 1, w)
        sd.network = _fn
        pushed, pos = [], 0
        for m in (1, n_fft // 2 + 3, 7 * n_fft + 1, 0, 5 * hop, length):          # uneven pieces; the last takes the rest
            pushed.append(sd.push(xd[:, pos:pos + m]))
            pos = min(pos + m, length)
        pushed.append(sd.flush())
        assert torch.equal(torch.cat(pushed, dim=1), out), (w, b, a, hop, length)
        win_h, y_h, out_h = _h(win), _h(y), _h(out)
        first = sp.stream_first(t, w, b, a)
        for c in range(N):
            what = f"W {w} B {b} A {a} hop {hop} L {length} clip {c}"
            spec = dref.stft(x[c], n_fft, hop)
            wscale = sp.windows_scale(sp.forward_scale(x[c], n_fft, hop), win_h[c].shape, first)
            w_win = max(w_win, sp.check(win_h[c], sref.windows(np.abs(spec), w, b, a), wscale, "stream_windows", n_fft, what, failures))
            hat = dref.rephase(sref.join(y_h[c], t, w, b, a), spec)
            w_out = max(w_out, sp.check(out_h[c], sref.resynth(y_h[c], spec, length, hop, w, b, a), sp.inverse_scale(hat, hop, length),
                                        "stream_audio", n_fft, what, failures))
    print(f"share stream_windows n_fft {n_fft}: {w_win:.3f} of the bound (floor {sp.floor('stream_windows', n_fft):.3g})")
    _done("stream_audio", n_fft, w_out, failures)


@pytest.mark.parametrize("n_fft", (128, 4096))
def test_stream_pool_is_the_solo_stream(dev, model, n_fft):
    """Three slots of different lengths, opened at different ticks: each returns, bit for bit, what StreamDenoiser(n_streams=1)
    returns for the same samples (the map in the network's place is the same for every window, whatever batch it is in)."""
    from audiodenoiser_amd import StreamDenoiser, StreamPool
    hop, (w, b, a) = n_fft // 4, sp.STREAM_PLANS[0]
    lengths = (20 * n_fft + 37, 9 * n_fft + 2, 2 * hop - 1)                      # slot 2 opens late and ends first
    xd = _to(dev, sp.audio(n_fft, hop, lengths[0]))
    pool = StreamPool(model, max_streams=3, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a)
    pool.network = _fn
    got, sent, open_at, sids = {s: [] for s in range(3)}, [0, 0, 0], (0, 0, 3), {}
    for tick in range(400):
        for s in range(3):
            if tick == open_at[s]:
                sids[s] = pool.open()
            if s in sids and sent[s] < lengths[s]:
                m = min((s + 1) * hop + 5 * (tick % 3), lengths[s] - sent[s], pool.room(sids[s]))
                pool.push(sids[s], xd[s, sent[s]:sent[s] + m])
                sent[s] += m
                if sent[s] == lengths[s]:
                    pool.close(sids[s])
        ran = pool.step()
        for sid, samples, _ in ran:
            got[sid].append(samples)
        if not ran and all(sent[s] == lengths[s] for s in range(3)):
            break
    for s in range(3):
        solo = StreamDenoiser(model, n_streams=1, n_fft=n_fft, hop_length=hop, window_frames=w, block_frames=b, lookahead_frames=a)
        solo.network = _fn
        want = torch.cat([solo.push(xd[s:s + 1, :lengths[s]].contiguous()), solo.flush()], dim=1)[0]
        mine = torch.cat(got[sids[s]])
        assert mine.shape == (lengths[s],) and torch.equal(mine, want), (n_fft, s)
