"""Dereverberation baseline on the device (csrc/dereverb_kernels.hip, audiodenoiser_amd/dereverb.py) against the float64
restatement in tests/dereverb_ref.py.

Bounds (derived, not tuned):
* adn_wpe, per clip: max |d_dev - d_64| <= 4 FLOOR max |d_64|.  FLOOR (dereverb_ref.FLOOR) is the error of the same statements run
  in float32 on the host over these very cases (python tests/dereverb_cases.py), never a device figure; the factor 4 is the
  project's convention.  The restatement is applied to the DOWNLOADED device spectrogram, so the STFT's own error does not enter.
* adn_wpe, per (clip, bin): E = max_t |d_dev - d_64| / max_t |d_64| <= 4 floor for every bin of every clip, beside the bound above
  (tests/solver_bounds.py).  The floor is the case's own: the largest E of the float32 restatement on the same input over every
  bin, the three clips and both orders of the sums over t (pairwise and sequential), measured when the test runs, never below
  2^-23 and never from the device.  The same bound holds the tilted cases (an 80 dB slope over the bins, built on the host and
  uploaded), and a power of two per bin, 2^-((5 b) mod 13), has to come back bit for bit as the equally scaled unscaled result.
* mag_out against |spec_out| computed in float64 from the device's own spec_out: 2 ulp (one rounding of im * im, one of the fmaf,
  one of the square root, which halves the relative error of its argument: under 1.5 ulp).
* Repeat, batch, bin-subset, pass-through and isolation tests: exact equality, as include/adn.h pins them.
* End to end: bit-identical to the public pieces composed by hand, and within the tree's inverse-STFT tolerance TOL = 1e-4 of
  max |ref| (tests/test_gpu_denoise.py::test_resynth) of denoise_ref.istft applied to the device's own spec_out.
* Quality: caps, not parity -- half of the restatement's gain and of the restatement's margin.
Measured on the MI355X: parity uses at most 1.42 of a floor (bound 4): n_fft 512, T = 97, loading 1e-6, clip 0, 4.1e-4 of max |d|;
at the defaults at most 0.34 (n_fft 64, T = 22, clip 1), the median over all cases 0.05; the inverse-STFT link 1.7e-7 - 2.1e-7 of
the maximum; SI-SDR 3.33 -> 6.54 dB, the cascade 8.79 dB against 6.49 dB for the gain alone: the restatement's, to the printed digits.
Per bin (profiles/solver_bins.md): at most 2.85 of the case's floor (bound 4): n_fft 64, T = 5, clip 0, bin 14, E 6.3e-5; the tilted
cases at most 1.35, the power-of-two case 0.83 and bit for bit; the median over the 57 runs 1.05.
The lane layouts that grid does not reach (tests/variant_cover.py: K = 19, 21, 28, 29 at T = 23 and 97, per bin only): at most
1.88 floors (K = 21, T = 23, clip 1, bin 16, E 1.8e-4), the median over the 16 runs 1.02.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref  # noqa: E402
import dereverb_cases as dc  # noqa: E402
import dereverb_ref as dr  # noqa: E402
import footprint as fp  # noqa: E402
import solver_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _spec(dev, n_fft, n_frames, n_clips):
    """The device's own STFT of the first clips of the parity audio: device complex64 (n, T, F)."""
    from audiodenoiser_amd.griffin_lim import stft_complex
    x = torch.from_numpy(dc.parity_audio(n_fft, n_frames, 3)[:n_clips].copy()).to(dev)
    spec = stft_complex(x, n_fft, n_fft // 4)
    assert spec.shape == (n_clips, n_frames, n_fft // 2 + 1)
    return spec


def _bits(t):
    """A tensor as its 32-bit words: equality of these is equality bit for bit (NaN payloads and the sign of zero included)."""
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _params(kw):
    from audiodenoiser_amd.dereverb import WpeParams
    return None if kw is None else WpeParams(**kw)


def _raw(spec, spec_out, mag_out, params=None, ws=None, ws_bytes=0, width=None, n_frames=None):
    """adn_wpe itself; returns the status."""
    from audiodenoiser_amd import _lib
    n, t, f = spec.shape
    s = torch.view_as_real(spec.contiguous())
    rc = _lib.load().adn_wpe(s.data_ptr(), n, t if n_frames is None else n_frames, f, params, ws.data_ptr() if ws is not None else None,
                             ws_bytes, spec_out.data_ptr() if spec_out is not None else None,
                             mag_out.data_ptr() if mag_out is not None else None,
                             (int(mag_out.shape[-1]) if mag_out is not None else 0) if width is None else width,
                             torch.cuda.current_stream(spec.device).cuda_stream)
    torch.cuda.synchronize(spec.device)
    return rc


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
def _parity(dev, n_fft, n_frames, kw):
    from audiodenoiser_amd.dereverb import wpe
    spec = _spec(dev, n_fft, n_frames, 3)
    bounds = sb.wpe_bounds(spec.cpu().numpy(), kw)             # the float64 restatement and the case's own float32 floor
    want = list(bounds.ref)
    worst = 0.0
    for n_clips in dc.PARITY_CLIPS:
        got, mag = wpe(spec[:n_clips].contiguous(), _params(kw))
        assert got.shape == (n_clips, n_frames, n_fft // 2 + 1) and got.dtype == torch.complex64
        assert mag.shape == (n_clips, 1, n_fft // 2 + 1, n_frames) and mag.dtype == torch.float32
        got_h, mag_h = got.cpu().numpy(), mag.cpu().numpy()[:, 0]
        for c in range(n_clips):
            err, scale = float(np.abs(got_h[c].astype(np.complex128) - want[c]).max()), float(np.abs(want[c]).max())
            share = err / scale / dr.FLOOR
            worst = max(worst, share)
            print(f"n_fft {n_fft} T {n_frames} {kw or 'defaults'} clips {n_clips} clip {c}: max err {err:.3g} = {err / scale:.3g} of "
                  f"max |d| ({share:.2f} floors; bound 4)")
            assert err <= 4.0 * dr.FLOOR * scale, (n_clips, c, err / scale)
            ref = np.sqrt(got_h[c].real.astype(np.float64) ** 2 + got_h[c].imag.astype(np.float64) ** 2).T      # (F, T)
            ulps = np.abs(mag_h[c].astype(np.float64) - ref) / np.spacing(np.maximum(ref, np.finfo(np.float32).tiny).astype(np.float32))
            assert ulps.max() <= 2.0, (n_clips, c, float(ulps.max()))
        sb.check(f"{sb.wpe_label(n_fft, n_frames, kw)} [clips {n_clips}]", got_h, bounds.ref[:n_clips], bounds)
    return worst


@pytest.mark.parametrize("n_frames", dc.PARITY_FRAMES)
@pytest.mark.parametrize("n_fft", dc.PARITY_N_FFT)
def test_parity_with_the_float64_restatement(dev, n_fft, n_frames):
    _parity(dev, n_fft, n_frames, None)


@pytest.mark.parametrize("kw", dc.EXTRA_PARAMS, ids=("smallest", "largest", "loading1e-6"))
@pytest.mark.parametrize("n_fft", dc.PARITY_N_FFT)
def test_parity_at_other_parameters(dev, n_fft, kw):
    _parity(dev, n_fft, dc.EXTRA_FRAMES, kw)


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


def _mag_within_2_ulp(got_h, mag_h):
    ref = np.sqrt(got_h.real.astype(np.float64) ** 2 + got_h.imag.astype(np.float64) ** 2).transpose(0, 2, 1)   # (n, F, T)
    ulps = np.abs(mag_h.astype(np.float64) - ref) / np.spacing(np.maximum(ref, np.finfo(np.float32).tiny).astype(np.float32))
    assert ulps.max() <= 2.0, float(ulps.max())


@pytest.mark.parametrize("n_fft,n_frames,kw", tuple(dc.variant_cases()), ids=lambda v: f"K{v['taps']}" if isinstance(v, dict) else str(v))
def test_parity_at_the_lane_layouts_the_grid_does_not_reach(dev, n_fft, n_frames, kw):
    """K = 19, 21, 28, 29 (tests/variant_cover.py): wpe_kernel<32>, and a partial last block row at every lane grouping.  Per bin
    only: dereverb_ref.FLOOR is measured over the parity grid and does not speak for these."""
    from audiodenoiser_amd.dereverb import wpe
    spec = _spec(dev, n_fft, n_frames, 3)
    bounds = sb.wpe_bounds(spec.cpu().numpy(), kw)             # the float64 restatement and the case's own float32 floor
    assert bounds.floor <= sb.VARIANT_CAP, bounds.floor
    for n_clips in dc.PARITY_CLIPS:
        got, mag = wpe(spec[:n_clips].contiguous(), _params(kw))
        assert got.shape == (n_clips, n_frames, n_fft // 2 + 1) and got.dtype == torch.complex64
        got_h = got.cpu().numpy()
        _mag_within_2_ulp(got_h, mag.cpu().numpy()[:, 0])
        sb.check(f"{sb.wpe_label(n_fft, n_frames, kw, 'variant')} [clips {n_clips}]", got_h, bounds.ref[:n_clips], bounds)


@pytest.mark.parametrize("n_fft", sb.TILTED_WPE)
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, n_fft):
    """80 dB from the first bin to the last: the clip-wide bound allows the quiet bins an error of their own size."""
    from audiodenoiser_amd.dereverb import wpe
    spec_h = sb.scale_spec(sb.wpe_spec(n_fft, sb.TILTED_FRAMES), sb.tilt(n_fft // 2 + 1))
    bounds = sb.wpe_bounds(spec_h)
    for n_clips in dc.PARITY_CLIPS:
        got, mag = wpe(_upload(dev, spec_h[:n_clips]))
        got_h = got.cpu().numpy()
        sb.check(f"{sb.wpe_label(n_fft, sb.TILTED_FRAMES, None, 'tilted')} [clips {n_clips}]", got_h, bounds.ref[:n_clips], bounds)
        _mag_within_2_ulp(got_h, mag.cpu().numpy()[:, 0])


def test_a_power_of_two_per_bin_comes_back_bit_for_bit(dev):
    """R, the taps and the weights' product with the signal are scale-free and the 1e-30 constants far below an ulp of what they
    are added to, so 2^-k times a bin's input is 2^-k times its output, exactly (tests/test_solver_bounds_host.py checks that the
    float32 restatement has the property, and here that no square leaves the normal range)."""
    from audiodenoiser_amd.dereverb import wpe
    base, f = sb.wpe_spec(64, sb.TILTED_FRAMES), sb.pow2(33)
    scaled = sb.scale_spec(base, f)
    sb.assert_squares_stay_normal(scaled)
    ft = _upload(dev, f.astype(np.float32))
    plain, plain_mag = wpe(_upload(dev, base))
    got, mag = wpe(_upload(dev, scaled))
    sb.assert_squares_stay_normal(got.cpu().numpy())
    assert _same(got, torch.view_as_complex(torch.view_as_real(plain) * ft[None, None, :, None]))
    assert _same(mag, plain_mag * ft[None, None, :, None])
    sb.check(sb.wpe_label(64, sb.TILTED_FRAMES, None, "pow2"), got.cpu().numpy(), sb.wpe_bounds(scaled).ref, sb.wpe_bounds(scaled))


# ---- 2. exact pins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (None, dc.EXTRA_PARAMS[1]), ids=("defaults", "largest"))
def test_repeat_batch_and_bin_subsets_are_exact(dev, kw):
    from audiodenoiser_amd.dereverb import wpe
    spec = _spec(dev, 512, 97, 3)
    p = _params(kw)
    full, full_mag = wpe(spec, p)
    again, again_mag = wpe(spec, p)
    assert _same(again, full) and _same(again_mag, full_mag)                       # two calls
    alone, alone_mag = wpe(spec[1:2].contiguous(), p)
    assert _same(alone[0], full[1]) and _same(alone_mag[0], full_mag[1])           # a clip alone
    for lo, hi in ((100, 133), (0, 1), (256, 257), (7, 24)):                        # bins repacked contiguous and run alone
        part, part_mag = wpe(spec[:, :, lo:hi].contiguous(), p)
        assert _same(part, full[:, :, lo:hi]) and _same(part_mag, full_mag[:, :, lo:hi]), (lo, hi)


def test_short_rows_first_frames_and_zero_rows(dev):
    from audiodenoiser_amd.dereverb import WpeParams, wpe
    for n_frames in (1, 2, 3):                                                      # T <= D: bit for bit
        spec = _spec(dev, 512, 3, 3)[:, :n_frames].contiguous()
        got, mag = wpe(spec)
        ref = torch.view_as_real(spec).double().pow(2).sum(-1).sqrt().transpose(1, 2)
        assert _same(got, spec) and bool(((mag[:, 0].double() - ref).abs() <= 2.4e-7 * ref).all())       # 2 ulp
    spec = _spec(dev, 64, 22, 3)
    assert _same(wpe(spec[:, :8].contiguous(), WpeParams(delay=8))[0], spec[:, :8])
    for delay in (1, 3, 8):                                                         # the first D frames: bit for bit
        got, _ = wpe(spec, WpeParams(delay=delay))
        assert _same(got[:, :delay], spec[:, :delay]) and not _same(got[:, delay:], spec[:, delay:])
    clean, clean_mag = wpe(spec)
    zeroed = spec.clone()
    zeroed[1, :, 17] = 0
    zeroed[2, :, 32] = 0
    got, mag = wpe(zeroed)
    assert bool((_bits(got[1, :, 17]) == 0).all()) and bool((_bits(got[2, :, 32]) == 0).all())
    assert bool((mag[1, 0, 17] == 0).all()) and bool((mag[2, 0, 32] == 0).all())
    keep = torch.ones((3, 33), dtype=torch.bool, device=dev)
    keep[1, 17] = keep[2, 32] = False
    assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])


# ---- 3. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames,kw", ((512, 65, None), (64, 5, None), (64, 70, dc.EXTRA_PARAMS[1])))
def test_footprint_only_what_the_call_owns(dev, n_fft, n_frames, kw):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import wpe
    n, f = 2, n_fft // 2 + 1
    spec = _spec(dev, n_fft, n_frames, n)
    p = _params(kw)
    ps = ctypes.byref(p.to_struct()) if p is not None else None
    plain, plain_mag = wpe(spec, p)
    need = ctypes.c_size_t(0)
    assert _lib.load().adn_wpe_workspace_bytes(n, n_frames, f, ps, ctypes.byref(need)) == 0
    ws_bytes = max(int(need.value), 4096)                     # a workspace larger than asked for is the caller's right
    width = n_frames + 7
    out, h_out = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    mag, h_mag = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    ws, h_ws = fp.carve(ws_bytes, 0xFF, dev)
    assert _raw(spec, out, mag, ps, ws, ws_bytes) == 0
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_ws, "workspace")):
        fp.assert_guards_intact(h, what)
    if need.value == 0:
        assert fp.keeps_fill(h_ws, 0xFF)                      # nothing was asked for: nothing is touched
    assert _same(torch.view_as_complex(out), plain) and _same(mag[..., :n_frames], plain_mag)
    assert bool((mag.view(torch.int32)[..., n_frames:] == -1).all())
    # mag_out = NULL, workspace = NULL when none is needed: spec_out is written, the same bits
    out2, h_out2 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    if need.value == 0:
        assert _raw(spec, out2, None, ps) == 0
    else:
        assert _raw(spec, out2, None, ps, ws, ws_bytes) == 0
    fp.assert_guards_intact(h_out2, "spec_out")
    fp.assert_guards_intact(h_mag, "mag_out")
    assert _same(out2, out)


def test_refusals_leave_every_buffer_untouched(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeParams, wpe
    spec = _spec(dev, 64, 22, 2)
    out, h_out = fp.carve_tensor((2, 22, 33, 2), 0xFF, dev)
    mag, h_mag = fp.carve_tensor((2, 1, 33, 32), 0xFF, dev)
    ws, h_ws = fp.carve(4096, 0xFF, dev)
    L = _lib.load()
    for name, value in (("taps", 0), ("taps", 33), ("delay", 0), ("delay", 9), ("iterations", 0), ("iterations", 9), ("loading", 0.0),
                        ("loading", 2.0), ("loading", float("nan")), ("power_floor", 0.0), ("power_floor", float("nan"))):
        s = WpeParams().to_struct()
        setattr(s, name, value)
        assert _raw(spec, out, mag, ctypes.byref(s), ws, 4096) == 1 and name.encode() in L.adn_last_error(), (name, value)
    assert _raw(spec, out, mag, width=21) == 1                                      # width < n_frames
    assert _raw(spec, out, mag, n_frames=0) == 1
    assert _raw(spec, None, mag) == 1
    assert _raw(spec, spec, mag) == 1                                               # spec_out may not overlap spec
    s = torch.view_as_real(spec)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for args in ((None, 2, 22, 33, None, None, 0, out.data_ptr(), mag.data_ptr(), 32), (s.data_ptr(), 0, 22, 33, None, None, 0, out.data_ptr(), mag.data_ptr(), 32),
                 (s.data_ptr(), 2, 22, 0, None, None, 0, out.data_ptr(), mag.data_ptr(), 32), (s.data_ptr() + 4, 2, 21, 33, None, None, 0, out.data_ptr(), mag.data_ptr(), 32),
                 (s.data_ptr(), 2, 22, 33, None, None, 0, out.data_ptr() + 4, mag.data_ptr(), 32), (s.data_ptr(), 2, 22, 33, None, None, 0, out.data_ptr(), mag.data_ptr() + 2, 32)):
        assert L.adn_wpe(*args, stream) == 1 and L.adn_last_error().startswith(b"adn_wpe:"), args
    torch.cuda.synchronize(dev)
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_ws, "workspace")):
        assert fp.keeps_fill(h, 0xFF), what
        fp.assert_guards_intact(h, what)
    with pytest.raises(ValueError):
        wpe(spec.cpu())
    with pytest.raises(ValueError):
        wpe(spec, mag_out=torch.zeros((2, 1, 33, 22), device=dev).transpose(2, 3))


# ---- 4. isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_a_non_finite_value_stays_in_its_own_row(dev, bad):
    from audiodenoiser_amd.dereverb import wpe
    spec = _spec(dev, 512, 70, 3)
    clean, clean_mag = wpe(spec)
    clip, bin_, frame = 1, 130, 37
    poisoned = spec.clone()
    poisoned[clip, frame, bin_] = complex(bad, 0.25)
    got, mag = wpe(poisoned)
    keep = torch.ones((3, 257), dtype=torch.bool, device=dev)
    keep[clip, bin_] = False
    assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])
    assert _same(mag[:, 0][keep], clean_mag[:, 0][keep])


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def _resynth_by_hand(dev, y, d, length):
    from audiodenoiser_amd import _lib
    out = torch.empty((d.shape[0], length), device=dev)
    _lib.check(_lib.load().adn_denoise_resynth(y.data_ptr(), torch.view_as_real(d).data_ptr(), d.shape[0], length, 512, 128,
                                               int(y.shape[3]), 0, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "adn_denoise_resynth")
    return out


@pytest.mark.parametrize("length,n_clips", ((24000, 1), (2047, 1), (100, 1), (24000, 2)))
def test_end_to_end(dev, length, n_clips):
    from audiodenoiser_amd.baseline import spectral_gain
    from audiodenoiser_amd.dereverb import Dereverberator, wpe
    from audiodenoiser_amd.griffin_lim import stft_complex
    dn = Dereverberator(dev)
    x = np.stack([dc.reverberant(32000, 50 + c)[0][8000:8000 + length] for c in range(n_clips)])       # stereo: two clips
    assert x.shape == (n_clips, length)
    xd = torch.from_numpy(x).to(dev)
    out = dn.denoise(xd)
    assert out.shape == xd.shape and out.is_cuda and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    # bit-identical to the public pieces composed by hand
    n_frames = 1 + length // 128
    spec = stft_complex(xd, 512, 128)
    y = torch.zeros((n_clips, 1, 257, max(n_frames, 16)), device=dev)
    d, _ = wpe(spec, mag_out=y)
    assert bool((y[..., n_frames:] == 0).all())
    assert torch.equal(out, _resynth_by_hand(dev, y, d, length))
    # the audio is the inverse STFT of d
    d_h, got = d.cpu().numpy().astype(np.complex128), out.cpu().numpy().astype(np.float64)
    for c in range(n_clips):
        link = denoise_ref.istft(d_h[c], 128, length)
        e = float(np.abs(got[c] - link).max() / np.abs(link).max())
        print(f"end to end L {length} clip {c}: against the float64 inverse STFT of the device's spec_out {e:.3g} (TOL {TOL})")
        assert e <= TOL
    # numpy in -> numpy out, (L,) in -> (L,) out, the same values
    one = dn.denoise(x[0])
    assert isinstance(one, np.ndarray) and one.shape == (length,) and one.dtype == np.float32
    assert np.array_equal(one, dn.denoise(xd[:1]).cpu().numpy()[0])
    # the cascade: the gain of the spectral baseline on spec_out, the phase of d
    y2 = torch.zeros_like(y)
    spectral_gain(d, out=y2)
    cascade = Dereverberator(dev, gain=True).denoise(xd)
    assert torch.equal(cascade, _resynth_by_hand(dev, y2, d, length)) and not torch.equal(cascade, out)


def test_other_rate_comes_back_at_its_length(dev):
    from audiodenoiser_amd.dereverb import Dereverberator
    x = torch.from_numpy(np.stack([dc.reverberant(32000, 60)[0][:16501]])).to(dev)
    out = Dereverberator(dev).denoise(x, sr=16000)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())


# ---- 6. file and command line ----------------------------------------------------------------------------------------------------
def test_file_and_command_line(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.dereverb import Dereverberator
    from audiodenoiser_amd.wav import read_wav, write_wav
    wet, dry = (v[:16000] for v in dc.quality_case())
    src, ref, dst, dst_cli = (str(tmp_path / n) for n in ("room.wav", "dry.wav", "out.wav", "out_cli.wav"))
    write_wav(src, wet, 8000, "PCM_16")
    write_wav(ref, dry, 8000, "PCM_16")
    assert Dereverberator(dev).denoise_file(src, dst) == (16000, 8000)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.dereverb", src, dst_cli, "--reference", ref], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert np.array_equal(read_wav(dst_cli)[0], read_wav(dst)[0])
    row = json.loads(run.stdout.strip().splitlines()[-1])
    print(f"SI-SDR of the 2 s clip: {row['noisy']['si_sdr']:.2f} -> {row['denoised']['si_sdr']:.2f} dB")
    assert row["denoised"]["si_sdr"] > row["noisy"]["si_sdr"]


# ---- 7. quality ------------------------------------------------------------------------------------------------------------------
def test_si_sdr_on_the_reverberant_clip(dev):
    from audiodenoiser_amd.baseline import SpectralDenoiser
    from audiodenoiser_amd.dereverb import Dereverberator
    from audiodenoiser_amd.metrics import evaluate
    wet, dry = dc.quality_case()
    r_in, r_wpe, r_wiener, r_cascade = dc.restatement_si_sdr()
    wd, dd = torch.from_numpy(wet.copy()).to(dev), torch.from_numpy(dry.copy()).to(dev)

    def score(audio):
        return float(evaluate(audio, dd, sr=8000)["si_sdr"][0])

    before, after = score(wd), score(Dereverberator(dev).denoise(wd))
    wiener, cascade = score(SpectralDenoiser(dev).denoise(wd)), score(Dereverberator(dev, gain=True).denoise(wd))
    print(f"SI-SDR on the device: input {before:.2f}, WPE {after:.2f}, spectral baseline {wiener:.2f}, cascade {cascade:.2f} dB "
          f"(the restatement's: {r_in:.2f}, {r_wpe:.2f}, {r_wiener:.2f}, {r_cascade:.2f})")
    assert r_wpe - r_in >= 2.0 and after - before >= 0.5 * (r_wpe - r_in)
    assert r_cascade - r_wiener >= 1.0 and cascade - wiener >= 0.5 * (r_cascade - r_wiener)


# ---- the building blocks of the window plan, which this class does not have ---------------------------------------------------------
@pytest.mark.parametrize("gain", (False, True))
def test_the_network_s_building_blocks_refuse_and_leave_the_object_usable(dev, gain):
    """No model and no window plan: what ``Denoiser`` builds around its network says so (a ``RuntimeError``, the stream variants'
    sentence) before it looks at its argument, and the object dereverberates afterwards as before."""
    from audiodenoiser_amd.dereverb import Dereverberator
    dn = Dereverberator(dev, gain=gain)
    y = torch.zeros((1, 1, 33, 16), device=dev)
    spec = torch.zeros((1, 3, 33), dtype=torch.complex64, device=dev)
    for call in (lambda: dn.network(y), lambda: dn.windows(spec), lambda: dn.plan(40),
                 lambda: dn.denoise_spectrogram(torch.zeros((33, 16), device=dev)), lambda: dn.stitch(y, 1, 16, False),
                 lambda: dn.resynth(y, spec, 600)):
        with pytest.raises(RuntimeError, match=r"^Dereverberator: there is no network"):
            call()
    clip = np.random.default_rng(600).uniform(-0.5, 0.5, 600).astype(np.float32)
    out = dn.denoise(clip)
    assert out.shape == (600,) and out.dtype == np.float32 and np.isfinite(out).all()
