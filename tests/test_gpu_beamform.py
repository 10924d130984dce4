"""The beamformer on the device (csrc/beamform_kernels.hip, audiodenoiser_amd/beamform.py) against the float64 restatement in
tests/beamform_ref.py.

Bounds (derived, not tuned):
* adn_mvdr, per group: max |Y_dev - Y_64| <= 4 floor max |Y_64|.  The floors are the error of the same statements run in float32 on
  the host over these very cases (python tests/beamform_cases.py), never a device figure; the factor 4 is the project's convention.
  The cases with fewer frames than channels (rank-deficient covariances) and the one at loading 1e-6 are held to beamform_ref.FLOOR,
  which they set; every other case to the six times smaller FLOOR_FULL_RANK.  The restatement is applied to the DOWNLOADED device
  spectrogram and the DOWNLOADED device mask magnitudes, so neither the STFT's nor the gain's own error enters.
* adn_mvdr, per (group, bin): E = max_t |Y_dev - Y_64| / max_t |Y_64| <= 4 floor for every bin of every group, beside the bound
  above (tests/solver_bounds.py).  The floor is the case's own: the largest E of the float32 restatement on the same inputs over
  every bin, the three groups, both reference channels and both orders of the sums over t (pairwise and sequential), measured
  when the test runs, never below 2^-23 and never from the device.  The same bound holds the tilted cases (an 80 dB slope over
  the bins of the spectrograms and of the mask magnitudes, built on the host and uploaded), and a power of two per bin,
  2^-((5 b) mod 13), has to come back bit for bit as the equally scaled unscaled result.
* mag_out against sqrtf(fmaf(re, re, im * im)) of the device's own spec_out, evaluated in float32 on the host: equal bit for bit.
* Repeat, batch, bin-subset, pitch, one-channel, zero-group and isolation tests: exact equality, as include/adn.h pins them.
* End to end: bit-identical to the public pieces composed by hand; SI-SDR within the quality cap of tests/test_gpu_dereverb.py (at
  least half of the restatement's gain over the input).
Measured on the MI355X: parity uses at most 0.69 of a floor among the full-rank cases (bound 4): n_fft 64, T = 2, C = 2, ref 1,
3.4e-5 of max |Y|; 0.66 of FLOOR among the rank-deficient ones (T = 1, C = 8, ref 7, 2.1e-4 of max |Y|); 0.01 of FLOOR at loading
1e-6; the median over all 212 comparisons 0.05.  SI-SDR of the class 1.62 -> 4.74 dB at C = 2 and 1.62 -> 7.77 dB at C = 4: the
restatement's, to the printed digits.
Per bin (profiles/solver_bins.md): at most 2.34 of the case's floor (bound 4): n_fft 64, T = 23, C = 2, ref 0, group 1, bin 15,
E 4.4e-6; the tilted cases at most 2.04, the power-of-two cases 1.75 and bit for bit; the median over the 118 runs 0.90.
The instantiations that grid does not reach (tests/variant_cover.py: C = 4, 6, 7 over the parity frames, C = 6 at reference
channel 3, per bin only): at most 3.03 floors (C = 7, T = 97, ref 0, group 2, bin 1, E 7.6e-6 on a floor of 2.5e-6), 3.00 at ref 6;
the median over the 62 runs 0.89.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import dereverb_ref as dr  # noqa: E402
import footprint as fp  # noqa: E402
import solver_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu

PIN_CHANNELS = (2, 3, 4, 5, 7, 8)                          # 4 and 8 lanes per bin; 1, 2, 3, 2, 4 and 5 triangle entries per lane


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _inputs(dev, n_fft, n_frames, channels, extra=None, n_groups=3):
    """The device's own STFT of the parity recordings, complex64 (n_groups * channels, T, F), and the mask magnitudes
    (n_groups * channels, 1, F, T + extra columns): the device's spectral gain of every channel, or the seeded uniform ones."""
    from audiodenoiser_amd.baseline import spectral_gain
    from audiodenoiser_amd.griffin_lim import stft_complex
    extra = extra or {}
    x = torch.from_numpy(bc.parity_audio(n_fft, n_frames, channels)[:n_groups * channels].copy()).to(dev)
    spec = stft_complex(x, n_fft, n_fft // 4)
    f = n_fft // 2 + 1
    assert spec.shape == (n_groups * channels, n_frames, f)
    mag = torch.full((n_groups * channels, 1, f, n_frames + extra.get("mag_extra", 0)), float("nan"), device=dev)
    if extra.get("uniform_mask"):
        spec_h = spec.cpu().numpy().reshape(n_groups, channels, n_frames, f)
        m = np.concatenate([bc.uniform_magnitudes(spec_h[g], 5) for g in range(n_groups)])
        mag[..., :n_frames] = torch.from_numpy(m).to(dev)[:, None]
    else:
        spectral_gain(spec, out=mag)
    return spec, mag


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _params(kw):
    from audiodenoiser_amd.beamform import MvdrParams
    return None if kw is None else MvdrParams(**kw)


def _raw(spec, mag, channels, spec_out, mag_out, params=None, ws=None, ws_bytes=0, spec_ptr=None):
    """adn_mvdr itself; returns the status."""
    from audiodenoiser_amd import _lib
    n, t, f = spec.shape
    s = torch.view_as_real(spec.contiguous())
    rc = _lib.load().adn_mvdr(s.data_ptr() if spec_ptr is None else spec_ptr, mag.data_ptr(), int(mag.shape[-1]), n // channels, channels,
                              t, f, params, ws.data_ptr() if ws is not None else None, ws_bytes,
                              spec_out if isinstance(spec_out, int) else spec_out.data_ptr(),
                              (mag_out if isinstance(mag_out, int) else mag_out.data_ptr()) if mag_out is not None else None,
                              t + 7 if isinstance(mag_out, int) else int(mag_out.shape[-1]) if mag_out is not None else 0,
                              torch.cuda.current_stream(spec.device).cuda_stream)
    torch.cuda.synchronize(spec.device)
    return rc


def _mag_of(y):
    """sqrtf(fmaf(re, re, im * im)) of a complex64 array, in float32."""
    return np.sqrt(dr._power(y, np.float32))


# ---- 1. parity, 2. magnitudes ----------------------------------------------------------------------------------------------------
def _parity(dev, n_fft, n_frames, channels, extra):
    from audiodenoiser_amd.beamform import mvdr
    floor, f = bc.floor_for(n_frames, channels, extra), n_fft // 2 + 1
    spec, mag = _inputs(dev, n_fft, n_frames, channels, extra)
    # the float64 restatement at both reference channels and the case's own float32 floor
    bounds = sb.mvdr_bounds(spec.cpu().numpy(), mag.cpu().numpy()[:, 0], channels, bc.params_of(extra, 0))
    for ref in bc.refs_of(channels):
        kw = bc.params_of(extra, ref)
        want = list(bounds.ref[ref])
        for n_groups in bc.PARITY_GROUPS:
            got, out_mag = mvdr(spec[:n_groups * channels].contiguous(), mag[:n_groups * channels].contiguous(), channels, _params(kw))
            assert got.shape == (n_groups, n_frames, f) and got.dtype == torch.complex64
            assert out_mag.shape == (n_groups, 1, f, n_frames) and out_mag.dtype == torch.float32
            got_h = got.cpu().numpy()
            for g in range(n_groups):
                err, scale = float(np.abs(got_h[g].astype(np.complex128) - want[g]).max()), float(np.abs(want[g]).max())
                print(f"n_fft {n_fft} T {n_frames} C {channels} ref {ref} {extra or ''} groups {n_groups} group {g}: max err {err:.3g} = "
                      f"{err / scale:.3g} of max |Y| ({err / scale / floor:.2f} floors of {floor:.2g}; bound 4)")
                assert err <= 4.0 * floor * scale, (n_groups, g, err / scale)
            assert np.array_equal(out_mag.cpu().numpy()[:, 0].view(np.int32), _mag_of(got_h).transpose(0, 2, 1).view(np.int32))
            sb.check(f"{sb.mvdr_label(n_fft, n_frames, channels, extra)} [ref {ref} groups {n_groups}]", got_h,
                     bounds.ref[ref][:n_groups], bounds)


@pytest.mark.parametrize("channels", bc.PARITY_CHANNELS, ids=lambda c: f"C{c}")
@pytest.mark.parametrize("n_frames", bc.PARITY_FRAMES)
def test_parity_with_the_float64_restatement(dev, n_frames, channels):
    _parity(dev, bc.PARITY_N_FFT, n_frames, channels, dict())


@pytest.mark.parametrize("case", (bc.WIDE_CASE, bc.LOADING_CASE, bc.PITCH_CASE, bc.UNIFORM_CASE),
                         ids=("n_fft512", "loading1e-6", "wide_mag", "uniform_mask"))
def test_parity_at_the_wide_transform_the_weakest_loading_a_wide_pitch_and_another_mask(dev, case):
    _parity(dev, *case)


@pytest.mark.parametrize("n_fft,n_frames,channels,refs", tuple(bc.variant_cases()),
                         ids=[f"T{t}-C{c}" + ("" if r == bc.refs_of(c) else f"-ref{r[0]}") for _, t, c, r in bc.variant_cases()])
def test_parity_at_the_instantiations_the_grid_does_not_reach(dev, n_fft, n_frames, channels, refs):
    """mvdr_kernel<4> (the edge of the 4-lane layout), <6> and <7> (21 and 28 triangle entries over 8 lanes, a partial last round)
    over the parity frames at both ends of the reference channel, and C = 6 once at an interior column of G
    (tests/variant_cover.py).  Per bin only: the FLOOR constants of beamform_ref are measured over the parity grid."""
    from audiodenoiser_amd.beamform import mvdr
    f = n_fft // 2 + 1
    spec, mag = _inputs(dev, n_fft, n_frames, channels)
    bounds = sb.mvdr_bounds(spec.cpu().numpy(), mag.cpu().numpy()[:, 0], channels, None, refs)
    assert bounds.floor <= sb.VARIANT_CAP, bounds.floor
    label = sb.mvdr_label(n_fft, n_frames, channels, sb.mvdr_variant_extra(channels, refs), "variant")
    for ref in refs:
        for n_groups in bc.PARITY_GROUPS:
            got, out_mag = mvdr(spec[:n_groups * channels].contiguous(), mag[:n_groups * channels].contiguous(), channels,
                                _params(dict(ref_channel=ref)))
            assert got.shape == (n_groups, n_frames, f) and got.dtype == torch.complex64
            got_h = got.cpu().numpy()
            assert np.array_equal(out_mag.cpu().numpy()[:, 0].view(np.int32), _mag_of(got_h).transpose(0, 2, 1).view(np.int32))
            sb.check(f"{label} [ref {ref} groups {n_groups}]", got_h, bounds.ref[ref][:n_groups], bounds)


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


@pytest.mark.parametrize("channels", sb.TILTED_MVDR, ids=lambda c: f"C{c}")
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, channels):
    """80 dB from the first bin to the last, the mask magnitudes scaled alike: the group-wide bound allows the quiet bins an error
    of their own size."""
    from audiodenoiser_amd.beamform import mvdr
    c = channels
    spec, mags = sb.mvdr_inputs(64, sb.TILTED_FRAMES, c)
    spec_h, mags_h = sb.scale_spec(spec, sb.tilt(33)), sb.scale_mags(mags, sb.tilt(33))
    bounds = sb.mvdr_bounds(spec_h, mags_h, c)
    for ref in bc.refs_of(c):
        for n_groups in bc.PARITY_GROUPS:
            got, out_mag = mvdr(_upload(dev, spec_h[:n_groups * c]), _upload(dev, mags_h[:n_groups * c, None]), c,
                                _params(dict(ref_channel=ref)))
            got_h = got.cpu().numpy()
            sb.check(f"{sb.mvdr_label(64, sb.TILTED_FRAMES, c, None, 'tilted')} [ref {ref} groups {n_groups}]", got_h,
                     bounds.ref[ref][:n_groups], bounds)
            assert np.array_equal(out_mag.cpu().numpy()[:, 0].view(np.int32), _mag_of(got_h).transpose(0, 2, 1).view(np.int32))


@pytest.mark.parametrize("channels", sb.TILTED_MVDR, ids=lambda c: f"C{c}")
def test_a_power_of_two_per_bin_comes_back_bit_for_bit(dev, channels):
    """The mask, both normalised covariances' solve and the filter are scale-free and the 1e-30 constants far below an ulp of what
    they are added to, so 2^-k times a bin's spectrogram and magnitudes is 2^-k times its output, exactly
    (tests/test_solver_bounds_host.py checks that the float32 restatement has the property, and here that no square leaves the
    normal range)."""
    from audiodenoiser_amd.beamform import mvdr
    c, f = channels, sb.pow2(33)
    spec, mags = sb.mvdr_inputs(64, sb.TILTED_FRAMES, c)
    s_spec, s_mags = sb.scale_spec(spec, f), sb.scale_mags(mags, f)
    sb.assert_squares_stay_normal(s_spec, s_mags)
    ft = _upload(dev, f.astype(np.float32))
    bounds = sb.mvdr_bounds(s_spec, s_mags, c)
    for ref in bc.refs_of(c):
        p = _params(dict(ref_channel=ref))
        plain, plain_mag = mvdr(_upload(dev, spec), _upload(dev, mags[:, None]), c, p)
        got, out_mag = mvdr(_upload(dev, s_spec), _upload(dev, s_mags[:, None]), c, p)
        sb.assert_squares_stay_normal(got.cpu().numpy())
        assert _same(got, torch.view_as_complex(torch.view_as_real(plain) * ft[None, None, :, None])), ref
        assert _same(out_mag, plain_mag * ft[None, None, :, None]), ref
        sb.check(f"{sb.mvdr_label(64, sb.TILTED_FRAMES, c, None, 'pow2')} [ref {ref}]", got.cpu().numpy(), bounds.ref[ref], bounds)


# ---- 3. exact pins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", PIN_CHANNELS, ids=lambda c: f"C{c}")
def test_repeat_batch_bin_subsets_and_pitch_are_exact(dev, channels):
    from audiodenoiser_amd.beamform import mvdr
    c, p = channels, _params(dict(ref_channel=channels - 1))
    spec, mag = _inputs(dev, 64, 97, c)
    full, full_mag = mvdr(spec, mag, c, p)
    again, again_mag = mvdr(spec, mag, c, p)
    assert _same(again, full) and _same(again_mag, full_mag)                       # two calls
    alone, alone_mag = mvdr(spec[c:2 * c].contiguous(), mag[c:2 * c].contiguous(), c, p)
    assert _same(alone, full[1:2]) and _same(alone_mag, full_mag[1:2])             # group 1 of 3 alone
    for lo, hi in ((5, 21), (0, 1), (32, 33)):                                      # bins repacked contiguous and run alone
        part, part_mag = mvdr(spec[:, :, lo:hi].contiguous(), mag[:, :, lo:hi].contiguous(), c, p)
        assert _same(part, full[:, :, lo:hi]) and _same(part_mag, full_mag[:, :, lo:hi]), (lo, hi)
    wide = torch.full((3 * c, 1, 33, 97 + 11), float("nan"), device=dev)            # mag_width wider than T against exactly T
    wide[..., :97] = mag
    out_wide = torch.full((3, 1, 33, 97 + 5), float("nan"), device=dev)
    got, got_mag = mvdr(spec, wide, c, p, out_wide)
    assert got_mag is out_wide and _same(got, full) and _same(out_wide[..., :97], full_mag) and bool(torch.isnan(out_wide[..., 97:]).all())
    assert not _same(full, spec[c - 1::c])


def test_one_channel_is_the_identity_and_zero_groups_give_zeros(dev):
    from audiodenoiser_amd.beamform import mvdr
    spec, mag = _inputs(dev, 64, 97, 1)
    got, got_mag = mvdr(spec, mag, 1)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(spec))          # as values: a signed zero may differ
    assert np.array_equal(got_mag.cpu().numpy()[:, 0], _mag_of(got.cpu().numpy()).transpose(0, 2, 1))
    spec, mag = _inputs(dev, 64, 23, 3)
    clean, clean_mag = mvdr(spec, mag, 3)
    zeroed, zmag = spec.clone(), mag.clone()
    zeroed[3:6] = 0                                                                 # group 1 of 3 is all zero
    zmag[3:6] = 0
    zeroed[6:9, :, 17] = 0                                                          # and one bin of group 2
    got, got_mag = mvdr(zeroed, zmag, 3)
    assert bool((torch.view_as_real(got[1]) == 0).all()) and bool((got_mag[1] == 0).all())
    assert bool((torch.view_as_real(got[2, :, 17]) == 0).all()) and bool((got_mag[2, 0, 17] == 0).all())
    assert _same(got[:1], clean[:1]) and _same(got_mag[:1], clean_mag[:1])
    keep = torch.ones(33, dtype=torch.bool, device=dev)
    keep[17] = False
    assert _same(got[2][:, keep], clean[2][:, keep])


@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
@pytest.mark.parametrize("channels", (2, 5), ids=lambda c: f"C{c}")
def test_a_non_finite_value_stays_in_its_own_group_and_bin(dev, channels, bad):
    from audiodenoiser_amd.beamform import mvdr
    c = channels
    spec, mag = _inputs(dev, 64, 65, c)
    clean, clean_mag = mvdr(spec, mag, c)
    group, channel, bin_, frame = 1, c - 1, 13, 37
    poisoned = spec.clone()
    poisoned[group * c + channel, frame, bin_] = complex(bad, 0.25)
    got, got_mag = mvdr(poisoned, mag, c)
    keep = torch.ones((3, 33), dtype=torch.bool, device=dev)
    keep[group, bin_] = False
    assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])
    assert _same(got_mag[:, 0][keep], clean_mag[:, 0][keep])
    poisoned_mag = mag.clone()                                                     # and a NaN in the magnitude estimate
    poisoned_mag[group * c, 0, bin_, frame] = float("nan")
    got, got_mag = mvdr(spec, poisoned_mag, c)
    assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep]) and _same(got_mag[:, 0][keep], clean_mag[:, 0][keep])


# ---- 4. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames,channels", ((64, 65, 2), (64, 5, 3), (64, 23, 8), (512, 23, 4), (64, 23, 7)),
                         ids=("C2", "C3short", "C8", "n_fft512", "C7"))
def test_footprint_only_what_the_call_owns(dev, n_fft, n_frames, channels):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.beamform import mvdr
    c, groups, f = channels, 2, n_fft // 2 + 1
    spec, mag = _inputs(dev, n_fft, n_frames, c, None, groups)
    p = _params(dict(ref_channel=c - 1))
    ps = ctypes.byref(p.to_struct())
    plain, plain_mag = mvdr(spec, mag, c, p)
    need = ctypes.c_size_t(0)
    assert _lib.load().adn_mvdr_workspace_bytes(groups, c, n_frames, f, ps, ctypes.byref(need)) == 0
    ws_bytes = max(int(need.value), 4096)                     # a workspace larger than asked for is the caller's right
    width = n_frames + 7
    out, h_out = fp.carve_tensor((groups, n_frames, f, 2), 0xFF, dev)
    out_mag, h_mag = fp.carve_tensor((groups, 1, f, width), 0xFF, dev)
    ws, h_ws = fp.carve(ws_bytes, 0xFF, dev)
    assert _raw(spec, mag, c, out, out_mag, ps, ws, ws_bytes) == 0
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_ws, "workspace")):
        fp.assert_guards_intact(h, what)
    if need.value == 0:
        assert fp.keeps_fill(h_ws, 0xFF)                      # nothing was asked for: nothing is touched
    assert _same(torch.view_as_complex(out), plain) and _same(out_mag[..., :n_frames], plain_mag)     # spec_out in full
    assert bool((out_mag.view(torch.int32)[..., n_frames:] == -1).all())            # columns >= T untouched
    # mag_out = NULL, workspace = NULL when none is needed: spec_out is written, the same bits
    out2, h_out2 = fp.carve_tensor((groups, n_frames, f, 2), 0xFF, dev)
    if need.value == 0:
        assert _raw(spec, mag, c, out2, None, ps) == 0
    else:
        assert _raw(spec, mag, c, out2, None, ps, ws, ws_bytes) == 0
    fp.assert_guards_intact(h_out2, "spec_out")
    fp.assert_guards_intact(h_mag, "mag_out")
    assert _same(out2, out)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def test_end_to_end_and_quality(dev):
    from audiodenoiser_amd.baseline import spectral_gain
    from audiodenoiser_amd.beamform import Beamformer, MvdrParams, mvdr
    from audiodenoiser_amd.dereverb import wpe_joint
    from audiodenoiser_amd.griffin_lim import stft_complex
    from audiodenoiser_amd.metrics import evaluate
    beam = Beamformer(dev)
    for c in (2, 4):
        noisy, dry = bc.recording(c)
        length = noisy.shape[1]
        xd, dd = torch.from_numpy(noisy.copy()).to(dev), torch.from_numpy(dry.copy()).to(dev)
        out = beam.denoise(xd)
        assert out.shape == (length,) and out.is_cuda and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        # bit-identical to the public pieces composed by hand
        n_frames = 1 + length // 128
        spec = stft_complex(xd, 512, 128)
        mag, _ = spectral_gain(spec)
        y = torch.zeros((1, 1, 257, max(n_frames, 16)), device=dev)
        d, _ = mvdr(spec, mag, c, None, y)
        assert torch.equal(out, beam._resynth(y, d, length, int(y.shape[3]), 0)[0])
        # SI-SDR against the restatement's, the quality cap of the single-channel test: at least half of its gain over the input
        r_in, r_out = bc.restatement_si_sdr("microphone 0 as recorded", c), bc.restatement_si_sdr("MVDR, mask from the spectral gain", c)
        before, after = (float(evaluate(a[None], dd[None], sr=8000)["si_sdr"][0]) for a in (xd[0], out))
        print(f"C = {c}: SI-SDR on the device {before:.2f} -> {after:.2f} dB (the restatement's: {r_in:.2f} -> {r_out:.2f})")
        assert r_out - r_in >= 2.0 and after - before >= 0.5 * (r_out - r_in)
    # shapes: (N, C, L) -> (N, L), every recording as alone; (L,) -> (L,); numpy in -> numpy out
    short = xd[:, 4000:10000].contiguous()
    batch = torch.stack([short, short.flip(0), 0.5 * short])
    got = beam.denoise(batch)
    assert got.shape == (3, 6000)
    for i in range(3):
        assert torch.equal(got[i], beam.denoise(batch[i]))
    assert beam.denoise(short[0]).shape == (6000,)
    as_np = beam.denoise(short.cpu().numpy())
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float32 and np.array_equal(as_np, got[0].cpu().numpy())
    # wpe=True and gain=True compose: joint WPE at taps = 32 // C, the gain's mask, MVDR at the last microphone, the gain on Y
    s4 = stft_complex(short, 512, 128)
    dw, _ = wpe_joint(s4, 4)
    y2 = torch.zeros((1, 1, 257, 1 + 6000 // 128), device=dev)
    yw, _ = mvdr(dw, spectral_gain(dw)[0], 4, MvdrParams(ref_channel=3), y2)
    spectral_gain(yw, out=y2)
    cascade = Beamformer(dev, params=MvdrParams(ref_channel=3), wpe=True, gain=True).denoise(short)
    assert torch.equal(cascade, beam._resynth(y2, yw, 6000, int(y2.shape[3]), 0)[0]) and not torch.equal(cascade, got[0])
    # another rate comes back at its length
    assert beam.denoise(xd[:, :16501].contiguous(), sr=44100).shape == (16501,)
    assert beam.denoise(batch[:, :2, :5000].contiguous(), sr=16000).shape == (3, 5000)
    # a reference channel the input does not have is the call's ValueError
    with pytest.raises(ValueError, match="ref_channel"):
        Beamformer(dev, params=MvdrParams(ref_channel=4)).denoise(short)
    with pytest.raises(ValueError, match="channels"):
        beam.denoise(torch.zeros((9, 600), device=dev))


def test_file_and_command_line(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.beamform import Beamformer
    from audiodenoiser_amd.wav import read_wav, write_wav
    noisy, dry = bc.recording(4)
    src, ref, dst, dst_cli = (str(tmp_path / n) for n in ("room4ch.wav", "dry.wav", "out.wav", "out_cli.wav"))
    write_wav(src, np.ascontiguousarray(noisy[:, :16000].T), 8000, "PCM_16")
    write_wav(ref, dry[:16000], 8000, "PCM_16")
    assert Beamformer(dev).denoise_file(src, dst) == (16000, 8000)
    audio, rate = read_wav(dst, mono=False)
    assert audio.shape == (16000, 1) and rate == 8000
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.beamform", src, dst_cli, "--reference", ref], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert np.array_equal(read_wav(dst_cli, mono=False)[0], audio)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    row = json.loads(lines[0])
    # "noisy" is the MONO MIX of the file, itself a delay-free sum of the four microphones: the line is checked for its form only
    assert row["file"] == src and all(np.isfinite(row[k]["si_sdr"]) for k in ("noisy", "denoised"))


# ---- 6. refusals on the device ---------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.beamform import MvdrParams
    c, groups, n_frames, f = 2, 2, 23, 33
    spec, mag = _inputs(dev, 64, n_frames, c, None, groups)
    out, h_out = fp.carve_tensor((groups, n_frames, f, 2), 0xFF, dev)
    out_mag, h_mag = fp.carve_tensor((groups, 1, f, n_frames + 7), 0xFF, dev)
    L = _lib.load()
    s = torch.view_as_real(spec)

    def refused(word, code=1, **kw):
        assert _raw(spec, mag, c, kw.get("out", out), kw.get("out_mag", out_mag), kw.get("params"), spec_ptr=kw.get("spec_ptr")) == code, word
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_mvdr:") and word in msg, msg
        assert fp.keeps_fill(h_out, 0xFF) and fp.keeps_fill(h_mag, 0xFF), word
        fp.assert_guards_intact(h_out, "spec_out")
        fp.assert_guards_intact(h_mag, "mag_out")

    refused(b"overlap", out=s.data_ptr())                                         # spec_out on spec
    refused(b"overlap", out=s.data_ptr() + 8 * (2 * c * n_frames * f - 1))        # spec_out on spec's last cell
    refused(b"overlap", out=mag.data_ptr())                                       # spec_out on mag
    refused(b"overlap", out_mag=mag.data_ptr())                                   # mag_out on mag
    refused(b"overlap", out_mag=out.data_ptr())                                   # mag_out on spec_out
    refused(b"aligned", out=out.data_ptr() + 4)
    refused(b"aligned", out_mag=out_mag.data_ptr() + 2)
    refused(b"aligned", spec_ptr=s.data_ptr() + 4)
    bad = MvdrParams().to_struct()
    bad.ref_channel = c
    refused(b"ref_channel", params=ctypes.byref(bad))
    need = ctypes.c_size_t(0)
    assert L.adn_mvdr_workspace_bytes(groups, c, n_frames, f, None, ctypes.byref(need)) == 0
    if need.value > 0:                                                            # a workspace below the reported need: code 3
        rc = L.adn_mvdr(s.data_ptr(), mag.data_ptr(), n_frames, groups, c, n_frames, f, None, None, need.value - 1, out.data_ptr(),
                        out_mag.data_ptr(), n_frames + 7, None)
        assert rc == 3 and L.adn_last_error().startswith(b"adn_mvdr:") and fp.keeps_fill(h_out, 0xFF)
    assert _raw(spec, mag, c, out, out_mag) == 0                                  # and the same buffers are then written
    assert not fp.keeps_fill(h_out, 0xFF)
