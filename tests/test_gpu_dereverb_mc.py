"""Multichannel dereverberation on the device (csrc/dereverb_mc_kernels.hip, audiodenoiser_amd/dereverb.py) against the float64
restatement in tests/dereverb_mc_ref.py.

Bounds (derived, not tuned):
* adn_wpe_mc, per group: max |d_dev - d_64| <= 4 floor max |d_64|.  The floors are the error of the same statements run in float32
  on the host over these very cases (python tests/dereverb_mc_cases.py), never a device figure; the factor 4 is the project's
  convention.  The one case at loading 1e-6 is held to dereverb_mc_ref.FLOOR, which it sets; every case at the default loading to
  the 140 times smaller FLOOR_DEFAULT_LOADING.  The restatement is applied to the DOWNLOADED device spectrogram, so the STFT's
  own error does not enter.
* adn_wpe_mc, per (row, bin): E = max_t |d_dev - d_64| / max_t |d_64| <= 4 floor for every bin of every channel of every group,
  beside the bound above (tests/solver_bounds.py).  The floor is the case's own: the largest E of the float32 restatement on the
  same input over every bin, the three groups and both orders of the sums over t (pairwise and sequential), measured when the
  test runs, never below 2^-23 and never from the device.  The same bound holds the tilted cases (an 80 dB slope over the bins,
  built on the host and uploaded), and a power of two per bin, 2^-((5 b) mod 13), has to come back bit for bit as the equally
  scaled unscaled result.
* mag_out against sqrtf(fmaf(re, re, im * im)) of the device's own spec_out, evaluated in float32 on the host: equal bit for bit.
* Repeat, batch, bin-subset, one-channel, pass-through, zero-group and isolation tests: exact equality, as include/adn.h pins them.
* End to end: bit-identical to the public pieces composed by hand; SI-SDR within the quality cap of tests/test_gpu_dereverb.py
  (at least half of the restatement's gain), per channel.
Measured on the MI355X: parity uses at most 3.94 of a floor at the default loading (bound 4): n_fft 64, T = 97, (8, 4), group 1,
2.7e-4 of max |d|; next 3.61 at (2, 10), T = 97; 3.24 of its own floor at loading 1e-6; the median over all 176 comparisons 0.04.
SI-SDR of the joint class 3.33 -> 9.95 and 3.36 -> 10.52 dB: the restatement's, to the printed digits.
Per bin (profiles/solver_bins.md): at most 3.62 of the case's floor (bound 4): the power-of-two case at (2, 10), T = 97, group 0,
channel 0, bin 1, E 3.2e-4 -- the bin of the group-wide figure above; 3.18 there unscaled, 2.59 tilted; both power-of-two cases bit
for bit; the median over the 94 runs 0.85.
The 17 layouts PARITY_CK does not reach (tests/variant_cover.py: 19 pairs at T = 23 and 97, per bin only): at most 1.96 floors
((5, 2), T = 23, group 1, channel 4, bin 10, E 1.1e-4), next 1.94 at (6, 5); the median over the 76 runs 1.19.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_ref as dr  # noqa: E402
import footprint as fp  # noqa: E402
import solver_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu

# 16, 32, 32 and 64 lanes per bin; K % 4 != 0 twice, == 0 twice; (5, 6): two P block columns, the second with a repeated last channel;
# (3, 2): lanes doubled beyond what the blocks need
PIN_CK = ((2, 5), (3, 7), (3, 8), (2, 16), (5, 6), (3, 2))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _spec(dev, n_fft, n_frames, channels, n_groups=3):
    """The device's own STFT of the parity recordings: device complex64 (n_groups * channels, T, F)."""
    from audiodenoiser_amd.griffin_lim import stft_complex
    x = torch.from_numpy(mc.parity_audio(n_fft, n_frames, channels)[:n_groups * channels].copy()).to(dev)
    spec = stft_complex(x, n_fft, n_fft // 4)
    assert spec.shape == (n_groups * channels, n_frames, n_fft // 2 + 1)
    return spec


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _params(kw):
    from audiodenoiser_amd.dereverb import WpeParams
    return None if kw is None else WpeParams(**kw)


def _raw(spec, channels, spec_out, mag_out, params=None, ws=None, ws_bytes=0):
    """adn_wpe_mc itself; returns the status."""
    from audiodenoiser_amd import _lib
    n, t, f = spec.shape
    s = torch.view_as_real(spec.contiguous())
    rc = _lib.load().adn_wpe_mc(s.data_ptr(), n // channels, channels, t, f, params, ws.data_ptr() if ws is not None else None, ws_bytes,
                                spec_out.data_ptr(), mag_out.data_ptr() if mag_out is not None else None,
                                int(mag_out.shape[-1]) if mag_out is not None else 0, torch.cuda.current_stream(spec.device).cuda_stream)
    torch.cuda.synchronize(spec.device)
    return rc


def _mag_of(d):
    """sqrtf(fmaf(re, re, im * im)) of a complex64 array, in float32."""
    return np.sqrt(dr._power(d, np.float32))


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
def _parity(dev, n_fft, n_frames, ck, extra):
    from audiodenoiser_amd.dereverb import wpe_joint
    channels, kw, floor = ck[0], mc.params_of(ck, extra), mc.floor_for(extra)
    spec = _spec(dev, n_fft, n_frames, channels)
    bounds = sb.wpe_mc_bounds(spec.cpu().numpy(), channels, kw)     # the float64 restatement and the case's own float32 floor
    want = list(bounds.ref.reshape(3, channels, n_frames, -1))
    for n_groups in mc.PARITY_GROUPS:
        got, mag = wpe_joint(spec[:n_groups * channels].contiguous(), channels, _params(kw))
        assert got.shape == (n_groups * channels, n_frames, n_fft // 2 + 1) and got.dtype == torch.complex64
        assert mag.shape == (n_groups * channels, 1, n_fft // 2 + 1, n_frames) and mag.dtype == torch.float32
        got_h, mag_h = got.cpu().numpy().reshape(n_groups, channels, n_frames, -1), mag.cpu().numpy()[:, 0]
        for g in range(n_groups):
            err, scale = float(np.abs(got_h[g].astype(np.complex128) - want[g]).max()), float(np.abs(want[g]).max())
            print(f"n_fft {n_fft} T {n_frames} (C, K) {ck} {extra or ''} groups {n_groups} group {g}: max err {err:.3g} = "
                  f"{err / scale:.3g} of max |d| ({err / scale / floor:.2f} floors of {floor:.2g}; bound 4)")
            assert err <= 4.0 * floor * scale, (n_groups, g, err / scale)
        assert np.array_equal(mag_h.view(np.int32), _mag_of(got.cpu().numpy()).transpose(0, 2, 1).view(np.int32))
        sb.check(f"{sb.mc_label(n_fft, n_frames, ck, extra)} [groups {n_groups}]", got.cpu().numpy(),
                 bounds.ref[:n_groups * channels], bounds)


@pytest.mark.parametrize("ck", mc.PARITY_CK, ids=lambda ck: f"C{ck[0]}K{ck[1]}")
@pytest.mark.parametrize("n_frames", mc.PARITY_FRAMES)
def test_parity_with_the_float64_restatement(dev, n_frames, ck):
    _parity(dev, mc.PARITY_N_FFT, n_frames, ck, None)


@pytest.mark.parametrize("case", (mc.WIDE_CASE, mc.LOADING_CASE), ids=("n_fft512", "loading1e-6"))
def test_parity_at_the_wide_transform_and_the_weakest_loading(dev, case):
    _parity(dev, *case)


@pytest.mark.parametrize("n_frames", mc.VARIANT_FRAMES)
@pytest.mark.parametrize("ck", mc.VARIANT_CK, ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_parity_at_the_lane_layouts_the_grid_does_not_reach(dev, ck, n_frames):
    """One (C, K) per key of tests/variant_cover.py that PARITY_CK leaves out: the doubled lane groups, two P block columns with a
    repeated last channel (C = 5, 6, 7), the defaults taps = 32 // C of 3, 5, 6 and 7 microphones.  Per bin only: the FLOOR constants
    of dereverb_mc_ref are measured over the parity grid and do not speak for these."""
    from audiodenoiser_amd.dereverb import wpe_joint
    n_fft, channels, kw = mc.PARITY_N_FFT, ck[0], mc.params_of(ck)
    spec = _spec(dev, n_fft, n_frames, channels)
    bounds = sb.wpe_mc_bounds(spec.cpu().numpy(), channels, kw)     # the float64 restatement and the case's own float32 floor
    assert bounds.floor <= sb.VARIANT_CAP, bounds.floor
    for n_groups in mc.PARITY_GROUPS:
        got, mag = wpe_joint(spec[:n_groups * channels].contiguous(), channels, _params(kw))
        assert got.shape == (n_groups * channels, n_frames, n_fft // 2 + 1) and got.dtype == torch.complex64
        got_h = got.cpu().numpy()
        assert np.array_equal(mag.cpu().numpy()[:, 0].view(np.int32), _mag_of(got_h).transpose(0, 2, 1).view(np.int32))
        sb.check(f"{sb.mc_label(n_fft, n_frames, ck, None, 'variant')} [groups {n_groups}]", got_h,
                 bounds.ref[:n_groups * channels], bounds)


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


@pytest.mark.parametrize("ck", sb.TILTED_MC, ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, ck):
    """80 dB from the first bin to the last: the group-wide bound allows the quiet bins an error of their own size."""
    from audiodenoiser_amd.dereverb import wpe_joint
    c, kw = ck[0], mc.params_of(ck)
    spec_h = sb.scale_spec(sb.mc_spec(64, sb.TILTED_FRAMES, c), sb.tilt(33))
    bounds = sb.wpe_mc_bounds(spec_h, c, kw)
    for n_groups in mc.PARITY_GROUPS:
        got, mag = wpe_joint(_upload(dev, spec_h[:n_groups * c]), c, _params(kw))
        got_h = got.cpu().numpy()
        sb.check(f"{sb.mc_label(64, sb.TILTED_FRAMES, ck, None, 'tilted')} [groups {n_groups}]", got_h, bounds.ref[:n_groups * c], bounds)
        assert np.array_equal(mag.cpu().numpy()[:, 0].view(np.int32), _mag_of(got_h).transpose(0, 2, 1).view(np.int32))


@pytest.mark.parametrize("ck", sb.TILTED_MC, ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_a_power_of_two_per_bin_comes_back_bit_for_bit(dev, ck):
    """R, the taps and the weights' product with the signal are scale-free and the 1e-30 constants far below an ulp of what they
    are added to, so 2^-k times a bin's input is 2^-k times its output, exactly (tests/test_solver_bounds_host.py checks that the
    float32 restatement has the property, and here that no square leaves the normal range)."""
    from audiodenoiser_amd.dereverb import wpe_joint
    c, kw = ck[0], mc.params_of(ck)
    base, f = sb.mc_spec(64, sb.TILTED_FRAMES, c), sb.pow2(33)
    scaled = sb.scale_spec(base, f)
    sb.assert_squares_stay_normal(scaled)
    ft = _upload(dev, f.astype(np.float32))
    plain, plain_mag = wpe_joint(_upload(dev, base), c, _params(kw))
    got, mag = wpe_joint(_upload(dev, scaled), c, _params(kw))
    sb.assert_squares_stay_normal(got.cpu().numpy())
    assert _same(got, torch.view_as_complex(torch.view_as_real(plain) * ft[None, None, :, None]))
    assert _same(mag, plain_mag * ft[None, None, :, None])
    bounds = sb.wpe_mc_bounds(scaled, c, kw)
    sb.check(sb.mc_label(64, sb.TILTED_FRAMES, ck, None, "pow2"), got.cpu().numpy(), bounds.ref, bounds)


# ---- 2. exact pins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", PIN_CK, ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_repeat_batch_and_bin_subsets_are_exact(dev, ck):
    from audiodenoiser_amd.dereverb import wpe_joint
    c, p = ck[0], _params(dict(taps=ck[1]))
    spec = _spec(dev, 64, 97, c)
    full, full_mag = wpe_joint(spec, c, p)
    again, again_mag = wpe_joint(spec, c, p)
    assert _same(again, full) and _same(again_mag, full_mag)                       # two calls
    alone, alone_mag = wpe_joint(spec[c:2 * c].contiguous(), c, p)
    assert _same(alone, full[c:2 * c]) and _same(alone_mag, full_mag[c:2 * c])     # group 1 of 3 alone
    for lo, hi in ((5, 21), (0, 1), (32, 33), (7, 24)):                             # bins repacked contiguous and run alone
        part, part_mag = wpe_joint(spec[:, :, lo:hi].contiguous(), c, p)
        assert _same(part, full[:, :, lo:hi]) and _same(part_mag, full_mag[:, :, lo:hi]), (lo, hi)
    assert not _same(full, spec)


@pytest.mark.parametrize("kw", (None, dict(taps=20), dict(taps=32, delay=8, iterations=2), dict(taps=5, loading=1e-6)),
                         ids=("null", "k20", "largest", "k5"))
def test_one_channel_returns_adn_wpe_s_bits(dev, kw):
    from audiodenoiser_amd.dereverb import WpeParams, wpe, wpe_joint
    spec = _spec(dev, 64, 97, 1)
    got, got_mag = wpe_joint(spec, 1, _params(kw))
    want, want_mag = wpe(spec, WpeParams(taps=32) if kw is None else _params(kw))  # NULL at one channel: taps = 32 / 1
    assert _same(got, want) and _same(got_mag, want_mag) and not _same(got, spec)


def test_short_groups_first_frames_and_zero_groups(dev):
    from audiodenoiser_amd.dereverb import WpeParams, wpe_joint
    for n_frames in (1, 2, 3):                                                      # T <= D: bit for bit
        spec = _spec(dev, 64, 3, 3)[:, :n_frames].contiguous()
        got, mag = wpe_joint(spec, 3)
        assert _same(got, spec)
        assert np.array_equal(mag.cpu().numpy()[:, 0], _mag_of(spec.cpu().numpy()).transpose(0, 2, 1))
    spec = _spec(dev, 64, 23, 2)
    assert _same(wpe_joint(spec[:, :8].contiguous(), 2, WpeParams(taps=16, delay=8))[0], spec[:, :8])
    for delay in (1, 3, 8):                                                         # the first D frames of every channel
        got, _ = wpe_joint(spec, 2, WpeParams(taps=10, delay=delay))
        assert _same(got[:, :delay], spec[:, :delay]) and not _same(got[:, delay:], spec[:, delay:])
    clean, clean_mag = wpe_joint(spec, 2)
    zeroed = spec.clone()
    zeroed[2:4] = 0                                                                 # group 1 of 3 is all zero
    zeroed[4:6, :, 17] = 0                                                          # and one bin of group 2
    got, mag = wpe_joint(zeroed, 2)
    assert bool((_bits(got[2:4]) == 0).all()) and bool((mag[2:4] == 0).all())
    assert bool((_bits(got[4:6, :, 17]) == 0).all()) and bool((mag[4:6, 0, 17] == 0).all())
    assert _same(got[:2], clean[:2]) and _same(mag[:2], clean_mag[:2])
    keep = torch.ones(33, dtype=torch.bool, device=dev)
    keep[17] = False
    assert _same(got[4:6][:, :, keep], clean[4:6][:, :, keep])


# ---- 3. isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
@pytest.mark.parametrize("ck", ((2, 10), (4, 8)), ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_a_non_finite_value_stays_in_its_own_group_and_bin(dev, ck, bad):
    from audiodenoiser_amd.dereverb import wpe_joint
    c, p = ck[0], _params(dict(taps=ck[1]))
    spec = _spec(dev, 64, 70, c)
    clean, clean_mag = wpe_joint(spec, c, p)
    group, channel, bin_, frame = 1, c - 1, 13, 37
    poisoned = spec.clone()
    poisoned[group * c + channel, frame, bin_] = complex(bad, 0.25)
    got, mag = wpe_joint(poisoned, c, p)
    keep = torch.ones((3 * c, 33), dtype=torch.bool, device=dev)
    keep[group * c:(group + 1) * c, bin_] = False
    assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])
    assert _same(mag[:, 0][keep], clean_mag[:, 0][keep])


# ---- 4. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames,ck", ((64, 65, (2, 10)), (64, 5, (3, 7)), (64, 70, (8, 4)), (512, 23, (2, 16)), (64, 23, (7, 4))),
                         ids=("C2K10", "C3K7short", "C8K4", "n_fft512", "C7K4"))
def test_footprint_only_what_the_call_owns(dev, n_fft, n_frames, ck):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import wpe_joint
    c, groups, f = ck[0], 2, n_fft // 2 + 1
    n = groups * c
    spec = _spec(dev, n_fft, n_frames, c, groups)
    p = _params(dict(taps=ck[1]))
    ps = ctypes.byref(p.to_struct())
    plain, plain_mag = wpe_joint(spec, c, p)
    need = ctypes.c_size_t(0)
    assert _lib.load().adn_wpe_mc_workspace_bytes(groups, c, n_frames, f, ps, ctypes.byref(need)) == 0
    ws_bytes = max(int(need.value), 4096)                     # a workspace larger than asked for is the caller's right
    width = n_frames + 7
    out, h_out = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    mag, h_mag = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    ws, h_ws = fp.carve(ws_bytes, 0xFF, dev)
    assert _raw(spec, c, out, mag, ps, ws, ws_bytes) == 0
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_ws, "workspace")):
        fp.assert_guards_intact(h, what)
    if need.value == 0:
        assert fp.keeps_fill(h_ws, 0xFF)                      # nothing was asked for: nothing is touched
    assert _same(torch.view_as_complex(out), plain) and _same(mag[..., :n_frames], plain_mag)     # spec_out in full: no 0xFF word left
    assert bool((mag.view(torch.int32)[..., n_frames:] == -1).all())
    # mag_out = NULL, workspace = NULL when none is needed: spec_out is written, the same bits
    out2, h_out2 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    if need.value == 0:
        assert _raw(spec, c, out2, None, ps) == 0
    else:
        assert _raw(spec, c, out2, None, ps, ws, ws_bytes) == 0
    fp.assert_guards_intact(h_out2, "spec_out")
    fp.assert_guards_intact(h_mag, "mag_out")
    assert _same(out2, out)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def _resynth_by_hand(dev, y, d, length):
    from audiodenoiser_amd import _lib
    out = torch.empty((d.shape[0], length), device=dev)
    _lib.check(_lib.load().adn_denoise_resynth(y.data_ptr(), torch.view_as_real(d).data_ptr(), d.shape[0], length, 512, 128,
                                               int(y.shape[3]), 0, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "adn_denoise_resynth")
    return out


def test_joint_end_to_end_and_quality(dev):
    from audiodenoiser_amd.baseline import spectral_gain
    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams, wpe_joint
    from audiodenoiser_amd.griffin_lim import stft_complex
    from audiodenoiser_amd.metrics import evaluate
    wet, dry = mc.recording(2)
    length = wet.shape[1]
    xd, dd = torch.from_numpy(wet.copy()).to(dev), torch.from_numpy(np.stack([dry, dry])).to(dev)
    dn = Dereverberator(dev, channels="joint")
    out = dn.denoise(xd)
    assert out.shape == xd.shape and out.is_cuda and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    # bit-identical to the public pieces composed by hand, at taps = 32 // 2
    n_frames = 1 + length // 128
    spec = stft_complex(xd, 512, 128)
    y = torch.zeros((2, 1, 257, max(n_frames, 16)), device=dev)
    d, _ = wpe_joint(spec, 2, WpeParams(taps=16), y)
    assert torch.equal(out, _resynth_by_hand(dev, y, d, length))
    assert _same(d, wpe_joint(spec, 2)[0])
    # SI-SDR per channel against the restatement's, the quality cap of the single-channel test: at least half of its gain
    r_in, r_out = mc.restatement_si_sdr("input"), mc.restatement_si_sdr("joint, C = 2, K = 16")
    before, after = (evaluate(a, dd, sr=8000)["si_sdr"] for a in (xd, out))
    for c in range(2):
        print(f"channel {c}: SI-SDR on the device {float(before[c]):.2f} -> {float(after[c]):.2f} dB "
              f"(the restatement's: {r_in[c]:.2f} -> {r_out[c]:.2f})")
        assert r_out[c] - r_in[c] >= 2.0 and float(after[c]) - float(before[c]) >= 0.5 * (r_out[c] - r_in[c])
    # a batch of recordings (N, C, L): every recording as alone; numpy in -> numpy out
    short = xd[:, 4000:10000].contiguous()
    batch = torch.stack([short, short.flip(0), 0.5 * short])
    got = dn.denoise(batch)
    assert got.shape == batch.shape
    for i in range(3):
        assert torch.equal(got[i], dn.denoise(batch[i]))
    as_np = dn.denoise(short.cpu().numpy())
    assert isinstance(as_np, np.ndarray) and as_np.dtype == np.float32 and np.array_equal(as_np, got[0].cpu().numpy())
    # the cascade: the gain of the spectral baseline per channel on the joint result
    ds, _ = wpe_joint(stft_complex(short, 512, 128), 2)
    y2 = torch.zeros((2, 1, 257, 1 + 6000 // 128), device=dev)
    spectral_gain(ds, out=y2)
    cascade = Dereverberator(dev, channels="joint", gain=True).denoise(short)
    assert torch.equal(cascade, _resynth_by_hand(dev, y2, ds, 6000)) and not torch.equal(cascade, got[0])
    # another rate comes back at its length
    assert dn.denoise(xd[:, :16501].contiguous(), sr=16000).shape == (2, 16501)
    # parameters that do not fit the channel count are the call's ValueError; they fit one channel
    tight = Dereverberator(dev, channels="joint", params=WpeParams())
    with pytest.raises(ValueError, match=r"channels \* taps"):
        tight.denoise(short)
    with pytest.raises(ValueError, match="channels"):
        dn.denoise(torch.zeros((9, 600), device=dev))
    assert tight.denoise(short[0]).shape == (6000,)


@pytest.mark.parametrize("channels", (5, 6, 7), ids=lambda c: f"C{c}")
def test_no_parameters_is_the_library_s_null_at_five_six_and_seven_channels(dev, channels):
    """taps = 32 // C is stated twice, by joint_default_taps of the library and by the Python classes: a 5-, 6- or 7-channel
    recording through the class with no parameters is, bit for bit, adn_wpe_mc with params = NULL."""
    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams, wpe_joint
    from audiodenoiser_amd.griffin_lim import stft_complex
    c = channels
    xd = torch.from_numpy(mc.parity_audio(64, 97, c)[:c].copy()).to(dev)
    length = xd.shape[1]
    spec = stft_complex(xd, 512, 128)
    t = spec.shape[1]
    out = torch.empty((c, t, 257, 2), device=dev)
    y = torch.zeros((c, 1, 257, max(t, 16)), device=dev)
    assert _raw(spec, c, out, y, None) == 0                                         # params = NULL
    d = torch.view_as_complex(out)
    got, got_mag = wpe_joint(spec, c)                                               # Python's default
    assert _same(got, d) and _same(got_mag, y[..., :t]) and not _same(d, spec)
    assert _same(wpe_joint(spec, c, WpeParams(taps=32 // c))[0], d)
    assert not _same(wpe_joint(spec, c, WpeParams(taps=32 // c - 1))[0], d)
    assert torch.equal(Dereverberator(dev, channels="joint").denoise(xd), _resynth_by_hand(dev, y, d, length))


def test_separate_and_mono_are_today_s_bits(dev):
    from audiodenoiser_amd.dereverb import Dereverberator, wpe
    from audiodenoiser_amd.griffin_lim import stft_complex
    wet, _ = mc.recording(2)
    xd = torch.from_numpy(wet[:, 8000:14000].copy()).to(dev)
    spec = stft_complex(xd, 512, 128)
    y = torch.zeros((2, 1, 257, 1 + 6000 // 128), device=dev)
    d, _ = wpe(spec, mag_out=y)                                                     # adn_wpe, every channel a clip
    today = _resynth_by_hand(dev, y, d, 6000)
    assert torch.equal(Dereverberator(dev).denoise(xd), today)
    assert torch.equal(Dereverberator(dev, channels="separate").denoise(xd), today)
    joint = Dereverberator(dev, channels="joint")
    assert torch.equal(joint.denoise(xd[0]), today[0]) and torch.equal(joint.denoise(xd[1:2]), today[1:2])      # mono
    assert not torch.equal(joint.denoise(xd), today)
    with pytest.raises(ValueError):
        Dereverberator(dev).denoise(torch.zeros((2, 2, 600), device=dev))           # (N, C, L) is the joint form's


def test_file_and_command_line(dev, tmp_path):
    import subprocess
    from audiodenoiser_amd.dereverb import Dereverberator
    from audiodenoiser_amd.wav import read_wav, write_wav
    wet, _ = mc.recording(2)
    src, dst, dst_sep, dst_cli = (str(tmp_path / n) for n in ("room.wav", "joint.wav", "separate.wav", "joint_cli.wav"))
    write_wav(src, np.ascontiguousarray(wet[:, :16000].T), 8000, "PCM_16")
    assert Dereverberator(dev, channels="joint").denoise_file(src, dst) == (16000, 8000)
    assert Dereverberator(dev).denoise_file(src, dst_sep) == (16000, 8000)
    audio, rate = read_wav(dst, mono=False)
    assert audio.shape == (16000, 2) and rate == 8000
    assert not np.array_equal(audio, read_wav(dst_sep, mono=False)[0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.dereverb", src, dst_cli, "--joint"], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert np.array_equal(read_wav(dst_cli, mono=False)[0], audio)
