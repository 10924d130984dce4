"""Streaming multichannel dereverberation on the device (csrc/dereverb_mc_stream_kernels.hip, audiodenoiser_amd/dereverb.py) against
the float64 restatement in tests/dereverb_mc_stream_ref.py.

Bounds (derived, not tuned):
* adn_wpe_mc_online, per group: max |d_dev - d_64| <= 4 FLOOR max |d_64|.  FLOOR (dereverb_mc_stream_ref.FLOOR) is the error of the
  same statements run in float32 on the host over these very cases (python tests/dereverb_mc_stream_cases.py), never a device
  figure; the factor 4 is the project's standing margin.  The restatement is applied to the DOWNLOADED device spectrogram, so the
  STFT's own error does not enter.  mag_out likewise against |d_64|, on the same scale.
* adn_wpe_mc_online, per (channel row, bin): E = max_t |d_dev - d_64| / max_t |d_64| <= 4 floor for every bin of every row, beside
  the bound above (tests/recursive_bounds.py).  The floor is the case's own: the largest E of the float32 restatement on the same
  downloaded spectrogram over every bin of the case's three groups and over two float32 arithmetics -- "plain" (every product
  rounded, what FLOOR was measured with; the "pairwise" column of the printed line) and "fma" (the header's pairing and order of
  every multiply-add; the "sequential" column) -- measured when the test runs, never below 2^-23 (the cases with T <= D, whose
  reference is the input bit for bit), never from the device, and asserted under the cap of 1e-4.  The same bound holds the tilted
  cases (an 80 dB slope over the bins, built on the host and uploaded) at (C, K) = (2, 16) and (8, 4).  There is no power-of-two
  case: P_0 = 1 / delta and the 1e-30 in phi_t are absolute, the operator is not scale invariant.
* mag_out, bit for bit: sqrtf(fmaf(re, re, im * im)) of the device's own spec_out, evaluated in float32 on the host.
* StreamDereverberator(channels=C), per channel: max |audio_dev - audio_64| <= 4 FLOOR_AUDIO max |audio_64|, FLOOR_AUDIO the error
  of the end-to-end form with every statement in float32 on the host, the two transforms included.
* Quality: the device's SI-SDR gain per channel is at least half the float64 restatement's (the cap of test_gpu_dereverb_mc.py).
* Repeat, cut, batch, bin-subset, poisoned-state, one-channel, pass-through, isolation, push-size, block, reset and footprint tests:
  exact equality, as include/adn.h pins them.
Measured on the MI355X: parity uses at most 0.32 of a floor (bound 4): n_fft 64, T = 97, (2, 16) at forget 0.984375, group 2; at
the default forget at most 0.18, the median over all 112 comparisons under 0.01; mag_out at most 0.31 floors.  The streams against
the float64 end-to-end form: 1.6e-7 - 4.8e-7 of the maximum, 0.08 - 0.24 of the audio floor (bound 4).  Quality: 3.33 -> 6.17 and
3.36 -> 6.12 dB, the restatement's to the printed digits.  The whole file: 52 cases in 10.8 s, the command-line case 4.2 s, every
other one under 0.7 s.  The rest: profiles/bench_dereverb_mc_stream.md.
Per bin (profiles/recursive_bins.md): at most 0.74 of the case's floor (bound 4): n_fft 64, T = 23, (8, 4), group 1, channel 0, bin 24,
E 1.9e-7; at T = 97 0.06 - 0.44, where the plain arithmetic sets the floor and the device follows the fma one; the tilted cases
0.21 and 0.32, the device's worst E there the fma restatement's own to the printed digits.  With the floors the file is 54 cases
in 14 s, the n_fft 512 parity case 1.1 s, every other parity case under 0.5 s.
The channel counts that grid does not reach (tests/variant_cover.py: C = 5, 6, 7 at T = 4, 23, 97, per bin only): at most 0.94
floors ((6, 5), T = 23, group 2, channel 2, bin 6, E 1.7e-7), the median over the 30 runs 0.24.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_stream_cases as msc  # noqa: E402
import dereverb_mc_stream_ref as ms  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402
import footprint as fp  # noqa: E402
import recursive_bounds as rb  # noqa: E402
import solver_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


_SPECS = {}


def _spec(dev, n_fft, n_frames, channels):
    """The device's own STFT of the three parity recordings of `channels` microphones: device complex64 (3 C, T, F), computed once."""
    key = (n_fft, n_frames, channels)
    if key not in _SPECS:
        from audiodenoiser_amd.griffin_lim import stft_complex
        x = torch.from_numpy(msc.parity_audio(n_fft, n_frames, channels).copy()).to(dev)
        _SPECS[key] = stft_complex(x, n_fft, n_fft // 4)
        assert _SPECS[key].shape == (3 * channels, n_frames, n_fft // 2 + 1)
    return _SPECS[key]


def _bits(t):
    """A tensor as its 32-bit words: equality of these is equality bit for bit (NaN payloads and the sign of zero included)."""
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _params(ck, extra=None):
    from audiodenoiser_amd.dereverb import WpeStreamParams
    return WpeStreamParams(**msc.params_of(ck, extra))


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


def _mag_is_of_spec_out(got_h, mag_h):
    """mag_out (n, F, T) is, bit for bit, sqrtf(fmaf(re, re, im * im)) of the device's own spec_out (n, T, F), evaluated in float32
    on the host: the header defines M_{t,c} as that function of e_c, and the kernel computes it from the value it stores."""
    assert mag_h.dtype == np.float32 and got_h.dtype == np.complex64
    assert np.array_equal(mag_h.view(np.int32), np.sqrt(ds._power(got_h, np.float32)).transpose(0, 2, 1).view(np.int32))


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tuple(msc.parity_cases()), ids=msc.case_id)
def test_parity_with_the_float64_restatement(dev, case):
    from audiodenoiser_amd.dereverb import wpe_online_joint
    n_fft, n_frames, ck, extra = case
    channels, f = ck[0], n_fft // 2 + 1
    spec = _spec(dev, n_fft, n_frames, channels)
    label = rb.mc_label(n_fft, n_frames, ck, extra)
    bounds = rb.wpe_mc_online_bounds(spec.cpu().numpy(), channels, msc.params_of(ck, extra))   # on the downloaded device spectrogram
    rb.assert_cap(label, bounds)
    want = [bounds.ref[g * channels:(g + 1) * channels] for g in range(3)]     # ms.wpe_mc_online(group, params) in float64
    col0, width = 5, n_frames + 9
    nan = _bits(torch.full((1,), float("nan"), device=dev))
    for n_groups in msc.PARITY_GROUPS:
        n = n_groups * channels
        mag = torch.full((n, 1, f, width), float("nan"), device=dev)
        got, mag_out, state = wpe_online_joint(spec[:n].contiguous(), channels, params=_params(ck, extra), mag_out=mag, col0=col0)
        assert got.shape == (n, n_frames, f) and got.dtype == torch.complex64 and mag_out is mag and state.dtype == torch.uint8
        got_h, mag_h = got.cpu().numpy(), mag.cpu().numpy()[:, 0]
        sb.check(f"{label} [groups {n_groups}]", got_h, bounds.ref[:n], bounds)
        _mag_is_of_spec_out(got_h, mag_h[:, :, col0:col0 + n_frames])
        # the poisoned columns outside [col0, col0 + T) are untouched
        assert bool((_bits(mag[..., :col0]) == nan).all()) and bool((_bits(mag[..., col0 + n_frames:]) == nan).all())
        for g in range(n_groups):
            rows = slice(g * channels, (g + 1) * channels)
            scale = float(np.abs(want[g]).max())
            err = float(np.abs(got_h[rows].astype(np.complex128) - want[g]).max())
            err_m = float(np.abs(mag_h[rows][:, :, col0:col0 + n_frames].astype(np.float64) - np.abs(want[g]).transpose(0, 2, 1)).max())
            print(f"{msc.case_id(case)} groups {n_groups} group {g}: d {err / scale:.3g} of max |d| ({err / scale / ms.FLOOR:.2f} floors), "
                  f"M {err_m / scale / ms.FLOOR:.2f} floors; bound 4")
            assert err <= 4.0 * ms.FLOOR * scale, (n_groups, g, err / scale)
            assert err_m <= 4.0 * ms.FLOOR * scale, (n_groups, g, err_m / scale)


@pytest.mark.parametrize("case", tuple(msc.variant_cases()), ids=msc.case_id)
def test_parity_at_the_channel_counts_the_grid_does_not_reach(dev, case):
    """C = 5, 6, 7 (tests/variant_cover.py): N = 30, 30, 28 at the defaults taps = 32 // C, rows of P idle, records and rings of no
    round size; (5, 2) and (7, 1) the short rings.  Per bin only: dereverb_mc_stream_ref.FLOOR is measured over the parity grid.
    At T = 4 <= D + 1 the floor is 2^-23 or close to it: the pass-through of the first D frames is held exactly."""
    from audiodenoiser_amd.dereverb import wpe_online_joint
    n_fft, n_frames, ck, extra = case
    channels, f = ck[0], n_fft // 2 + 1
    spec = _spec(dev, n_fft, n_frames, channels)
    label = rb.mc_label(n_fft, n_frames, ck, extra, "variant")
    bounds = rb.wpe_mc_online_bounds(spec.cpu().numpy(), channels, msc.params_of(ck, extra))   # on the downloaded device spectrogram
    rb.assert_cap(label, bounds)
    col0, width = 5, n_frames + 9
    nan = _bits(torch.full((1,), float("nan"), device=dev))
    for n_groups in msc.PARITY_GROUPS:
        n = n_groups * channels
        mag = torch.full((n, 1, f, width), float("nan"), device=dev)
        got, mag_out, state = wpe_online_joint(spec[:n].contiguous(), channels, params=_params(ck, extra), mag_out=mag, col0=col0)
        assert got.shape == (n, n_frames, f) and got.dtype == torch.complex64 and mag_out is mag
        got_h, mag_h = got.cpu().numpy(), mag.cpu().numpy()[:, 0]
        delay = 3
        assert _same(got[:, :delay], spec[:n, :delay])                             # the first D frames: X itself
        sb.check(f"{label} [groups {n_groups}]", got_h, bounds.ref[:n], bounds)
        _mag_is_of_spec_out(got_h, mag_h[:, :, col0:col0 + n_frames])
        assert bool((_bits(mag[..., :col0]) == nan).all()) and bool((_bits(mag[..., col0 + n_frames:]) == nan).all())


@pytest.mark.parametrize("ck", rb.TILTED_MC, ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, ck):
    """80 dB from the first bin to the last, built on the host and uploaded: the group-wide bound allows the quiet bins an error of
    their own size -- a last bin that returns its input passes it (tests/test_recursive_bounds_host.py).  There is no power-of-two
    case beside it: P_0 = 1 / delta and the 1e-30 in phi_t are absolute, so the operator is not scale invariant."""
    from audiodenoiser_amd.dereverb import wpe_online_joint
    channels = ck[0]
    spec_h = sb.scale_spec(rb.mc_spec(64, rb.TILTED_FRAMES, channels), sb.tilt(33))
    bounds = rb.wpe_mc_online_bounds(spec_h, channels, msc.params_of(ck))
    label = rb.mc_label(64, rb.TILTED_FRAMES, ck, None, "tilted")
    rb.assert_cap(label, bounds)
    for n_groups in msc.PARITY_GROUPS:
        n = n_groups * channels
        got, mag, _ = wpe_online_joint(_upload(dev, spec_h[:n]), channels, params=_params(ck))
        got_h = got.cpu().numpy()
        sb.check(f"{label} [groups {n_groups}]", got_h, bounds.ref[:n], bounds)
        _mag_is_of_spec_out(got_h, mag.cpu().numpy()[:, 0])


# ---- 2. exact pins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", ((2, 16), (8, 4), (3, 7)), ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_repeat_cuts_batch_and_poisoned_state_are_exact(dev, ck):
    from audiodenoiser_amd.dereverb import wpe_online_joint, wpe_stream_state_bytes_joint
    n_frames, f, channels = 97, 257, ck[0]
    spec = _spec(dev, 512, n_frames, channels)
    p = _params(ck)
    full, full_mag, full_state = wpe_online_joint(spec, channels, params=p)
    again, again_mag, again_state = wpe_online_joint(spec, channels, params=p)
    assert _same(again, full) and _same(again_mag, full_mag) and torch.equal(again_state, full_state)           # two calls
    rows = slice(channels, 2 * channels)
    alone, alone_mag, alone_state = wpe_online_joint(spec[rows].contiguous(), channels, params=p)
    assert _same(alone, full[rows]) and _same(alone_mag, full_mag[rows])                                        # a group alone
    per = full_state.numel() // 3
    assert alone_state.numel() == per and torch.equal(alone_state, full_state[per:2 * per])                     # ... in another slot
    # a state filled with NaN (0xFF bytes) before a first_frame = 0 call changes nothing
    poisoned = torch.full((wpe_stream_state_bytes_joint(3, channels, f, p),), 0xFF, dtype=torch.uint8, device=dev)
    got, got_mag, st = wpe_online_joint(spec, channels, state=poisoned, params=p)
    assert st is poisoned and _same(got, full) and _same(got_mag, full_mag) and torch.equal(poisoned, full_state)
    # the frames cut into calls of 1, of B = 4 and of irregular sizes, the state carried
    for cuts in ((1,) * n_frames, (4,) * 24 + (1,), (7, 1, 30, 23, 36)):
        parts, mags, state, at = [], [], None, 0
        for n in cuts:
            d, m, state = wpe_online_joint(spec[:, at:at + n].contiguous(), channels, state=state, first_frame=at, params=p)
            parts.append(d)
            mags.append(m)
            at += n
        assert at == n_frames
        assert _same(torch.cat(parts, dim=1), full) and _same(torch.cat(mags, dim=3), full_mag), cuts
        assert torch.equal(state, full_state), cuts


@pytest.mark.parametrize("ck", ((2, 16), (4, 8)), ids=lambda ck: f"C{ck[0]}K{ck[1]}")
def test_a_bin_gives_the_same_bits_whichever_bins_share_the_call(dev, ck):
    from audiodenoiser_amd.dereverb import wpe_online_joint
    spec = _spec(dev, 512, 40, ck[0])
    p = _params(ck)
    full, full_mag, _ = wpe_online_joint(spec, ck[0], params=p)
    for lo, hi in ((0, 33), (100, 133), (0, 1), (256, 257), (250, 257)):            # bins repacked contiguous and run alone
        part, part_mag, _ = wpe_online_joint(spec[:, :, lo:hi].contiguous(), ck[0], params=p)
        assert _same(part, full[:, :, lo:hi]) and _same(part_mag, full_mag[:, :, lo:hi]), (lo, hi)


@pytest.mark.parametrize("kw", (None, dict(taps=1, delay=1), dict(taps=32, delay=8, forget=0.95)), ids=("defaults", "smallest", "largest"))
def test_one_channel_is_wpe_online_bit_for_bit(dev, kw):
    from audiodenoiser_amd.dereverb import WpeStreamParams, wpe_online, wpe_online_joint
    spec = _spec(dev, 64, 97, 2)[:3].contiguous()
    p = WpeStreamParams(**(kw or {}))
    want, want_mag, want_state = wpe_online(spec, params=p)
    got, got_mag, got_state = wpe_online_joint(spec, 1, params=p)
    assert _same(got, want) and _same(got_mag, want_mag) and torch.equal(got_state, want_state)
    # ... and continues it: the state is the single-channel one
    more, _, _ = wpe_online_joint(spec, 1, state=got_state, first_frame=97, params=p)
    assert _same(more, wpe_online(spec, state=want_state, first_frame=97, params=p)[0])


# ---- 3. zeros and non-finite values --------------------------------------------------------------------------------------------------
def test_first_frames_zero_groups_and_non_finite_values(dev):
    from audiodenoiser_amd.dereverb import WpeStreamParams, wpe_online_joint
    channels = 2
    spec = _spec(dev, 64, 23, channels)                                             # (6, 23, 33): three groups
    for delay in (1, 3, 8):                                                         # the first D frames: bit for bit
        got, _, _ = wpe_online_joint(spec, channels, params=WpeStreamParams(taps=5, delay=delay))
        assert _same(got[:, :delay], spec[:, :delay]) and not _same(got[:, delay:], spec[:, delay:])
    clean, clean_mag, _ = wpe_online_joint(spec, channels)
    zeroed = spec.clone()
    zeroed[2:4] = 0                                                                 # group 1, all channels and bins
    got, mag, _ = wpe_online_joint(zeroed, channels)
    assert bool((_bits(got[2:4]) == 0).all()) and bool((mag[2:4] == 0).all())
    assert _same(got[:2], clean[:2]) and _same(got[4:], clean[4:])
    for bad in (float("nan"), float("inf")):                                        # confined to its own (group, bin), all channels of it
        row, bin_, frame = 3, 30, 11                                                # channel 1 of group 1
        poisoned = spec.clone()
        poisoned[row, frame, bin_] = complex(bad, 0.25)
        got, mag, _ = wpe_online_joint(poisoned, channels)
        keep = torch.ones((6, 33), dtype=torch.bool, device=dev)
        keep[2:4, bin_] = False
        assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep]) and _same(mag[:, 0][keep], clean_mag[:, 0][keep])
        assert _same(got[2:4, :frame, bin_], clean[2:4, :frame, bin_])
        assert not bool(torch.isfinite(torch.view_as_real(got[2:4, -1, bin_])).all())


# ---- 4. StreamDereverberator(channels=C) ---------------------------------------------------------------------------------------------
def _sd(dev, **kw):
    from audiodenoiser_amd.dereverb import StreamDereverberator
    return StreamDereverberator(dev, **kw)


def _push_all(sd, xd, sizes):
    outs, pos = [], 0
    for size in sizes:
        outs.append(sd.push(xd[:, pos:pos + size]))
        pos += size
    assert pos >= xd.shape[1]
    outs.append(sd.flush())
    return torch.cat(outs, dim=1)


_WHOLE = {}
C2 = msc.E2E_CHANNELS


def _whole(dev, n_fft, gain):
    """The three end-to-end recordings of (n_fft, gain) through one object of 3 x C streams, pushed whole: computed once."""
    if (n_fft, gain) not in _WHOLE:
        xd = torch.from_numpy(msc.parity_audio(n_fft, msc.E2E_FRAMES, C2).copy()).to(dev)
        sd = _sd(dev, n_streams=3 * C2, channels=C2, n_fft=n_fft, hop_length=n_fft // 4, gain=gain)
        assert sd.params.taps == 32 // C2 and sd.channels == C2
        _WHOLE[n_fft, gain] = (xd, _push_all(sd, xd, [xd.shape[1]]))
    return _WHOLE[n_fft, gain]


@pytest.mark.parametrize("n_fft,gain", tuple(msc.e2e_cases()))
def test_stream_against_the_float64_end_to_end_form(dev, n_fft, gain):
    xd, got = _whole(dev, n_fft, gain)
    assert got.shape == xd.shape and got.is_cuda and got.dtype == torch.float32
    got_h = got.cpu().numpy().astype(np.float64)
    for g in range(3):
        want = msc.e2e_want(n_fft, gain, g)
        for c in range(C2):
            err, scale = float(np.abs(got_h[g * C2 + c] - want[c]).max()), float(np.abs(want[c]).max())
            print(f"n_fft {n_fft} gain {gain} recording {g} channel {c}: {err / scale:.3g} of the maximum "
                  f"({err / scale / ms.FLOOR_AUDIO:.2f} floors; bound 4)")
            assert err <= 4.0 * ms.FLOOR_AUDIO * scale, (g, c, err / scale)


@pytest.mark.parametrize("gain", (False, True))
def test_any_cut_into_pushes_neighbours_and_reset_give_the_same_bits(dev, gain):
    for n_fft, blocks in ((64, (1, 4)), (512, (4,))):
        xd, whole = _whole(dev, n_fft, gain)
        length = xd.shape[1]
        for block in blocks:
            kw = dict(n_fft=n_fft, hop_length=n_fft // 4, gain=gain, block_frames=block, channels=C2)
            three = _sd(dev, n_streams=3 * C2, **kw)
            ref = _push_all(three, xd, [length])
            assert torch.equal(ref, whole), (n_fft, block)                           # across block sizes
            assert torch.equal(_push_all(three, xd, [100] * (-(-length // 100))), ref), (n_fft, block)
            solo = _sd(dev, n_streams=C2, **kw)
            for g in range(3):                                                      # recording g of 3 is a solo recording
                one = xd[g * C2:(g + 1) * C2].contiguous()
                alone = _push_all(solo, one, [length])
                assert torch.equal(alone, ref[g * C2:(g + 1) * C2]), (n_fft, block, g)
                if n_fft == 64 and g == 1 and block == 4:
                    assert torch.equal(_push_all(solo, one, [1] * length), alone), "pushes of one sample"
            # reset() in mid-stream, then the same audio: the same bits
            three.push(xd[:, :length // 2])
            three.reset()
            assert torch.equal(_push_all(three, xd, [length]), ref)
    with pytest.raises(RuntimeError):
        _sd(dev, n_streams=2, channels=2).network(None)


def test_channels_1_is_the_single_channel_object_and_the_joint_one_differs(dev):
    from audiodenoiser_amd.dereverb import wpe_stream_state_bytes, wpe_stream_state_bytes_joint
    xd, whole = _whole(dev, 64, False)
    kw = dict(n_streams=6, n_fft=64, hop_length=16)
    plain, one = _sd(dev, **kw), _sd(dev, channels=1, **kw)
    assert one.params == plain.params and one.params.taps == 20 and one.channels == 1
    assert one._wpe_state.numel() == plain._wpe_state.numel() == wpe_stream_state_bytes(6, 33)
    assert _sd(dev, channels=2, **kw)._wpe_state.numel() == wpe_stream_state_bytes_joint(3, 2, 33)
    want = _push_all(plain, xd, [xd.shape[1]])
    assert torch.equal(_push_all(one, xd, [700, xd.shape[1] - 700]), want)
    assert not torch.equal(want, whole)


def test_input_rate_48000_returns_as_many_samples_as_it_was_given(dev):
    length = 30011
    wet, _ = mc.recording(2)
    x = torch.from_numpy(wet[:, :length].copy()).to(dev)
    sd = _sd(dev, n_streams=2, channels=2, input_rate=48000)
    assert sd.input_rate == 48000 and sd.sample_rate == 8000
    got = _push_all(sd, x, [4800, 7, 12000, 13204])
    assert got.shape == (2, length) and bool(torch.isfinite(got).all())
    assert torch.equal(_push_all(sd, x, [length]), got)


# ---- 5. quality ------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_two_microphone_recording(dev):
    from audiodenoiser_amd.metrics import evaluate
    wet, dry = mc.recording(2)
    xd, dd = torch.from_numpy(wet.copy()).to(dev), torch.from_numpy(np.stack([dry, dry])).to(dev)
    out = _push_all(_sd(dev, n_streams=2, channels=2), xd, [1024] * (-(-xd.shape[1] // 1024)))
    assert out.shape == xd.shape and bool(torch.isfinite(out).all())
    r_in, r_out = msc.restatement_si_sdr("input"), msc.restatement_si_sdr("joint stream, C = 2, K = 16")
    before, after = (evaluate(a, dd, sr=8000)["si_sdr"] for a in (xd, out))
    for c in range(2):
        print(f"channel {c}: SI-SDR on the device {float(before[c]):.2f} -> {float(after[c]):.2f} dB "
              f"(the restatement's: {r_in[c]:.2f} -> {r_out[c]:.2f})")
        assert r_out[c] - r_in[c] > 0.0                          # the cap means something only if the restatement gains
        assert float(after[c]) - float(before[c]) >= 0.5 * (r_out[c] - r_in[c])


# ---- 6. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames,ck,extra", ((512, 23, (2, 16), None), (64, 4, (3, 7), None), (64, 23, (8, 4), dict(delay=8)),
                                                    (64, 23, (7, 4), None)))
def test_online_writes_only_what_the_call_owns(dev, n_fft, n_frames, ck, extra):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import wpe_online_joint, wpe_stream_state_bytes_joint
    channels, groups, f = ck[0], 2, n_fft // 2 + 1
    n = groups * channels
    spec = _spec(dev, n_fft, n_frames, channels)[:n].contiguous()
    p = _params(ck, extra)
    ps = ctypes.byref(p.to_struct())
    plain, plain_mag, plain_state = wpe_online_joint(spec, channels, params=p)
    need = wpe_stream_state_bytes_joint(groups, channels, f, p)
    width, col0 = n_frames + 7, 3
    out, h_out = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    mag, h_mag = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    state, h_state = fp.carve(need, 0xFF, dev)
    src, h_src = fp.carve_copy(torch.view_as_real(spec), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = _lib.load()
    assert L.adn_wpe_mc_online(src.data_ptr(), groups, channels, n_frames, f, 0, ps, state.data_ptr(), need, groups, out.data_ptr(),
                               mag.data_ptr(), width, col0, stream) == 0
    torch.cuda.synchronize(dev)
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_state, "state"), (h_src, "spec")):
        fp.assert_guards_intact(h, what)
    assert _same(src, torch.view_as_real(spec))
    assert _same(torch.view_as_complex(out), plain) and _same(mag[..., col0:col0 + n_frames], plain_mag) and torch.equal(state, plain_state)
    assert bool((mag.view(torch.int32)[..., :col0] == -1).all()) and bool((mag.view(torch.int32)[..., col0 + n_frames:] == -1).all())
    # mag_out = NULL: spec_out and the state are written, the same bits; a refused call writes nothing
    out2, h_out2 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    state2, h_state2 = fp.carve(need, 0xFF, dev)
    assert L.adn_wpe_mc_online(src.data_ptr(), groups, channels, n_frames, f, 0, ps, state2.data_ptr(), need, groups, out2.data_ptr(), None,
                               0, 0, stream) == 0
    torch.cuda.synchronize(dev)
    fp.assert_guards_intact(h_out2, "spec_out")
    fp.assert_guards_intact(h_state2, "state")
    assert _same(out2, out) and torch.equal(state2, state)
    out3, h_out3 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    state3, h_state3 = fp.carve(need, 0xFF, dev)
    for args in ((src.data_ptr(), groups, channels, n_frames, f, -1, ps, state3.data_ptr(), need, groups, out3.data_ptr(), None, 0, 0),
                 (src.data_ptr(), groups, channels, n_frames, f, 0, ps, state3.data_ptr(), need - 1, groups, out3.data_ptr(), None, 0, 0),
                 (src.data_ptr(), groups, channels, n_frames, f, 0, ps, state3.data_ptr(), need, 1, out3.data_ptr(), None, 0, 0),
                 (src.data_ptr(), groups, channels, n_frames, f, 0, ps, state3.data_ptr(), need, groups, src.data_ptr(), None, 0, 0)):
        assert L.adn_wpe_mc_online(*args, stream) in (1, 3) and L.adn_last_error().startswith(b"adn_wpe_mc_online:"), args
    torch.cuda.synchronize(dev)
    assert fp.keeps_fill(h_out3, 0xFF) and fp.keeps_fill(h_state3, 0xFF)


@pytest.mark.parametrize("gain", (False, True))
def test_stream_writes_only_its_columns_and_its_states(dev, gain):
    """The class with its device states carved out of guarded, NaN-poisoned allocations: the same bits, the guards intact, of the
    windows buffer only the columns [W - B, W) change, adn_wpe_mc_stream at one channel is adn_wpe_stream, and refused calls leave
    the fill."""
    from audiodenoiser_amd import _lib
    xd, whole = _whole(dev, 64, gain)
    length = xd.shape[1]
    sd = _sd(dev, n_streams=3 * C2, channels=C2, n_fft=64, hop_length=16, gain=gain)
    state, h_state = fp.carve(sd._state.numel(), 0xFF, dev)
    wstate, h_wstate = fp.carve(sd._wpe_state.numel(), 0xFF, dev)
    sd._state, sd._wpe_state = state, wstate
    sd.reset()                                                   # clears the stream state; the WPE state keeps its NaNs
    assert fp.keeps_fill(h_wstate, 0xFF)
    with fp.carved_outputs(dev) as made:
        got = _push_all(sd, xd, [700, length - 700])
    torch.cuda.synchronize(dev)
    assert torch.equal(got, whole) and made
    for h in made:
        fp.assert_guards_intact(h, "a buffer of the stream")
    fp.assert_guards_intact(h_state, "stream state")
    fp.assert_guards_intact(h_wstate, "WPE state")
    # of the windows, only the block's columns change
    w, b = sd.window_frames, sd.block_frames
    sd.reset()
    win = sd.analyze(xd.contiguous(), length, 0, 2)              # steps 0 and 1 of a new stream: frames 0 ... 2 B - 1
    before = win.clone()
    after = sd._net(win, 0, 2)
    assert after is win and _same(after[..., :w - b], before[..., :w - b]) and not _same(after[..., w - b:], before[..., w - b:])
    sd.reset()

    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ps = ctypes.byref(sd.params.to_struct())
    # one channel through adn_wpe_mc_stream is adn_wpe_stream: the same bits in the windows, the ring and the WPE state
    one = _sd(dev, n_streams=3 * C2, n_fft=64, hop_length=16)
    p1 = ctypes.byref(one.params.to_struct())
    results = []
    for name, extra in (("adn_wpe_stream", ()), ("adn_wpe_mc_stream", (1,))):
        one.reset()
        one._wpe_state.fill_(0xFF)
        win1 = one.analyze(xd.contiguous(), length, 0, 2)
        assert getattr(L, name)(one._state.data_ptr(), one._state.numel(), win1.data_ptr(), 3 * C2, *extra, 0, 2, -1, *one._plan,
                                one.max_steps, p1, one._wpe_state.data_ptr(), one._wpe_state.numel(), stream) == 0, name
        torch.cuda.synchronize(dev)
        results.append((win1.clone(), one._state.clone(), one._wpe_state.clone()))
    for a, b_ in zip(*results):
        assert _same(a, b_) if a.dtype != torch.uint8 else torch.equal(a, b_)
    # refused calls return 1 or 3 and leave the fill
    sstate, h_s = fp.carve(sd._state.numel(), 0xFF, dev)
    y, h_y = fp.carve_tensor((3 * C2 * 2, 1, 33, w), 0xFF, dev)
    ws, h_w = fp.carve(sd._wpe_state.numel(), 0xFF, dev)
    n_fft, hop, window, block, _ = sd._plan
    for n_streams, channels, plan, wbytes in ((3 * C2 - 1, C2, sd._plan, ws.numel()), (3 * C2, C2, (n_fft, hop, window, block, 1), ws.numel()),
                                              (3 * C2, C2, sd._plan, ws.numel() - 1), (3 * C2, 9, sd._plan, ws.numel())):
        rc = L.adn_wpe_mc_stream(sstate.data_ptr(), sstate.numel(), y.data_ptr(), n_streams, channels, 0, 2, -1, *plan, sd.max_steps, ps,
                                 ws.data_ptr(), wbytes, stream)
        assert rc in (1, 3) and L.adn_last_error().startswith(b"adn_wpe_mc_stream:"), (n_streams, channels, plan, wbytes)
    torch.cuda.synchronize(dev)
    assert fp.keeps_fill(h_s, 0xFF) and fp.keeps_fill(h_y, 0xFF) and fp.keeps_fill(h_w, 0xFF)


# ---- 7. seven channels: the lockstep stream against the online form, and no parameters against the library's NULL --------------------
def test_stream_is_online_bit_for_bit_and_writes_nothing_else_at_seven_channels(dev):
    """adn_wpe_mc_stream at (C, K) = (7, 4), the least round record: every step of a StreamDereverberator over two recordings is
    compared, call by call, with adn_wpe_mc_online on the ring's own spectrogram -- the ring cells, the kept columns of the windows
    and the WPE state bit for bit, and not one byte else.  The ring is the first section of the stream state: [stream][RX][F]
    float2, frame t at t mod RX, RX = max_steps * block (csrc/stream_kernels.hip)."""
    from audiodenoiser_amd.dereverb import StreamDereverberator, wpe_online_joint
    c, f, hop, block, n_frames = 7, 33, 16, 4, 23
    length = (n_frames - 1) * hop + 5                            # 23 frames: five whole blocks and one of three frames

    class Traced(StreamDereverberator):
        online_state, calls = None, 0

        def ring(self):
            n, rx = self.n_streams, self.max_steps * self.block_frames
            return torch.view_as_complex(self._state.view(torch.float32)[:n * rx * f * 2].view(n, rx, f, 2))

        def _net(self, x, first_step, n_steps, final_length=-1):
            n, w, b = self.n_streams, self.window_frames, self.block_frames
            rx = self.max_steps * b
            end = (first_step + n_steps) * b
            if final_length >= 0:
                end = min(end, 1 + final_length // self.hop_length)
            frames = list(range(first_step * b, end))
            idx = [t % rx for t in frames]
            ring = self.ring()
            spec = ring[:, idx].clone()
            x_before, ring_before = x.clone(), ring.clone()
            d, m, self.online_state = wpe_online_joint(spec, c, state=self.online_state, first_frame=frames[0], params=self.params)
            super()._net(x, first_step, n_steps, final_length)
            kept = x.view(n, n_steps, f, w)[..., w - b:].permute(0, 2, 1, 3).reshape(n, 1, f, n_steps * b)
            assert _same(ring[:, idx], d) and _same(kept[..., :len(frames)], m), (first_step, n_steps)
            assert torch.equal(self._wpe_state, self.online_state), (first_step, n_steps)
            x_want, ring_want = x_before.clone(), ring_before.clone()
            want_kept = x_want.view(n, n_steps, f, w)[..., w - b:].permute(0, 2, 1, 3).reshape(n, 1, f, n_steps * b).clone()
            want_kept[..., :len(frames)] = m
            x_want.view(n, n_steps, f, w)[..., w - b:] = want_kept.view(n, f, n_steps, b).permute(0, 2, 1, 3)
            ring_want[:, idx] = d
            assert _same(x, x_want) and _same(ring, ring_want) and not _same(x, x_before), (first_step, n_steps)
            Traced.calls += 1
            return x

    xd = torch.from_numpy(msc.parity_audio(64, n_frames, c)[:2 * c, :length].copy()).to(dev)
    sd = Traced(dev, n_streams=2 * c, channels=c, n_fft=64, hop_length=hop, block_frames=block, params=_params((c, 4)))
    got = _push_all(sd, xd, [200, length - 200])
    torch.cuda.synchronize(dev)
    assert Traced.calls >= 2 and got.shape == (2 * c, length) and bool(torch.isfinite(got).all())
    plain = _sd(dev, n_streams=2 * c, channels=c, n_fft=64, hop_length=hop, block_frames=block)       # no parameters: taps = 32 // 7
    assert torch.equal(_push_all(plain, xd, [length]), got)


@pytest.mark.parametrize("channels", (5, 6, 7), ids=lambda c: f"C{c}")
def test_no_parameters_is_the_library_s_null_at_five_six_and_seven_channels(dev, channels):
    """taps = 32 // C is stated twice, by joint_default_taps of the library and by the Python classes: with no parameters the
    online call and the stream class give, bit for bit, what the ABI gives for params = NULL."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import WpeStreamParams, wpe_online_joint, wpe_stream_state_bytes_joint
    c, f, n_frames = channels, 33, 23
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    spec = _spec(dev, 64, n_frames, c)[:c].contiguous()
    want, want_mag, want_state = wpe_online_joint(spec, c)                          # Python's default
    need = ctypes.c_size_t(0)
    assert L.adn_wpe_mc_stream_state_bytes(1, c, f, None, ctypes.byref(need)) == 0
    assert need.value == want_state.numel() == wpe_stream_state_bytes_joint(1, c, f, WpeStreamParams(taps=32 // c))
    out = torch.empty((c, n_frames, f, 2), device=dev)
    mag = torch.empty((c, 1, f, n_frames), device=dev)
    state = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=dev)
    assert L.adn_wpe_mc_online(torch.view_as_real(spec).data_ptr(), 1, c, n_frames, f, 0, None, state.data_ptr(), need.value, 1,
                               out.data_ptr(), mag.data_ptr(), n_frames, 0, stream) == 0
    torch.cuda.synchronize(dev)
    assert _same(torch.view_as_complex(out), want) and _same(mag, want_mag) and torch.equal(state, want_state)
    assert not _same(wpe_online_joint(spec, c, params=WpeStreamParams(taps=32 // c - 1))[0], want)
    # the class: its own step, adn_wpe_mc_stream with its parameters, and adn_wpe_mc_stream with NULL
    sd = _sd(dev, n_streams=c, channels=c, n_fft=64, hop_length=16)
    assert sd.params == WpeStreamParams(taps=32 // c) and sd._wpe_state.numel() == need.value
    xd = torch.from_numpy(msc.parity_audio(64, n_frames, c)[:c].copy()).to(dev)
    results = []
    for p in ("class", ctypes.byref(sd.params.to_struct()), None):
        sd.reset()
        sd._wpe_state.fill_(0xFF)
        win = sd.analyze(xd.contiguous(), xd.shape[1], 0, 2)
        if p == "class":
            sd._net(win, 0, 2)
        else:
            assert L.adn_wpe_mc_stream(sd._state.data_ptr(), sd._state.numel(), win.data_ptr(), c, c, 0, 2, -1, *sd._plan, sd.max_steps, p,
                                       sd._wpe_state.data_ptr(), sd._wpe_state.numel(), stream) == 0
        torch.cuda.synchronize(dev)
        results.append((win.clone(), sd._state.clone(), sd._wpe_state.clone()))
    for other in results[1:]:
        for a, b_ in zip(results[0], other):
            assert _same(a, b_) if a.dtype != torch.uint8 else torch.equal(a, b_)
    sd.reset()


# ---- 8. command line -------------------------------------------------------------------------------------------------------------
def test_command_line_live_joint(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.wav import read_wav, write_wav
    wet, dry = mc.recording(2)
    wet, dry = wet[:, :12352], dry[:12352]
    src, ref, dst = (str(tmp_path / n) for n in ("room2ch.wav", "dry.wav", "out.wav"))
    write_wav(src, np.ascontiguousarray(wet.T), 8000, "PCM_16")
    write_wav(ref, dry, 8000, "PCM_16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.dereverb", src, dst, "--live", "--joint", "--reference", ref], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out, rate = read_wav(dst, mono=False)
    assert rate == 8000 and out.shape == (12352, 2)
    assert "latency 896 samples" in run.stdout
    row = json.loads(run.stdout.strip().splitlines()[-1])
    each_in, each_out = row["noisy"]["si_sdr_per_channel"], row["denoised"]["si_sdr_per_channel"]
    print(f"SI-SDR of the 1.5 s two-channel clip, live and joint: {each_in} -> {each_out} dB")
    assert len(each_in) == len(each_out) == 2 and np.isfinite(each_out).all() and np.isfinite(row["denoised"]["si_sdr"])
    # the joint form is not the per-channel one, and it is what the class gives for the same pushes
    sep = str(tmp_path / "separate.wav")
    run2 = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.dereverb", src, sep, "--live"], cwd=root, capture_output=True,
                          text=True, timeout=300)
    assert run2.returncode == 0, run2.stderr[-2000:]
    assert not np.array_equal(read_wav(sep, mono=False)[0], out)
