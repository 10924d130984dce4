"""Spectral baseline on the device (csrc/baseline_kernels.hip, audiodenoiser_amd/baseline.py) against the float64 restatement in
tests/baseline_ref.py.

Bounds (derived, not tuned):
* adn_spectral_gain, per clip: max |M_dev - M_64| <= 4 FLOOR max M_64.  FLOOR (baseline_ref.FLOOR) is the error of the same
  statements run in float32 on the host over these very shapes (python tests/baseline_cases.py), never a device figure; the factor
  4 is the project's convention from the quality metrics.  The restatement is applied to the DOWNLOADED device spectrogram, so the
  STFT's own error does not enter.
* adn_spectral_gain, per (clip, bin): E = max_t |M_dev - M_64| / max_t M_64 <= 4 floor for every bin of every clip, beside the bound
  above (tests/recursive_bounds.py), and every entry of the state (clip, row of P / Pmin / S, bin) likewise against its own float64
  value.  The floor is the case's own: the largest E of the float32 restatement on the same downloaded spectrogram over every bin of
  the case's three clips, measured when the test runs, never below 2^-23, never from the device, and asserted under the cap of 1e-4.
  The operator has one arithmetic (contraction off, one step), so both floor columns of the printed line hold the same figure.  The
  same bound holds the tilted cases (an 80 dB slope over the bins, built on the host and uploaded), and a power of two per bin,
  2^-((5 b) mod 13), has to come back bit for bit: M scaled by the factor, the state by its square.
* Chunk, batch and isolation tests: exact equality, as include/adn.h pins them.
* End to end, in two links: the device's audio against the restatement's resynthesis fed the device's own magnitudes within the
  tree's inverse-STFT tolerance TOL = 1e-4 of max |ref| (tests/test_gpu_denoise.py::test_resynth); and against the whole float64
  restatement within TOL max |ref| plus the parity bound carried through: a magnitude error of at most d in every bin moves a
  frame's samples by at most d (the inverse real FFT averages its N bins), and the overlap-add divides sum w x by sum w^2 with
  sum w <= 2 and sum w^2 >= 0.25 over [0, L) at hop <= n_fft / 4: a factor of at most 8, so 8 x 4 FLOOR max M_64.
* Quality: a cap, not parity -- the device's SI-SDR gain on the 8 dB white mix is at least half the restatement's.
Measured on the MI355X: parity uses at most 0.47 of a floor (bound 4), typically 0.05; the resynthesis link 2.3e-7 of the maximum;
the whole chain 5.4e-8 absolute at worst; SI-SDR 7.98 -> 13.70 dB, the restatement's gain to the printed digits.
Per bin (profiles/recursive_bins.md): M at most 1.00 of the case's floor (bound 4), at least 0.71 (T = 1, where the floor is 2^-23);
the state 1.00 in every one of the 39 cases, the tilted and the power-of-two case included -- the device's worst E is the float32
restatement's own to the printed digits.  Every parity case takes under 0.2 s with its floor.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_cases as bc  # noqa: E402
import baseline_ref as br  # noqa: E402
import denoise_ref  # noqa: E402
import footprint as fp  # noqa: E402
import recursive_bounds as rb  # noqa: E402
import solver_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _spec(dev, n_fft, n_frames, n_clips):
    """The device's own STFT of the parity audio: (device complex64 (n, T, F), host complex128)."""
    from audiodenoiser_amd.griffin_lim import stft_complex
    x = torch.from_numpy(bc.parity_audio(n_fft, n_frames, n_clips)).to(dev)
    spec = stft_complex(x, n_fft, n_fft // 4)
    assert spec.shape == (n_clips, n_frames, n_fft // 2 + 1)
    return spec, spec.cpu().numpy().astype(np.complex128)


def _raw(spec, out, col0=0, params=None, state_in=None, state_out=None, n_frames=None, frame0=0):
    """adn_spectral_gain itself, on frames [frame0, frame0 + n_frames) of every clip; returns the status."""
    from audiodenoiser_amd import _lib
    n, t, f = spec.shape
    n_frames = t if n_frames is None else n_frames
    part = spec[:, frame0:frame0 + n_frames].contiguous()
    s = torch.view_as_real(part)
    rc = _lib.load().adn_spectral_gain(s.data_ptr(), n, n_frames, f, params, state_in.data_ptr() if state_in is not None else None,
                                       state_out.data_ptr() if state_out is not None else None, out.data_ptr(), int(out.shape[-1]),
                                       col0, torch.cuda.current_stream(spec.device).cuda_stream)
    torch.cuda.synchronize(spec.device)
    return rc


def _check(label, got, state, bounds):
    """The per-bin bound on the first clips of a case: M (n, 1, F, T) and the state (n, 3, F) of the device against the case's
    float64 restatement, each within 4 floors of the case's own float32 floor, the floors under the cap."""
    n = got.shape[0]
    rb.assert_cap(label, bounds)
    rb.assert_cap(label + " state", bounds.state)
    sb.check(f"{label} [clips {n}]", got.cpu().numpy()[:, 0].transpose(0, 2, 1), bounds.ref[:n], bounds)
    sb.check(f"{label} state [clips {n}]", rb.state_rows(state.cpu().numpy()), bounds.state.ref[:3 * n], bounds.state)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", bc.PARITY_FRAMES)
@pytest.mark.parametrize("n_fft", bc.PARITY_N_FFT)
def test_parity_with_the_float64_restatement(dev, n_fft, n_frames):
    from audiodenoiser_amd.baseline import spectral_gain
    spec3, spec3_h = _spec(dev, n_fft, n_frames, 3)
    bounds = rb.spectral_bounds(spec3.cpu().numpy())               # the floor of the case: on the downloaded device spectrogram
    for n_clips in bc.PARITY_CLIPS:
        spec, spec_h = spec3[:n_clips].contiguous(), spec3_h[:n_clips]
        got, state = spectral_gain(spec)
        assert got.shape == (n_clips, 1, n_fft // 2 + 1, n_frames) and got.dtype == torch.float32
        assert state.shape == (n_clips, 3, n_fft // 2 + 1)
        _check(rb.gain_label(n_fft, n_frames), got, state, bounds)
        got_h, state_h = got.cpu().numpy().astype(np.float64)[:, 0], state.cpu().numpy().astype(np.float64)
        for c in range(n_clips):
            want, want_state = br.spectral_gain(spec_h[c])
            err, scale = float(np.abs(got_h[c] - want).max()), float(want.max())
            print(f"n_fft {n_fft} T {n_frames} clips {n_clips} clip {c}: max err {err:.3g} = {err / scale:.3g} of max M "
                  f"({err / scale / br.FLOOR:.2f} floors; bound 4)")
            assert err <= 4.0 * br.FLOOR * scale, (n_clips, c, err / scale)
            # the state is the same recurrence: P, Pmin and S against their own largest value
            for row in range(3):
                assert np.abs(state_h[c, row] - want_state[row]).max() <= 4.0 * br.FLOOR * np.abs(want_state[row]).max(), (c, row)


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n_fft", rb.TILTED_GAIN)
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, n_fft):
    """80 dB from the first bin to the last, built on the host and uploaded: the clip-wide bound allows the quiet bins an error of
    their own size, and a wrong gain_floor, gamma or alpha in the last bin alone passes it (tests/test_recursive_bounds_host.py)."""
    from audiodenoiser_amd.baseline import spectral_gain
    spec_h = sb.scale_spec(rb.gain_spec(n_fft, rb.TILTED_FRAMES), sb.tilt(n_fft // 2 + 1))
    bounds = rb.spectral_bounds(spec_h)
    for n_clips in bc.PARITY_CLIPS:
        got, state = spectral_gain(_upload(dev, spec_h[:n_clips]))
        _check(rb.gain_label(n_fft, rb.TILTED_FRAMES, "tilted"), got, state, bounds)


def test_a_power_of_two_per_bin_comes_back_bit_for_bit(dev):
    """Every rule of the operator is a ratio or is homogeneous in p_t, and the 1e-30 under N_t is far below every power here, so
    2^-k times a bin's input is 2^-k times its magnitudes and 2^-2k times its state, exactly
    (tests/test_recursive_bounds_host.py checks that the float32 restatement has the property; here no square leaves the normal
    range).  There is no such case for adn_wpe_online and adn_wpe_mc_online: P_0 = 1 / delta and the 1e-30 in phi_t are absolute,
    so those two operators are not scale invariant."""
    from audiodenoiser_amd.baseline import spectral_gain
    base, f = rb.gain_spec(rb.POW2_GAIN, rb.TILTED_FRAMES), sb.pow2(rb.POW2_GAIN // 2 + 1)
    scaled = sb.scale_spec(base, f)
    sb.assert_squares_stay_normal(base, scaled)
    ft = _upload(dev, f.astype(np.float32))
    plain, plain_state = spectral_gain(_upload(dev, base))
    got, state = spectral_gain(_upload(dev, scaled))
    sb.assert_squares_stay_normal(plain.cpu().numpy(), got.cpu().numpy(), plain_state.cpu().numpy(), state.cpu().numpy())
    assert _same_bits(got, plain * ft[None, None, :, None])
    assert _same_bits(state, plain_state * (ft * ft)[None, None, :])
    _check(rb.gain_label(rb.POW2_GAIN, rb.TILTED_FRAMES, "pow2"), got, state, rb.spectral_bounds(scaled))


# ---- 2. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames", ((512, 1), (512, 33), (64, 70)))
def test_footprint_only_the_columns_of_the_call(dev, n_fft, n_frames):
    from audiodenoiser_amd.baseline import spectral_gain
    n, f = 2, n_fft // 2 + 1
    spec, _ = _spec(dev, n_fft, n_frames, n)
    plain, plain_state = spectral_gain(spec)
    col0, width = 5, 5 + n_frames + 7
    out, h_out = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    state, h_state = fp.carve_tensor((n, 3, f), 0xFF, dev)
    assert _raw(spec, out, col0=col0, state_out=state) == 0
    fp.assert_guards_intact(h_out, "out")
    fp.assert_guards_intact(h_state, "state_out")
    assert torch.equal(out[..., col0:col0 + n_frames], plain) and torch.equal(state, plain_state)
    untouched = out.view(torch.int32)
    assert bool((untouched[..., :col0] == -1).all()) and bool((untouched[..., col0 + n_frames:] == -1).all())
    # without a state_out nothing but `out` is written, and a NULL state_in equals an all-fresh one
    out2, h_out2 = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    fresh = torch.full((n, 3, f), -1.0, device=dev)
    assert _raw(spec, out2, col0=col0, state_in=fresh) == 0
    fp.assert_guards_intact(h_out2, "out")
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and bool((fresh == -1.0).all())


def test_short_clip_through_the_denoiser_leaves_the_padding_zero(dev):
    from audiodenoiser_amd.baseline import SpectralDenoiser, spectral_gain
    dn = SpectralDenoiser(dev)
    for n_frames in (1, 15, 16, 40):
        spec, _ = _spec(dev, 512, n_frames, 2)
        with fp.carved_outputs(dev) as made:
            y = dn.gain(spec)
        for h in made:
            fp.assert_guards_intact(h, "gain")
        assert y.shape == (2, 1, 257, max(n_frames, 16))
        assert torch.equal(y[..., :n_frames], spectral_gain(spec)[0]) and bool((y[..., n_frames:] == 0).all())


# ---- 3. chunk invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames", ((512, 130), (64, 188)))
def test_chunk_invariance_is_exact(dev, n_fft, n_frames):
    from audiodenoiser_amd.baseline import spectral_gain
    n, f = 2, n_fft // 2 + 1
    spec, _ = _spec(dev, n_fft, n_frames, 3)
    spec = spec[:n].contiguous()
    whole, whole_state = spectral_gain(spec)
    for cuts in ((1, 8, 40), (bc.TILE, 2 * bc.TILE, 3 * bc.TILE), (n_frames - 1,)):
        # carried through new tensors, by the Python face
        st, lo = None, 0
        out = torch.full((n, 1, f, n_frames), float("nan"), device=dev)
        for hi in cuts + (n_frames,):
            _, st = spectral_gain(spec[:, lo:hi], state=st, out=out, col0=lo)
            lo = hi
        assert torch.equal(out, whole) and torch.equal(st, whole_state), cuts
        # carried in place: state_in == state_out, the first call from the fresh-start sentinel
        st = torch.full((n, 3, f), -1.0, device=dev)
        out = torch.full((n, 1, f, n_frames), float("nan"), device=dev)
        lo = 0
        for hi in cuts + (n_frames,):
            assert _raw(spec, out, col0=lo, state_in=st, state_out=st, n_frames=hi - lo, frame0=lo) == 0
            lo = hi
        assert torch.equal(out, whole) and torch.equal(st, whole_state), cuts
    assert torch.equal(spectral_gain(spec)[0], whole)                      # two calls: the same bits


# ---- 4. batch invariance, per-row start ------------------------------------------------------------------------------------------
def test_batch_invariance_and_per_row_start(dev):
    from audiodenoiser_amd.baseline import spectral_gain
    spec, _ = _spec(dev, 512, 97, 3)
    batch, batch_state = spectral_gain(spec)
    alone, alone_state = spectral_gain(spec[1:2].contiguous())
    assert torch.equal(alone[0], batch[1]) and torch.equal(alone_state[0], batch_state[1])
    # row 0 continues from a carried state, row 1 starts (P = -1, the other two rows holding anything)
    two = spec[:2].contiguous()
    _, carried = spectral_gain(two[:1, :40].contiguous())
    state = torch.full((2, 3, 257), float("nan"), device=dev)
    state[0] = carried[0]
    state[1, 0] = -1.0
    mixed, mixed_state = spectral_gain(two[:, 40:].contiguous(), state=state)
    cont, cont_state = spectral_gain(two[:1, 40:].contiguous(), state=carried)
    fresh, fresh_state = spectral_gain(two[1:, 40:].contiguous())
    assert torch.equal(mixed[0], cont[0]) and torch.equal(mixed_state[0], cont_state[0])
    assert torch.equal(mixed[1], fresh[0]) and torch.equal(mixed_state[1], fresh_state[0])
    assert torch.equal(cont[0], batch[0, ..., 40:])                        # and the continued row is the uncut one


# ---- 5. isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_a_non_finite_value_poisons_its_own_row_only(dev, bad):
    from audiodenoiser_amd.baseline import spectral_gain
    spec, _ = _spec(dev, 512, 70, 3)
    clean, clean_state = spectral_gain(spec)
    clip, bin_, frame = 1, 130, 37
    poisoned = spec.clone()
    poisoned[clip, frame, bin_] = complex(bad, 0.25)
    got, state = spectral_gain(poisoned)
    keep = torch.ones((3, 257), dtype=torch.bool, device=dev)
    keep[clip, bin_] = False
    assert torch.equal(got[:, 0][keep], clean[:, 0][keep])
    assert torch.equal(state.transpose(1, 2)[keep], clean_state.transpose(1, 2)[keep])
    assert torch.equal(got[clip, 0, bin_, :frame], clean[clip, 0, bin_, :frame])
    assert bool(torch.isnan(got[clip, 0, bin_, frame:]).all()) and not bool(torch.isfinite(state[clip, :, bin_]).any())


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,n_clips", ((24000, 1), (2047, 1), (100, 1), (24000, 2)))
def test_end_to_end(dev, length, n_clips):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import SpectralDenoiser, spectral_gain
    from audiodenoiser_amd.griffin_lim import stft_complex
    dn = SpectralDenoiser(dev)
    x = np.stack([bc.white_mix(8000 + length, 8.0, 50 + c)[0][8000:] for c in range(n_clips)])         # stereo: two clips
    assert x.shape == (n_clips, length)
    xd = torch.from_numpy(x).to(dev)
    out = dn.denoise(xd)
    assert out.shape == xd.shape and out.is_cuda and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    # bit-identical to the public pieces composed by hand
    n_frames = 1 + length // 128
    spec = stft_complex(xd, 512, 128)
    y = torch.zeros((n_clips, 1, 257, max(n_frames, 16)), device=dev)
    spectral_gain(spec, out=y)
    by_hand = torch.empty((n_clips, length), device=dev)
    _lib.check(_lib.load().adn_denoise_resynth(y.data_ptr(), torch.view_as_real(spec).data_ptr(), n_clips, length, 512, 128,
                                               max(n_frames, 16), 0, by_hand.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               "adn_denoise_resynth")
    assert torch.equal(out, by_hand)
    spec_h, y_h = spec.cpu().numpy().astype(np.complex128), y.cpu().numpy().astype(np.float64)[:, 0, :, :n_frames]
    got = out.cpu().numpy().astype(np.float64)
    for c in range(n_clips):
        link = denoise_ref.istft(denoise_ref.rephase(y_h[c], spec_h[c]), 128, length)     # the device's magnitudes, float64 way back
        e_link = float(np.abs(got[c] - link).max() / np.abs(link).max())
        want = br.denoise(x[c].astype(np.float64), 512, 128, spec=spec_h[c])
        m64 = br.spectral_gain(spec_h[c])[0]
        e_all, bound = float(np.abs(got[c] - want).max()), TOL * float(np.abs(want).max()) + 8 * 4 * br.FLOOR * float(m64.max())
        print(f"end to end L {length} clip {c}: resynthesis link {e_link:.3g} (TOL {TOL}), whole {e_all:.3g} (bound {bound:.3g})")
        assert e_link <= TOL and e_all <= bound
    # numpy in -> numpy out, (L,) in -> (L,) out, the same values
    one = dn.denoise(x[0])
    assert isinstance(one, np.ndarray) and one.shape == (length,) and one.dtype == np.float32
    assert np.array_equal(one, dn.denoise(xd[:1]).cpu().numpy()[0])


def test_other_rate_comes_back_at_its_length(dev):
    from audiodenoiser_amd.baseline import SpectralDenoiser
    dn = SpectralDenoiser(dev)
    x = torch.from_numpy(np.stack([bc.white_mix(33001, 8.0, 60)[0]])).to(dev)
    out = dn.denoise(x, sr=16000)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())


def test_file_and_command_line(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.baseline import SpectralDenoiser
    from audiodenoiser_amd.wav import read_wav, write_wav
    noisy, clean = bc.quality_case(8.0, seconds=2.0)
    src, ref, dst, dst_cli = (str(tmp_path / n) for n in ("noisy.wav", "clean.wav", "out.wav", "out_cli.wav"))
    write_wav(src, noisy, 8000, "PCM_16")
    write_wav(ref, clean, 8000, "PCM_16")
    assert SpectralDenoiser(dev).denoise_file(src, dst) == (16000, 8000)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.baseline", src, dst_cli, "--reference", ref], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert np.array_equal(read_wav(dst_cli)[0], read_wav(dst)[0])
    row = json.loads(run.stdout.strip().splitlines()[-1])
    assert row["denoised"]["si_sdr"] > row["noisy"]["si_sdr"] + 1.0


# ---- 7. quality ------------------------------------------------------------------------------------------------------------------
def test_si_sdr_gain_on_the_8_db_white_mix(dev):
    from audiodenoiser_amd.baseline import SpectralDenoiser
    from audiodenoiser_amd.metrics import evaluate
    noisy, clean = bc.quality_case(8.0)
    want_gain = br.si_sdr(br.denoise(noisy.astype(np.float64), 512, 128), clean) - br.si_sdr(noisy, clean)
    nd, cd = torch.from_numpy(noisy).to(dev), torch.from_numpy(clean).to(dev)
    out = SpectralDenoiser(dev).denoise(nd)
    before, after = float(evaluate(nd, cd, sr=8000)["si_sdr"][0]), float(evaluate(out, cd, sr=8000)["si_sdr"][0])
    print(f"SI-SDR on the device: {before:.2f} -> {after:.2f} dB (gain {after - before:.2f}; the restatement's {want_gain:.2f})")
    assert want_gain >= 3.0 and after - before >= 0.5 * want_gain


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import SpectralParams
    spec, _ = _spec(dev, 64, 17, 2)
    out, h = fp.carve_tensor((2, 1, 33, 32), 0xFF, dev)
    st, h_st = fp.carve_tensor((2, 3, 33), 0xFF, dev)
    L = _lib.load()
    for name, value in (("smooth", 1.0), ("beta", -0.1), ("gamma", 0.0), ("alpha", 1.5), ("gain_floor", 0.0), ("bias", 101.0),
                        ("bias", float("nan"))):
        s = SpectralParams().to_struct()
        setattr(s, name, value)
        assert _raw(spec, out, params=ctypes.byref(s), state_out=st) == 1 and name.encode() in L.adn_last_error()
    assert _raw(spec, out, col0=16, state_out=st) == 1                      # 16 + 17 > 32
    assert _raw(spec, out, col0=-1, state_out=st) == 1
    assert _raw(spec, out, n_frames=0, state_out=st) == 1
    s = torch.view_as_real(spec)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for args in ((None, 2, 17, 33, None, None, st.data_ptr(), out.data_ptr(), 32, 0), (s.data_ptr(), 2, 17, 33, None, None, st.data_ptr(), None, 32, 0),
                 (s.data_ptr(), 0, 17, 33, None, None, st.data_ptr(), out.data_ptr(), 32, 0), (s.data_ptr(), 2, 17, 0, None, None, st.data_ptr(), out.data_ptr(), 32, 0),
                 (s.data_ptr() + 4, 2, 16, 33, None, None, st.data_ptr(), out.data_ptr(), 32, 0)):
        assert L.adn_spectral_gain(*args, stream) == 1
    torch.cuda.synchronize(dev)
    assert fp.keeps_fill(h, 0xFF) and fp.keeps_fill(h_st, 0xFF)
    fp.assert_guards_intact(h, "out")
    with pytest.raises(ValueError):
        from audiodenoiser_amd.baseline import spectral_gain
        spectral_gain(spec.cpu())


# ---- the building blocks of the window plan, which this class does not have ---------------------------------------------------------
def test_the_network_s_building_blocks_refuse_and_leave_the_object_usable(dev):
    """No model and no window plan: what ``Denoiser`` builds around its network says so (a ``RuntimeError``, the stream variants'
    sentence) before it looks at its argument, and the object denoises afterwards as before."""
    from audiodenoiser_amd.baseline import SpectralDenoiser
    dn = SpectralDenoiser(dev)
    y = torch.zeros((1, 1, 33, 16), device=dev)
    spec = torch.zeros((1, 3, 33), dtype=torch.complex64, device=dev)
    for call in (lambda: dn.network(y), lambda: dn.windows(spec), lambda: dn.plan(40),
                 lambda: dn.denoise_spectrogram(torch.zeros((33, 16), device=dev)), lambda: dn.stitch(y, 1, 16, False),
                 lambda: dn.resynth(y, spec, 600)):
        with pytest.raises(RuntimeError, match=r"^SpectralDenoiser: there is no network"):
            call()
    out = dn.denoise(bc.white_mix(600, 8.0, 5)[0].astype(np.float32))
    assert out.shape == (600,) and out.dtype == np.float32 and np.isfinite(out).all()
