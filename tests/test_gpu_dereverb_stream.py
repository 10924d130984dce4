"""Streaming dereverberation on the device (csrc/dereverb_stream_kernels.hip, audiodenoiser_amd/dereverb.py) against the float64
restatement in tests/dereverb_stream_ref.py.

Bounds (derived, not tuned):
* adn_wpe_online, per row: max |d_dev - d_64| <= 4 FLOOR max |d_64|.  FLOOR (dereverb_stream_ref.FLOOR) is the error of the same
  statements run in float32 on the host over these very cases (python tests/dereverb_stream_cases.py), never a device figure; the
  factor 4 is the project's standing margin.  The restatement is applied to the DOWNLOADED device spectrogram, so the STFT's own
  error does not enter.  mag_out likewise against |d_64|, on the same scale.
* adn_wpe_online, per (row, bin): E = max_t |d_dev - d_64| / max_t |d_64| <= 4 floor for every bin of every row, beside the bound
  above (tests/recursive_bounds.py).  The floor is the case's own: the largest E of the float32 restatement on the same downloaded
  spectrogram over every bin of the case's three rows and over two float32 arithmetics -- "plain" (every product rounded, what FLOOR
  was measured with; the "pairwise" column of the printed line) and "fma" (the header's pairing and order of every multiply-add; the
  "sequential" column) -- measured when the test runs, never below 2^-23 (which is what the cases with T <= D get, whose reference is
  the input bit for bit), never from the device, and asserted under the cap of 1e-4.  The same bound holds the tilted cases (an 80 dB
  slope over the bins, built on the host and uploaded) at the defaults and at the largest parameter set.  There is no power-of-two
  case: P_0 = 1 / delta and the 1e-30 in phi_t are absolute, the operator is not scale invariant.
* mag_out, bit for bit: sqrtf(fmaf(re, re, im * im)) of the device's own spec_out, evaluated in float32 on the host.
* StreamDereverberator, per stream: max |audio_dev - audio_64| <= 4 FLOOR_AUDIO max |audio_64|, FLOOR_AUDIO the error of the
  end-to-end form with every statement in float32 on the host, the two transforms included.
* Repeat, cut, batch, bin-subset, poisoned-state, pass-through, isolation, pool and reset tests: exact equality, as include/adn.h
  pins them.
Measured on the MI355X: parity uses at most 0.67 of a floor (bound 4): n_fft 64, T = 97, (K, D, alpha) = (32, 8, 0.95), row 2,
1.94e-6 of max |d|; at the defaults at most 0.15, the median over all 192 comparisons 0.01; mag_out at most 0.52 floors.  The
streams against the float64 end-to-end form: 1.8e-7 - 4.1e-7 of the maximum, 0.08 - 0.19 of the audio floor (bound 4).  The whole
file: 69 cases in 7.9 s, the command-line case 2.2 s, every other one under 0.5 s.  The rest: profiles/bench_dereverb_stream.md.
Per bin (profiles/recursive_bins.md): at most 1.00 of the case's floor (bound 4), reached at the largest parameter set at T = 97
(n_fft 64: row 2, bin 1, E 1.9e-6), where the fma arithmetic sets the floor and the device's worst E is that restatement's own to
the printed digits; at the defaults at most 0.52, the tilted cases 0.15 - 1.00, the median over the 48 parity cases 0.43.  With the floors
the file is 73 cases in 17 s: the n_fft 512 cases at the largest parameter set 2.2 s each (three host runs of K = 32 over 771 bins),
every other parity case under 1 s.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dereverb_cases as dc  # noqa: E402
import dereverb_stream_cases as sc  # noqa: E402
import dereverb_stream_ref as ds  # noqa: E402
import footprint as fp  # noqa: E402
import recursive_bounds as rb  # noqa: E402
import solver_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _spec(dev, n_fft, n_frames, n_rows):
    """The device's own STFT of the first rows of the parity audio: device complex64 (n, T, F)."""
    from audiodenoiser_amd.griffin_lim import stft_complex
    x = torch.from_numpy(sc.parity_audio(n_fft, n_frames, n_rows).copy()).to(dev)
    spec = stft_complex(x, n_fft, n_fft // 4)
    assert spec.shape == (n_rows, n_frames, n_fft // 2 + 1)
    return spec


def _bits(t):
    """A tensor as its 32-bit words: equality of these is equality bit for bit (NaN payloads and the sign of zero included)."""
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _params(kw):
    from audiodenoiser_amd.dereverb import WpeStreamParams
    return None if kw is None else WpeStreamParams(**kw)


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


def _mag_is_of_spec_out(got_h, mag_h):
    """mag_out (n, F, T) is, bit for bit, sqrtf(fmaf(re, re, im * im)) of the device's own spec_out (n, T, F), evaluated in float32
    on the host: the header defines M_t as that function of e_t, and the kernel computes it from the value it stores."""
    assert mag_h.dtype == np.float32 and got_h.dtype == np.complex64
    assert np.array_equal(mag_h.view(np.int32), np.sqrt(ds._power(got_h, np.float32)).transpose(0, 2, 1).view(np.int32))


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", sc.PARITY_PARAMS, ids=sc.PARAM_IDS)
@pytest.mark.parametrize("n_frames", sc.PARITY_FRAMES)
@pytest.mark.parametrize("n_fft", sc.PARITY_N_FFT)
def test_parity_with_the_float64_restatement(dev, n_fft, n_frames, kw):
    from audiodenoiser_amd.dereverb import wpe_online
    f = n_fft // 2 + 1
    spec = _spec(dev, n_fft, n_frames, 3)
    bounds = rb.wpe_online_bounds(spec.cpu().numpy(), kw)        # the floor of the case: on the downloaded device spectrogram
    rb.assert_cap(rb.online_label(n_fft, n_frames, kw), bounds)
    want = list(bounds.ref)                                      # ds.wpe_online(row, kw) in float64, row by row
    col0, width = 5, n_frames + 9
    for n_rows in sc.PARITY_ROWS:
        mag = torch.full((n_rows, 1, f, width), float("nan"), device=dev)
        got, mag_out, state = wpe_online(spec[:n_rows].contiguous(), params=_params(kw), mag_out=mag, col0=col0)
        assert got.shape == (n_rows, n_frames, f) and got.dtype == torch.complex64 and mag_out is mag and state.dtype == torch.uint8
        got_h, mag_h = got.cpu().numpy(), mag.cpu().numpy()[:, 0]
        sb.check(f"{rb.online_label(n_fft, n_frames, kw)} [rows {n_rows}]", got_h, bounds.ref[:n_rows], bounds)
        _mag_is_of_spec_out(got_h, mag_h[:, :, col0:col0 + n_frames])
        # the poisoned columns outside [col0, col0 + T) are untouched
        assert bool((_bits(mag[..., :col0]) == _bits(torch.full((1,), float("nan"), device=dev))).all())
        assert bool((_bits(mag[..., col0 + n_frames:]) == _bits(torch.full((1,), float("nan"), device=dev))).all())
        for c in range(n_rows):
            scale = float(np.abs(want[c]).max())
            err = float(np.abs(got_h[c].astype(np.complex128) - want[c]).max())
            err_m = float(np.abs(mag_h[c][:, col0:col0 + n_frames].astype(np.float64) - np.abs(want[c]).T).max())
            print(f"n_fft {n_fft} T {n_frames} {kw or 'defaults'} rows {n_rows} row {c}: d {err / scale:.3g} of max |d| "
                  f"({err / scale / ds.FLOOR:.2f} floors), M {err_m / scale / ds.FLOOR:.2f} floors; bound 4")
            assert err <= 4.0 * ds.FLOOR * scale, (n_rows, c, err / scale)
            assert err_m <= 4.0 * ds.FLOOR * scale, (n_rows, c, err_m / scale)


@pytest.mark.parametrize("kw", rb.TILTED_ONLINE_PARAMS, ids=("defaults", "largest"))
@pytest.mark.parametrize("n_fft", rb.TILTED_ONLINE)
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, n_fft, kw):
    """80 dB from the first bin to the last, built on the host and uploaded: the row-wide bound allows the quiet bins an error of
    their own size -- a last bin that returns its input passes it (tests/test_recursive_bounds_host.py).  There is no power-of-two
    case beside it: P_0 = 1 / delta and the 1e-30 in phi_t are absolute, so the operator is not scale invariant."""
    from audiodenoiser_amd.dereverb import wpe_online
    spec_h = sb.scale_spec(rb.online_spec(n_fft, rb.TILTED_FRAMES), sb.tilt(n_fft // 2 + 1))
    bounds = rb.wpe_online_bounds(spec_h, kw)
    label = rb.online_label(n_fft, rb.TILTED_FRAMES, kw, "tilted")
    rb.assert_cap(label, bounds)
    for n_rows in sc.PARITY_ROWS:
        got, mag, _ = wpe_online(_upload(dev, spec_h[:n_rows]), params=_params(kw))
        got_h = got.cpu().numpy()
        sb.check(f"{label} [rows {n_rows}]", got_h, bounds.ref[:n_rows], bounds)
        _mag_is_of_spec_out(got_h, mag.cpu().numpy()[:, 0])


# ---- 2. exact pins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", sc.PARITY_PARAMS, ids=sc.PARAM_IDS)
def test_repeat_cuts_batch_and_poisoned_state_are_exact(dev, kw):
    from audiodenoiser_amd.dereverb import wpe_online, wpe_stream_state_bytes
    n_frames, f = 97, 257
    spec = _spec(dev, 512, n_frames, 3)
    p = _params(kw)
    full, full_mag, full_state = wpe_online(spec, params=p)
    again, again_mag, again_state = wpe_online(spec, params=p)
    assert _same(again, full) and _same(again_mag, full_mag) and torch.equal(again_state, full_state)           # two calls
    alone, alone_mag, _ = wpe_online(spec[1:2].contiguous(), params=p)
    assert _same(alone[0], full[1]) and _same(alone_mag[0], full_mag[1])                                        # a row alone
    # a state filled with NaN (0xFF bytes) before a first_frame = 0 call changes nothing
    poisoned = torch.full((wpe_stream_state_bytes(3, f, p),), 0xFF, dtype=torch.uint8, device=dev)
    got, got_mag, st = wpe_online(spec, state=poisoned, params=p)
    assert st is poisoned and _same(got, full) and _same(got_mag, full_mag) and torch.equal(poisoned, full_state)
    # the frames cut into calls of 1, of B = 4 and of irregular sizes, the state carried
    for cuts in ((1,) * n_frames, (4,) * 24 + (1,), (7, 1, 30, 23, 36)):
        parts, mags, state, at = [], [], None, 0
        for n in cuts:
            d, m, state = wpe_online(spec[:, at:at + n].contiguous(), state=state, first_frame=at, params=p)
            parts.append(d)
            mags.append(m)
            at += n
        assert at == n_frames
        assert _same(torch.cat(parts, dim=1), full) and _same(torch.cat(mags, dim=3), full_mag), cuts
        assert torch.equal(state, full_state), cuts


@pytest.mark.parametrize("kw", (None, sc.PARITY_PARAMS[2]), ids=("defaults", "largest"))
def test_a_bin_gives_the_same_bits_whichever_bins_share_the_call(dev, kw):
    from audiodenoiser_amd.dereverb import wpe_online
    spec = _spec(dev, 512, 40, 3)
    p = _params(kw)
    full, full_mag, _ = wpe_online(spec, params=p)
    for lo, hi in ((0, 33), (100, 133), (0, 1), (256, 257), (7, 24), (250, 257)):      # bins repacked contiguous and run alone
        part, part_mag, _ = wpe_online(spec[:, :, lo:hi].contiguous(), params=p)
        assert _same(part, full[:, :, lo:hi]) and _same(part_mag, full_mag[:, :, lo:hi]), (lo, hi)


def test_first_frames_zero_rows_and_non_finite_values(dev):
    from audiodenoiser_amd.dereverb import WpeStreamParams, wpe_online
    spec = _spec(dev, 64, 40, 3)
    for delay in (1, 3, 8):                                                         # the first D frames: bit for bit
        got, _, _ = wpe_online(spec, params=WpeStreamParams(delay=delay))
        assert _same(got[:, :delay], spec[:, :delay]) and not _same(got[:, delay:], spec[:, delay:])
    clean, clean_mag, _ = wpe_online(spec)
    zeroed = spec.clone()
    zeroed[1, :, 17] = 0
    zeroed[2, :, 32] = 0
    got, mag, _ = wpe_online(zeroed)
    assert bool((_bits(got[1, :, 17]) == 0).all()) and bool((_bits(got[2, :, 32]) == 0).all())
    assert bool((mag[1, 0, 17] == 0).all()) and bool((mag[2, 0, 32] == 0).all())
    keep = torch.ones((3, 33), dtype=torch.bool, device=dev)
    keep[1, 17] = keep[2, 32] = False
    assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])
    for bad in (float("nan"), float("inf")):                                        # confined to its own (row, bin)
        row, bin_, frame = 1, 30, 21
        poisoned = spec.clone()
        poisoned[row, frame, bin_] = complex(bad, 0.25)
        got, mag, _ = wpe_online(poisoned)
        keep = torch.ones((3, 33), dtype=torch.bool, device=dev)
        keep[row, bin_] = False
        assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep]) and _same(mag[:, 0][keep], clean_mag[:, 0][keep])
        assert _same(got[row, :frame, bin_], clean[row, :frame, bin_])


# ---- 3. StreamDereverberator ---------------------------------------------------------------------------------------------------------
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


def _whole(dev, n_fft, gain):
    """The three end-to-end rows of (n_fft, gain) through one object of three streams, pushed whole: computed once."""
    if (n_fft, gain) not in _WHOLE:
        xd = torch.from_numpy(sc.parity_audio(n_fft, sc.E2E_FRAMES).copy()).to(dev)
        _WHOLE[n_fft, gain] = (xd, _push_all(_sd(dev, n_streams=3, n_fft=n_fft, hop_length=n_fft // 4, gain=gain), xd, [xd.shape[1]]))
    return _WHOLE[n_fft, gain]


@pytest.mark.parametrize("n_fft,gain", tuple(sc.e2e_cases()))
def test_stream_against_the_float64_end_to_end_form(dev, n_fft, gain):
    xd, got = _whole(dev, n_fft, gain)
    assert got.shape == xd.shape and got.is_cuda and got.dtype == torch.float32
    got_h = got.cpu().numpy().astype(np.float64)
    for c in range(3):
        want = sc.e2e_want(n_fft, gain, c)
        err, scale = float(np.abs(got_h[c] - want).max()), float(np.abs(want).max())
        print(f"n_fft {n_fft} gain {gain} stream {c}: {err / scale:.3g} of the maximum ({err / scale / ds.FLOOR_AUDIO:.2f} floors; bound 4)")
        assert err <= 4.0 * ds.FLOOR_AUDIO * scale, (c, err / scale)


@pytest.mark.parametrize("gain", (False, True))
def test_any_cut_into_pushes_neighbours_and_reset_give_the_same_bits(dev, gain):
    for n_fft, blocks in ((64, sc.E2E_BLOCKS), (512, (4,))):
        xd, whole = _whole(dev, n_fft, gain)
        length = xd.shape[1]
        for block in blocks:
            kw = dict(n_fft=n_fft, hop_length=n_fft // 4, gain=gain, block_frames=block)
            three = _sd(dev, n_streams=3, **kw)
            assert three.lookahead_frames == 0 and three.window_frames == 16
            ref = whole if block == 4 else _push_all(three, xd, [length])
            by_100 = _push_all(three, xd, [100] * (-(-length // 100)))
            assert torch.equal(by_100, ref), (n_fft, block)
            solo = _sd(dev, **kw)
            for c in range(3):                                                      # stream c of 3 is a solo stream of its samples
                one = xd[c:c + 1].contiguous()
                alone = _push_all(solo, one, [length])
                assert torch.equal(alone, ref[c:c + 1]), (n_fft, block, c)
                if n_fft == 64 and c == 1:
                    assert torch.equal(_push_all(solo, one, [1] * length), alone), "pushes of one sample"
            # reset() in mid-stream, then the same audio: the same bits
            three.push(xd[:, :length // 2])
            three.reset()
            assert torch.equal(_push_all(three, xd, [length]), ref)
    with pytest.raises(RuntimeError):
        _sd(dev).network(None)


def test_input_rate_48000_returns_as_many_samples_as_it_was_given(dev):
    length = 30011
    x = torch.from_numpy(dc.reverberant(32000, 60)[0][:length].copy()).to(dev)[None]
    sd = _sd(dev, input_rate=48000)
    assert sd.input_rate == 48000 and sd.sample_rate == 8000
    got = _push_all(sd, x, [4800, 7, 12000, 13204])
    assert got.shape == (1, length) and bool(torch.isfinite(got).all())
    assert torch.equal(_push_all(sd, x, [length]), got)


# ---- 4. DereverbStreamPool -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", (False, True))
def test_pool_streams_equal_solo_streams(dev, gain):
    """Staggered opens, uneven pushes (numpy and device tensors), one feed closed mid-way, a slot reused without a reset, one stream
    at 48 kHz."""
    from audiodenoiser_amd.dereverb import DereverbStreamPool
    pool = DereverbStreamPool(dev, max_streams=3, backlog_steps=16, gain=gain, input_rates=(48000,))
    assert pool.latency_samples == 896
    lengths, rates = (6000, 3100, 20000, 4000), (None, None, 48000, None)
    sig = [np.ascontiguousarray(dc.reverberant(32000, 90 + i)[0][4000:4000 + n]) for i, n in enumerate(lengths)]
    want = [_push_all(_sd(dev, gain=gain, input_rate=rates[i]), torch.from_numpy(s.copy()).to(dev)[None], [len(s)])[0].cpu()
            for i, s in enumerate(sig)]
    outs, sid, pos, by_sid = [[] for _ in sig], {}, [0] * 4, {}

    def take(result):
        for s, samples, finished in result:
            i = by_sid[s]
            outs[i].append(torch.from_numpy(samples) if isinstance(samples, np.ndarray) else samples.cpu())
            if finished:
                del by_sid[s]

    def open_(i):
        sid[i] = pool.open(rates[i])
        by_sid[sid[i]] = i

    def push(i, m):
        m = min(m, len(sig[i]) - pos[i], pool.room(sid[i]))
        block = sig[i][pos[i]:pos[i] + m]
        pool.push(sid[i], block if i % 2 == 0 else torch.from_numpy(block.copy()).to(dev))
        pos[i] += m

    open_(0)
    push(0, 700)
    take(pool.step())
    open_(1)
    open_(2)
    for m0, m1, m2 in ((1500, 3, 9000), (1, 2000, 1), (2000, 1097, 7000), (1799, 0, 3999)):
        push(0, m0)
        push(1, m1)
        push(2, m2)
        take(pool.step())
    assert pos[0] == 6000 and pos[1] == 3100
    pool.close(sid[0])                                           # closed while stream 2 is in mid-flight
    pool.close(sid[1])
    while 0 in by_sid.values() or 1 in by_sid.values():
        take(pool.step())
    open_(3)                                                     # the first stream's slot, left as it was: no reset
    assert sid[3] == sid[0]
    while pos[2] < lengths[2] or pos[3] < lengths[3]:
        push(2, 2500)
        push(3, 1234)
        take(pool.step())
    pool.close(sid[2])
    pool.close(sid[3])
    take(pool.drain())
    assert not by_sid and pool.step() == []
    for i in range(4):
        got = torch.cat(outs[i])
        assert got.shape == want[i].shape == (lengths[i],), (i, got.shape)
        assert torch.equal(got, want[i]), (i, float((got - want[i]).abs().max()))
    with pytest.raises(RuntimeError):
        pool.network(None)


# ---- 5. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames,kw", ((512, 40, None), (64, 5, None), (64, 40, sc.PARITY_PARAMS[2])))
def test_online_writes_only_what_the_call_owns(dev, n_fft, n_frames, kw):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import wpe_online, wpe_stream_state_bytes
    n, f = 2, n_fft // 2 + 1
    spec = _spec(dev, n_fft, n_frames, n)
    p = _params(kw)
    ps = ctypes.byref(p.to_struct()) if p is not None else None
    plain, plain_mag, plain_state = wpe_online(spec, params=p)
    need = wpe_stream_state_bytes(n, f, p)
    width, col0 = n_frames + 7, 3
    out, h_out = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    mag, h_mag = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    state, h_state = fp.carve(need, 0xFF, dev)
    src, h_src = fp.carve_copy(torch.view_as_real(spec), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = _lib.load()
    assert L.adn_wpe_online(src.data_ptr(), n, n_frames, f, 0, ps, state.data_ptr(), need, n, out.data_ptr(), mag.data_ptr(), width, col0,
                            stream) == 0
    torch.cuda.synchronize(dev)
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_state, "state"), (h_src, "spec")):
        fp.assert_guards_intact(h, what)
    assert _same(src, torch.view_as_real(spec))
    assert _same(torch.view_as_complex(out), plain) and _same(mag[..., col0:col0 + n_frames], plain_mag) and torch.equal(state, plain_state)
    assert bool((mag.view(torch.int32)[..., :col0] == -1).all()) and bool((mag.view(torch.int32)[..., col0 + n_frames:] == -1).all())
    # mag_out = NULL: spec_out and the state are written, the same bits; a refused call writes nothing
    out2, h_out2 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    state2, h_state2 = fp.carve(need, 0xFF, dev)
    assert L.adn_wpe_online(src.data_ptr(), n, n_frames, f, 0, ps, state2.data_ptr(), need, n, out2.data_ptr(), None, 0, 0, stream) == 0
    torch.cuda.synchronize(dev)
    fp.assert_guards_intact(h_out2, "spec_out")
    fp.assert_guards_intact(h_state2, "state")
    assert _same(out2, out) and torch.equal(state2, state)
    out3, h_out3 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    state3, h_state3 = fp.carve(need, 0xFF, dev)
    for args in ((src.data_ptr(), n, n_frames, f, -1, ps, state3.data_ptr(), need, n, out3.data_ptr(), None, 0, 0),
                 (src.data_ptr(), n, n_frames, f, 0, ps, state3.data_ptr(), need - 1, n, out3.data_ptr(), None, 0, 0),
                 (src.data_ptr(), n, n_frames, f, 0, ps, state3.data_ptr(), need, 1, out3.data_ptr(), None, 0, 0),
                 (src.data_ptr(), n, n_frames, f, 0, ps, state3.data_ptr(), need, n, src.data_ptr(), None, 0, 0)):
        assert L.adn_wpe_online(*args, stream) in (1, 3) and L.adn_last_error().startswith(b"adn_wpe_online:"), args
    torch.cuda.synchronize(dev)
    assert fp.keeps_fill(h_out3, 0xFF) and fp.keeps_fill(h_state3, 0xFF)


@pytest.mark.parametrize("gain", (False, True))
def test_stream_and_pool_write_only_their_columns_and_their_states(dev, gain):
    """The classes with their device states carved out of guarded, NaN-poisoned allocations: the same bits, the guards intact, and of
    the windows buffer only the columns [W - B, W) change."""
    from audiodenoiser_amd.dereverb import DereverbStreamPool
    xd, whole = _whole(dev, 64, gain)
    length = xd.shape[1]
    sd = _sd(dev, n_streams=3, n_fft=64, hop_length=16, gain=gain)
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
    sd.push(xd[:, :400])                                         # steps 0 ... of a new stream are behind us: analyse the next ones by hand
    k = sd._done
    base = (k * b - 1) * 16 + 32
    win = sd.analyze(xd[:, base:].contiguous(), length - base, k, 2)
    before = win.clone()
    after = sd._net(win, k, 2)
    assert after is win and _same(after[..., :w - b], before[..., :w - b]) and not _same(after[..., w - b:], before[..., w - b:])
    sd.reset()

    pool = DereverbStreamPool(dev, max_streams=2, backlog_steps=8, n_fft=64, hop_length=16, gain=gain)
    pstate, h_pstate = fp.carve(pool._state.numel(), 0xFF, dev)
    pwstate, h_pwstate = fp.carve(pool._wpe_state.numel(), 0xFF, dev)
    pool._state, pool._wpe_state = pstate, pwstate
    pool.reset()
    assert fp.keeps_fill(h_pwstate, 0xFF)
    outs = {}
    with fp.carved_outputs(dev) as made:
        for c in (0, 1):
            s = pool.open()
            outs[s] = []
            pos = 0
            while pos < length:                                  # the first stream still drains while the second one is fed
                m = min(pool.room(s), length - pos, 300 + 100 * c)
                pool.push(s, xd[c, pos:pos + m])
                pos += m
                for sid, samples, _ in pool.step():
                    outs[sid].append(samples)
            pool.close(s)
        for sid, samples, _ in pool.drain():
            outs[sid].append(samples)
    torch.cuda.synchronize(dev)
    for h in made:
        fp.assert_guards_intact(h, "a buffer of the pool")
    fp.assert_guards_intact(h_pstate, "pool state")
    fp.assert_guards_intact(h_pwstate, "WPE state of the pool")
    assert sorted(outs) == [0, 1]
    for c, sid in enumerate(sorted(outs)):
        assert torch.equal(torch.cat(outs[sid]), whole[c]), c


# ---- 6. command line -------------------------------------------------------------------------------------------------------------
def test_command_line_live(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.wav import read_wav, write_wav
    wet, dry = (v[:12352] for v in dc.quality_case())
    src, ref, dst = (str(tmp_path / n) for n in ("room.wav", "dry.wav", "out.wav"))
    write_wav(src, wet, 8000, "PCM_16")
    write_wav(ref, dry, 8000, "PCM_16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.dereverb", src, dst, "--live", "--reference", ref], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out, rate = read_wav(dst)
    assert rate == 8000 and out.shape[0] == 12352
    assert "latency 896 samples" in run.stdout
    row = json.loads(run.stdout.strip().splitlines()[-1])
    print(f"SI-SDR of the 1.5 s clip, live: {row['noisy']['si_sdr']:.2f} -> {row['denoised']['si_sdr']:.2f} dB")
    assert np.isfinite(row["denoised"]["si_sdr"])
