"""The echo canceller on the device (csrc/echo_stream_kernels.hip, audiodenoiser_amd/echo.py) against the float64 restatement in
tests/echo_ref.py.

* adn_aec_online, per (row, bin): E = max_t |e_dev - e_64| / max_t |e_64| <= 4 floor (tests/solver_bounds.py `per_bin` / `check`),
  the floor the case's own: the larger E of the float32 restatement in its two arithmetics on the very spectrograms the device ran
  on (they are built on the host and uploaded), measured when the test runs, never below 2^-23, never a device figure, capped at
  1e-4 (tests/recursive_bounds.py).  The same on spectra tilted by 80 dB.
* Pinned bit for bit: two calls; any cut of the frames into calls; a row alone or in a batch, in any slot; a bin whichever bins
  share the call, for each of the three lane layouts; mag_out against its own spec_out; a state handed over full of NaN.
* The header's consequences: R = 0, Y = 0, a NaN, the gate, a minute with a silent far end.
* adn_aec_stream: bit for bit adn_aec_online on the rings' own spectrograms, and not one byte else -- in particular none of the
  far-end stream's ring or windows; the classes' guarantees; the float64 chain end to end; quality; the command line.

Measured on the MI355X (profiles/bench_echo.md): parity and tilt use at most 1.00 of a case's floor (bound 4; median 0.30 over the
128 runs); the minute with a silent far end 1.00 of the float32 restatement's own error; the end-to-end audio at most 3.03 audio
floors (n_fft 512, pair 1: 5.96e-6 of the maximum against a floor of 1.97e-6; the other rows 0.7 ... 2.6); ERLE 19.08 dB and SI-SDR
3.57 -> 22.19 dB on the result's own STFT, the float64 chain's figures to the printed digits.  The cases run in 17 s, the
command-line case 6.4 s (three processes), every other one under 1.4 s.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import echo_cases as ec  # noqa: E402
import echo_ref as er  # noqa: E402
import footprint as fp  # noqa: E402
import recursive_bounds as rb  # noqa: E402
import solver_bounds as sb  # noqa: E402
from dereverb_stream_ref import _power  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (ec.PARITY_PARAMS[0], ec.PARITY_PARAMS[3], ec.PARITY_PARAMS[5])        # G = 8, 16, 32
LAYOUT_IDS = ("G8", "G16", "G32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _bits(t):
    """A tensor as its 32-bit words: equality of these is equality bit for bit (NaN payloads and the sign of zero included)."""
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _params(kw):
    from audiodenoiser_amd.echo import AecParams
    return None if kw is None else AecParams(**kw)


def _upload(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)                # a writable copy: the cases are read-only


def _online(mic, far, kw=None, **more):
    from audiodenoiser_amd.echo import aec_online
    return aec_online(mic.contiguous(), far.contiguous(), params=_params(kw), **more)


def _mag_is_of_spec_out(got_h, mag_h):
    """mag_out (n, F, T) is, bit for bit, sqrtf(fmaf(re, re, im * im)) of the device's own spec_out (n, T, F) in float32."""
    assert mag_h.dtype == np.float32 and got_h.dtype == np.complex64
    assert np.array_equal(mag_h.view(np.int32), np.sqrt(_power(got_h, np.float32)).transpose(0, 2, 1).view(np.int32))


def _pair(dev, n_fft, n_frames):
    mic, far = ec.parity_spec(n_fft, n_frames)
    return _upload(dev, mic), _upload(dev, far)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", ec.PARITY_PARAMS, ids=ec.PARAM_IDS)
@pytest.mark.parametrize("n_fft,n_frames", [(n, t) for n in ec.PARITY_N_FFT for t in ec.PARITY_FRAMES[n]])
def test_parity_with_the_float64_restatement(dev, n_fft, n_frames, kw):
    f = n_fft // 2 + 1
    mic_h, far_h = ec.parity_spec(n_fft, n_frames)
    bounds = ec.aec_bounds(mic_h, far_h, kw)
    rb.assert_cap(ec.label(n_fft, n_frames, kw), bounds)
    mic, far = _upload(dev, mic_h), _upload(dev, far_h)
    col0, width = 5, n_frames + 9
    for n_rows in ec.PARITY_ROWS:
        mag = torch.full((n_rows, 1, f, width), float("nan"), device=dev)
        got, mag_out, state = _online(mic[:n_rows], far[:n_rows], kw, mag_out=mag, col0=col0)
        assert got.shape == (n_rows, n_frames, f) and got.dtype == torch.complex64 and mag_out is mag and state.dtype == torch.uint8
        got_h, mag_h = got.cpu().numpy(), mag.cpu().numpy()[:, 0]
        sb.check(f"{ec.label(n_fft, n_frames, kw)} [rows {n_rows}]", got_h, bounds.ref[:n_rows], bounds)
        _mag_is_of_spec_out(got_h, mag_h[:, :, col0:col0 + n_frames])
        nan = _bits(torch.full((1,), float("nan"), device=dev))
        assert bool((_bits(mag[..., :col0]) == nan).all()) and bool((_bits(mag[..., col0 + n_frames:]) == nan).all())


@pytest.mark.parametrize("kw", ec.SHORT_PARAMS, ids=ec.SHORT_IDS)
@pytest.mark.parametrize("n_frames", ec.SHORT_FRAMES)
def test_short_rows_with_an_active_far_end(dev, n_frames, kw):
    """The grid's cases of up to five frames have a silent far end (tests/echo_cases.py): these have the same frame counts and an
    active one, so the update runs from the first frame on, in every lane layout."""
    mic_h, far_h = ec.short_spec(n_frames)
    bounds = ec.aec_bounds(mic_h, far_h, kw)
    label = ec.label(64, n_frames, kw, "short")
    rb.assert_cap(label, bounds)
    for n_rows in ec.PARITY_ROWS:
        got, mag, _ = _online(_upload(dev, mic_h[:n_rows]), _upload(dev, far_h[:n_rows]), kw)
        got_h = got.cpu().numpy()
        assert n_frames == 1 or not np.array_equal(got_h, mic_h[:n_rows])            # the filter has moved: e is not Y
        sb.check(f"{label} [rows {n_rows}]", got_h, bounds.ref[:n_rows], bounds)
        _mag_is_of_spec_out(got_h, mag.cpu().numpy()[:, 0])


@pytest.mark.parametrize("kw", ec.TILTED_PARAMS, ids=("defaults", "largest"))
@pytest.mark.parametrize("n_fft,n_frames", ((64, ec.TILTED_FRAMES), (512, 40)))
def test_a_tilted_spectrum_is_held_bin_by_bin(dev, n_fft, n_frames, kw):
    """80 dB from the first bin to the last on both inputs.  loading and quiet are absolute, so the operator is not scale invariant:
    the quiet bins are more heavily regularised and their frames are gated more often, in the restatement as on the device."""
    mic_h, far_h = (ec.tilted(s) for s in ec.parity_spec(n_fft, n_frames))
    bounds = ec.aec_bounds(mic_h, far_h, kw)
    label = ec.label(n_fft, n_frames, kw, "tilted")
    rb.assert_cap(label, bounds)
    for n_rows in ec.PARITY_ROWS:
        got, mag, _ = _online(_upload(dev, mic_h[:n_rows]), _upload(dev, far_h[:n_rows]), kw)
        got_h = got.cpu().numpy()
        sb.check(f"{label} [rows {n_rows}]", got_h, bounds.ref[:n_rows], bounds)
        _mag_is_of_spec_out(got_h, mag.cpu().numpy()[:, 0])


# ---- 2. exact pins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", ec.PARITY_PARAMS, ids=ec.PARAM_IDS)
def test_repeat_cuts_batch_slot_and_poisoned_state_are_exact(dev, kw):
    from audiodenoiser_amd.echo import aec_stream_state_bytes
    n_frames, f = 97, 33
    mic, far = _pair(dev, 64, n_frames)
    p = _params(kw)
    full, full_mag, full_state = _online(mic, far, kw)
    again, again_mag, again_state = _online(mic, far, kw)
    assert _same(again, full) and _same(again_mag, full_mag) and torch.equal(again_state, full_state)           # two calls
    per = aec_stream_state_bytes(1, f, p)
    for rows in ((1,), (2, 0), (1, 2)):                                                                         # alone, in other slots
        sel = list(rows)
        part, part_mag, part_state = _online(mic[sel], far[sel], kw)
        assert _same(part, full[sel]) and _same(part_mag, full_mag[sel]), rows
        for slot, row in enumerate(rows):
            assert torch.equal(part_state[slot * per:(slot + 1) * per], full_state[row * per:(row + 1) * per]), rows
    # a state filled with NaN (0xFF bytes) before a first_frame = 0 call changes nothing
    poisoned = torch.full((aec_stream_state_bytes(3, f, p),), 0xFF, dtype=torch.uint8, device=dev)
    got, got_mag, st = _online(mic, far, kw, state=poisoned)
    assert st is poisoned and _same(got, full) and _same(got_mag, full_mag) and torch.equal(poisoned, full_state)
    # the frames cut into calls of 1, of B = 4 and of irregular sizes, the state carried
    for cuts in ((1,) * n_frames, (4,) * 24 + (1,), (7, 1, 30, 23, 36)):
        parts, mags, state, at = [], [], None, 0
        for n in cuts:
            e, m, state = _online(mic[:, at:at + n], far[:, at:at + n], kw, state=state, first_frame=at)
            parts.append(e)
            mags.append(m)
            at += n
        assert at == n_frames
        assert _same(torch.cat(parts, dim=1), full) and _same(torch.cat(mags, dim=3), full_mag), cuts
        assert torch.equal(state, full_state), cuts


@pytest.mark.parametrize("kw", LAYOUTS, ids=LAYOUT_IDS)
def test_a_bin_gives_the_same_bits_whichever_bins_share_the_call(dev, kw):
    mic, far = _pair(dev, 512, 40)
    full, full_mag, _ = _online(mic, far, kw)
    # bins repacked contiguous and run alone: F = 33, 1, 17, 7, 9 are no multiple of the 32, 16 or 8 bins of a workgroup; 32 is
    for lo, hi in ((0, 33), (100, 133), (0, 1), (256, 257), (7, 24), (250, 257), (64, 96), (120, 129)):
        part, part_mag, _ = _online(mic[:, :, lo:hi], far[:, :, lo:hi], kw)
        assert _same(part, full[:, :, lo:hi]) and _same(part_mag, full_mag[:, :, lo:hi]), (lo, hi)


# ---- 3. the consequences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", LAYOUTS, ids=LAYOUT_IDS)
def test_zero_inputs_and_non_finite_values(dev, kw):
    mic, far = _pair(dev, 64, 40)
    got, mag, _ = _online(mic, torch.zeros_like(far), kw)
    assert _same(got, mic)                                                          # R = 0: Y's bits
    got, mag, _ = _online(torch.zeros_like(mic), far, kw)
    assert bool((_bits(got) == 0).all()) and bool((_bits(mag) == 0).all())          # Y = 0: zeros
    clean, clean_mag, _ = _online(mic, far, kw)
    assert not _same(clean, mic)
    for bad in (float("nan"), float("inf")):                                        # confined to its own (row, bin)
        for which in (0, 1):
            row, bin_, frame = 1, 30, 21
            inputs = [mic.clone(), far.clone()]
            inputs[which][row, frame, bin_] = complex(bad, 0.25)
            got, mag, _ = _online(inputs[0], inputs[1], kw)
            keep = torch.ones((3, 33), dtype=torch.bool, device=dev)
            keep[row, bin_] = False
            assert _same(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep]) and _same(mag[:, 0][keep], clean_mag[:, 0][keep])
            assert _same(got[row, :frame, bin_], clean[row, :frame, bin_])


def _filter_of(state, n_rows, f, k, d):
    """P and h of every (row, bin) of a state: the first 2 (K^2 + K) floats of a record of 2 K^2 + 4 K + 2 D."""
    return state.view(torch.float32).view(n_rows, f, 2 * k * k + 4 * k + 2 * d)[..., :2 * (k * k + k)]


@pytest.mark.parametrize("kw", (None, dict(taps=9, delay=2, forget=0.95), ec.PARITY_PARAMS[5]), ids=("defaults", "K9-D2", "K32-D8"))
def test_the_gate_leaves_p_and_h_as_they_are(dev, kw):
    k, d = (kw or er.DEFAULTS)["taps"], (kw or er.DEFAULTS).get("delay", 0)
    mic, far = _pair(dev, 64, 97)
    f, first = 33, 40
    silent = far.clone()
    silent[:, first:] = 0
    _, _, state = _online(mic[:, :first + k + d], silent[:, :first + k + d], kw)    # the stack is silent from frame first + K + D - 1 on
    held = _filter_of(state, 3, f, k, d).clone()
    e, _, state = _online(mic[:, first + k + d:], silent[:, first + k + d:], kw, state=state, first_frame=first + k + d)
    assert _same(_filter_of(state, 3, f, k, d), held)
    assert bool(torch.isfinite(torch.view_as_real(e)).all())
    whole, _, whole_state = _online(mic, silent, kw)
    assert _same(whole[:, first + k + d:], e) and torch.equal(whole_state, state)
    _, _, moved = _online(mic, far, kw)                                            # with a far end that goes on, the filter moves
    assert not _same(_filter_of(moved, 3, f, k, d), held)


def test_a_minute_with_a_silent_far_end(dev):
    """3750 frames at the defaults, the far end digital silence for frames 1000 ... 3000: finite, and max |e - e64| of the row within
    4 x the float32 restatement's own error on this input (the larger of its two arithmetics, measured here, no cap)."""
    mic_h, far_h = ec.long_spec()
    e64 = er.aec_online(mic_h.astype(np.complex128), far_h.astype(np.complex128))
    own = max(float(np.abs(er.aec_online(mic_h, far_h, dtype=np.float32, arithmetic=a).astype(np.complex128) - e64).max())
              for a in er.ARITHMETICS)
    got, mag, state = _online(_upload(dev, mic_h[None]), _upload(dev, far_h[None]))
    got_h = got.cpu().numpy()[0]
    assert np.isfinite(got_h).all() and bool(torch.isfinite(mag).all()) and bool(torch.isfinite(state.view(torch.float32)).all())
    err = float(np.abs(got_h.astype(np.complex128) - e64).max())
    print(f"long run: device {err:.3g}, the float32 restatement {own:.3g} ({err / own:.2f} of it; bound 4), max |e64| {np.abs(e64).max():.3g}")
    assert err <= 4.0 * own


# ---- 4. adn_aec_stream on a lockstep state -----------------------------------------------------------------------------------------
STREAM_N_FFT, STREAM_HOP, STREAM_BLOCK, STREAM_F = 64, 16, 4, 33


def _stream_audio(dev, n_frames=ec.E2E_FRAMES, n_fft=STREAM_N_FFT):
    """(6, L) on the device: microphone and far end of the three parity rows, interleaved as the streams of three pairs."""
    mic, far, _ = ec.parity_audio(n_fft, n_frames)
    return torch.from_numpy(np.stack([mic, far], axis=1).reshape(6, -1).astype(np.float32)).to(dev)


def _se(dev, **kw):
    from audiodenoiser_amd.echo import StreamEchoCanceller
    kw.setdefault("n_fft", STREAM_N_FFT)
    kw.setdefault("hop_length", kw["n_fft"] // 4)
    return StreamEchoCanceller(dev, **kw)


def _push_all(se, xd, sizes):
    outs, pos = [], 0
    for size in sizes:
        out = se.push(xd[:, pos:pos + size])
        outs.append(out[None] if out.dim() == 1 else out)
        pos += size
    assert pos >= xd.shape[1]
    out = se.flush()
    outs.append(out[None] if out.dim() == 1 else out)
    return torch.cat(outs, dim=1)


def _traced(dev, kw):
    """A StreamEchoCanceller over three pairs whose adn_aec_stream call is compared, call by call, with adn_aec_online on the rings'
    spectrograms, and whose writes are compared with a copy taken before the call.  The ring is the first section of the stream
    state: [stream][RX][F] float2, frame t at t mod RX, RX = max_steps * block (csrc/stream_kernels.hip)."""
    from audiodenoiser_amd.echo import StreamEchoCanceller, aec_online
    F = STREAM_F

    class Traced(StreamEchoCanceller):
        online_state, calls, changed = None, 0, False

        def ring(self):
            n, rx = self.n_streams, self.max_steps * self.block_frames
            return torch.view_as_complex(self._state.view(torch.float32)[:n * rx * F * 2].view(n, rx, F, 2))

        def _cancel(self, x, first_step, n_steps, final_length=-1):
            n, w, b = self.n_streams, self.window_frames, self.block_frames
            rx = self.max_steps * b
            end = (first_step + n_steps) * b
            if final_length >= 0:
                end = min(end, 1 + final_length // self.hop_length)
            frames = list(range(first_step * b, end))
            idx = [t % rx for t in frames]
            ring = self.ring()
            spec = ring[:, idx].clone()
            x_before, ring_before, rest_before = x.clone(), ring.clone(), self._state.clone()
            e, m, self.online_state = aec_online(spec[0::2].contiguous(), spec[1::2].contiguous(), state=self.online_state,
                                                 first_frame=frames[0], params=self.params)
            super()._cancel(x, first_step, n_steps, final_length)
            win = x.view(n, n_steps, F, w)
            assert _same(ring[0::2][:, idx], e), (first_step, n_steps)                   # bit for bit the online form ...
            kept = win[0::2][..., w - b:].permute(0, 2, 1, 3).reshape(n // 2, 1, F, n_steps * b)
            assert _same(kept[..., :len(frames)], m), (first_step, n_steps)
            assert torch.equal(self._aec_state, self.online_state)
            # ... and not one byte else: the far-end streams' windows and ring cells, the microphones' other columns and cells, the
            # columns of frames at and past the end of the finished stream, the rest of the stream state
            x_want, ring_want = x_before.clone(), ring_before.clone()
            want_kept = x_want.view(n, n_steps, F, w)[0::2][..., w - b:].permute(0, 2, 1, 3).reshape(n // 2, 1, F, n_steps * b).clone()
            want_kept[..., :len(frames)] = m
            x_want.view(n, n_steps, F, w)[0::2][..., w - b:] = want_kept.view(n // 2, F, n_steps, b).permute(0, 2, 1, 3)
            ring_want[0::2][:, idx] = e
            assert _same(x, x_want) and _same(ring, ring_want), (first_step, n_steps)
            assert _same(x.view(n, n_steps, F, w)[1::2], x_before.view(n, n_steps, F, w)[1::2]) and _same(ring[1::2], ring_before[1::2])
            tail = n * rx * F * 8
            assert torch.equal(self._state[tail:], rest_before[tail:])
            Traced.changed = Traced.changed or not _same(x, x_before)
            Traced.calls += 1
            return x

    se = Traced(dev, pairs=3, n_fft=STREAM_N_FFT, hop_length=STREAM_HOP, block_frames=STREAM_BLOCK, params=_params(kw))
    state, h_state = fp.carve(se._state.numel(), 0xFF, dev)
    astate, h_astate = fp.carve(se._aec_state.numel(), 0xFF, dev)
    se._state, se._aec_state = state, astate
    se.reset()
    assert fp.keeps_fill(h_astate, 0xFF)
    return se, Traced, (h_state, h_astate)


@pytest.mark.parametrize("kw", LAYOUTS, ids=LAYOUT_IDS)
def test_stream_is_online_bit_for_bit_and_writes_nothing_else(dev, kw):
    xd = _stream_audio(dev)[:, :98 * STREAM_HOP + 5]        # 99 frames, 24 whole blocks and one of three; long enough to hold far-end bursts
    se, traced, handles = _traced(dev, kw)
    with fp.carved_outputs(dev) as made:
        outs = [se.push(xd[:, :200]), se.push(xd[:, 200:]), se.flush()]
    torch.cuda.synchronize(dev)
    assert traced.calls >= 2 and traced.changed and made
    for h in made:
        fp.assert_guards_intact(h, "a buffer of the stream")
    for h, what in zip(handles, ("stream state", "echo state")):
        fp.assert_guards_intact(h, what)
    got = torch.cat(outs, dim=1)
    assert got.shape == (3, xd.shape[1]) and got.is_cuda and got.dtype == torch.float32 and bool(torch.isfinite(got).all())


_WHOLE = {}


def _whole(dev, n_fft, gain):
    """The three end-to-end pairs of (n_fft, gain) through one object, pushed whole: computed once."""
    if (n_fft, gain) not in _WHOLE:
        xd = _stream_audio(dev, ec.E2E_FRAMES, n_fft)
        _WHOLE[n_fft, gain] = (xd, _push_all(_se(dev, pairs=3, n_fft=n_fft, gain=gain), xd, [xd.shape[1]]))
    return _WHOLE[n_fft, gain]


@pytest.mark.parametrize("gain", (False, True))
@pytest.mark.parametrize("n_fft", ec.PARITY_N_FFT)
def test_stream_against_the_float64_end_to_end_form(dev, n_fft, gain):
    """Within 4 audio floors, a floor the float32 end-to-end restatement's max |a32 - a64| / max |a64| on the same pair, measured
    here as dereverb_stream_cases.measure_floor_audio measures it (never below 2^-23)."""
    xd, got = _whole(dev, n_fft, gain)
    assert got.shape == (3, xd.shape[1]) and got.is_cuda and got.dtype == torch.float32
    got_h = got.cpu().numpy().astype(np.float64)
    mic, far, _ = ec.parity_audio(n_fft, ec.E2E_FRAMES)
    for c in range(3):
        m32, f32 = mic[c].astype(np.float32), far[c].astype(np.float32)              # what the device was given
        want = er.echo_cancel(m32.astype(np.float64), f32.astype(np.float64), n_fft, n_fft // 4, gain=gain)
        a32 = er.echo_cancel(m32, f32, n_fft, n_fft // 4, gain=gain, dtype=np.float32)
        scale = float(np.abs(want).max())
        floor = max(float(np.abs(a32.astype(np.float64) - want).max()) / scale, sb.EPS)
        err = float(np.abs(got_h[c] - want).max())
        print(f"n_fft {n_fft} gain {gain} pair {c}: {err / scale:.3g} of the maximum, floor {floor:.3g} ({err / scale / floor:.2f} floors; bound 4)")
        assert err <= 4.0 * floor * scale, (c, err / scale, floor)


@pytest.mark.parametrize("gain", (False, True))
def test_any_cut_into_pushes_neighbours_and_reset_give_the_same_bits(dev, gain):
    from audiodenoiser_amd.baseline import spectral_gain_windows
    xd, whole = _whole(dev, 64, gain)
    length = xd.shape[1]
    for block in (1, 4):
        kw = dict(gain=gain, block_frames=block)
        three = _se(dev, pairs=3, **kw)
        assert three.lookahead_frames == 0 and three.window_frames == 16 and three.n_streams == 6
        ref = whole if block == 4 else _push_all(three, xd, [length])
        assert torch.equal(_push_all(three, xd, [100] * (-(-length // 100))), ref), block
        solo = _se(dev, **kw)
        for c in range(3):                                                          # pair c of 3 is a solo pair of its samples
            one = xd[2 * c:2 * c + 2].contiguous()
            alone = _push_all(solo, one, [length])
            assert torch.equal(alone, ref[c:c + 1]), (block, c)
            if c == 1:
                assert torch.equal(_push_all(solo, one, [1] * 300 + [length - 300]), alone), "pushes of one sample"
        three.push(xd[:, :length // 2])                                             # reset() in mid-stream, then the same audio
        three.reset()
        assert torch.equal(_push_all(three, xd, [length]), ref)
    # one pair returns (k,), several (pairs, k); numpy in, numpy out
    solo = _se(dev)
    out = solo.push(xd[:2].cpu().numpy())
    assert isinstance(out, np.ndarray) and out.ndim == 1
    solo.reset()
    if gain:                                                                        # the gain of a pair against the gain on its windows alone
        from audiodenoiser_amd.baseline import _gain_kept_columns
        from audiodenoiser_amd.echo import StreamEchoCanceller
        alone_state = torch.full((3, 3, STREAM_F), -1.0, device=dev)

        class Checked(StreamEchoCanceller):
            calls = 0

            def _net(self, x, first_step, n_steps, final_length=-1):
                self._cancel(x, first_step, n_steps, final_length)
                n, w, b = self.n_streams, self.window_frames, self.block_frames
                mics = x.view(n, n_steps, STREAM_F, w)[0::2].reshape(-1, 1, STREAM_F, w).contiguous()
                alone = spectral_gain_windows(mics, alone_state, w - b, b, n_steps, self.gain_params, None, mics.clone())
                _gain_kept_columns(x, None, n_steps, self._gain_state, self._plan, self.gain_params)
                both = x.view(n, n_steps, STREAM_F, w)[0::2].reshape(-1, 1, STREAM_F, w)
                assert _same(both[..., w - b:], alone[..., w - b:]) and _same(both[..., :w - b], mics[..., :w - b])
                Checked.calls += 1
                return x

        checked = Checked(dev, pairs=3, n_fft=STREAM_N_FFT, hop_length=STREAM_HOP, gain=True)
        assert torch.equal(_push_all(checked, xd, [700, length - 700]), whole) and Checked.calls >= 2
    with pytest.raises(RuntimeError):
        _se(dev).network(None)


def test_input_rate_48000_returns_as_many_samples_as_it_was_given(dev):
    length = 30011
    mic, far, _ = ec.quality_audio()
    x = torch.from_numpy(np.stack([mic[:length], far[:length]]).astype(np.float32)).to(dev)
    se = _se(dev, n_fft=512, input_rate=48000)
    assert se.input_rate == 48000 and se.sample_rate == 8000
    got = _push_all(se, x, [4800, 7, 12000, 13204])
    assert got.shape == (1, length) and bool(torch.isfinite(got).all())
    assert torch.equal(_push_all(se, x, [length]), got)


# ---- 5. footprint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_frames,kw", ((512, 40, None), (64, 5, ec.PARITY_PARAMS[3]), (64, 40, ec.PARITY_PARAMS[5])),
                         ids=("G8-F257", "G16-F33", "G32-F33"))
def test_online_writes_only_what_the_call_owns(dev, n_fft, n_frames, kw):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.echo import aec_stream_state_bytes
    n, f = 2, n_fft // 2 + 1
    mic, far = (s[:n].contiguous() for s in _pair(dev, n_fft, n_frames))
    p = _params(kw)
    ps = ctypes.byref(p.to_struct()) if p is not None else None
    plain, plain_mag, plain_state = _online(mic, far, kw)
    need = aec_stream_state_bytes(n, f, p)
    width, col0 = n_frames + 7, 3
    out, h_out = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    mag, h_mag = fp.carve_tensor((n, 1, f, width), 0xFF, dev)
    state, h_state = fp.carve(need, 0xFF, dev)
    src_m, h_m = fp.carve_copy(torch.view_as_real(mic), dev)
    src_f, h_f = fp.carve_copy(torch.view_as_real(far), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = _lib.load_echo()
    assert L.adn_aec_online(src_m.data_ptr(), src_f.data_ptr(), n, n_frames, f, 0, ps, state.data_ptr(), need, n, out.data_ptr(),
                            mag.data_ptr(), width, col0, stream) == 0
    torch.cuda.synchronize(dev)
    for h, what in ((h_out, "spec_out"), (h_mag, "mag_out"), (h_state, "state"), (h_m, "mic_spec"), (h_f, "far_spec")):
        fp.assert_guards_intact(h, what)
    assert _same(src_m, torch.view_as_real(mic)) and _same(src_f, torch.view_as_real(far))
    assert _same(torch.view_as_complex(out), plain) and _same(mag[..., col0:col0 + n_frames], plain_mag) and torch.equal(state, plain_state)
    assert bool((mag.view(torch.int32)[..., :col0] == -1).all()) and bool((mag.view(torch.int32)[..., col0 + n_frames:] == -1).all())
    # mag_out = NULL: spec_out and the state are written, the same bits; a refused call writes nothing
    out2, h_out2 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    state2, h_state2 = fp.carve(need, 0xFF, dev)
    assert L.adn_aec_online(src_m.data_ptr(), src_f.data_ptr(), n, n_frames, f, 0, ps, state2.data_ptr(), need, n, out2.data_ptr(), None,
                            0, 0, stream) == 0
    torch.cuda.synchronize(dev)
    fp.assert_guards_intact(h_out2, "spec_out")
    fp.assert_guards_intact(h_state2, "state")
    assert _same(out2, out) and torch.equal(state2, state)
    out3, h_out3 = fp.carve_tensor((n, n_frames, f, 2), 0xFF, dev)
    state3, h_state3 = fp.carve(need, 0xFF, dev)
    m, r = src_m.data_ptr(), src_f.data_ptr()
    for args in ((m, r, n, n_frames, f, -1, ps, state3.data_ptr(), need, n, out3.data_ptr(), None, 0, 0),
                 (m, r, n, n_frames, f, 0, ps, state3.data_ptr(), need - 1, n, out3.data_ptr(), None, 0, 0),
                 (m, r, n, n_frames, f, 0, ps, state3.data_ptr(), need, 1, out3.data_ptr(), None, 0, 0),
                 (m, r, n, n_frames, f, 0, ps, state3.data_ptr(), need, n, r, None, 0, 0)):
        assert L.adn_aec_online(*args, stream) in (1, 3) and L.adn_aec_last_error().startswith(b"adn_aec_online:"), args
    torch.cuda.synchronize(dev)
    assert fp.keeps_fill(h_out3, 0xFF) and fp.keeps_fill(h_state3, 0xFF)


# ---- 6. quality and the command line -----------------------------------------------------------------------------------------------
def test_quality_on_the_device(dev):
    """EchoCanceller.cancel on the quality recipe against the float64 chain on the same samples: ERLE and SI-SDR, both read off the
    first 372 frames of the result's own STFT, agree to 0.01 dB; and they are the restatement's (asserted at 10 dB on the host)."""
    from audiodenoiser_amd.echo import EchoCanceller
    mic, far, _ = (a.astype(np.float32) for a in ec.quality_audio())
    got = EchoCanceller(dev).cancel(mic, far)
    assert isinstance(got, np.ndarray) and got.shape == mic.shape and got.dtype == np.float32
    want = er.echo_cancel(mic.astype(np.float64), far.astype(np.float64))
    (erle, _, sdr), (erle64, sdr_in, sdr64) = ec.quality_of_audio(got), ec.quality_of_audio(want)
    print(f"device: ERLE {erle:.2f} dB, SI-SDR {sdr_in:.2f} -> {sdr:.2f} dB; float64 chain: ERLE {erle64:.2f} dB, SI-SDR -> {sdr64:.2f} dB")
    assert abs(erle - erle64) <= 0.01 and abs(sdr - sdr64) <= 0.01
    assert erle >= 10.0 and sdr >= sdr_in + 10.0
    # any rate, (N, L), tensors: as many samples as given
    x = torch.from_numpy(np.stack([mic[:30011], far[:30011]])).to(dev)
    out = EchoCanceller(dev, gain=True).cancel(x, x.flip(0), sr=44100)
    assert out.shape == x.shape and out.is_cuda and bool(torch.isfinite(out).all())


def test_command_line_offline_and_live(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.wav import read_wav, write_wav
    mic, far, near = (a[:24000].astype(np.float32) for a in ec.quality_audio())
    paths = [str(tmp_path / n) for n in ("mic.wav", "far.wav", "near.wav", "out.wav", "live.wav")]
    for path, a in zip(paths, (mic, far, near)):
        write_wav(path, a, 8000, "PCM_16")
    for extra, dst in (([], paths[3]), (["--live", "--chunk", "1000", "--gain"], paths[4])):
        run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.echo", paths[0], paths[1], dst, "--reference", paths[2], *extra],
                             cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        out, rate = read_wav(dst)
        assert rate == 8000 and out.shape[0] == 24000
        row = json.loads(run.stdout.strip().splitlines()[-1])
        print(f"{'live' if extra else 'offline'}: SI-SDR against the near end {row['noisy']['si_sdr']:.2f} -> {row['denoised']['si_sdr']:.2f} dB")
        assert row["denoised"]["si_sdr"] > row["noisy"]["si_sdr"]
        if extra:
            assert "latency 896 samples" in run.stdout
    bad = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.echo", paths[0], paths[1], paths[3], "--taps", "32", "--forget", "0.95"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "forget" in bad.stderr
