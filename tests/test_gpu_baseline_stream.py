"""Streaming spectral baseline on the device: adn_spectral_gain_windows (csrc/baseline_kernels.hip, the magnitude form of
include/adn.h, "baseline") and the classes built on it (audiodenoiser_amd/baseline.py: StreamSpectralDenoiser, SpectralStreamPool).

Bounds (derived, not tuned):
* the kernel against adn_spectral_gain on the same magnitudes rearranged to frame-major (m, 0), the carry over calls and steps, the
  row table, the classes against each other and against the pieces composed by hand: exact equality, as include/adn.h pins them.
* end to end against float64, in links as tests/test_gpu_baseline.py::test_end_to_end: the restatement is fed the device's own
  magnitudes (the kept columns of analyze) and the device's own phase (stft_complex), and the whole is bounded by the tree's
  inverse-STFT tolerance 1e-4 of max |want| plus the parity bound carried through, 8 x 4 FLOOR_WINDOWS max M64 (the factor 8:
  test_gpu_baseline.py's docstring; FLOOR_WINDOWS: the float32 host floor of the magnitude form, tests/baseline_stream_cases.py).
* quality: a cap, not parity -- the stream's SI-SDR gain on the 8 dB white mix is at least half the float64 restatement's.
Measured on the MI355X: end to end 3.3e-9 / 8.6e-9 / 5.4e-8 absolute at L 100 / 2047 / 24000 (bounds 5.2e-6 / 1.1e-5 / 1.2e-4); SI-SDR
of the stream 7.98 -> 13.70 dB, the restatement's gain of 5.72 dB to the printed digits; the 52 cases take 5 s.
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
import baseline_stream_cases as sc  # noqa: E402
import denoise_ref  # noqa: E402
import footprint as fp  # noqa: E402
import stream_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
FILL = 7.0                                      # what the columns outside a call hold in these tests: any finite value


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _windows(m, w, col0, n_cols, n_steps, fill=FILL):
    """(n_rows, n_steps * n_cols, F) magnitudes -> (n_rows * n_steps, 1, F, W): frame s n_cols + j at column col0 + j of step s."""
    n_rows, t, f = m.shape
    assert t == n_steps * n_cols
    win = torch.full((n_rows, n_steps, f, w), fill, dtype=torch.float32, device=m.device)
    win[..., col0:col0 + n_cols] = m.view(n_rows, n_steps, n_cols, f).permute(0, 1, 3, 2)
    return win.view(n_rows * n_steps, 1, f, w).contiguous()


def _frames(y, n_rows, col0, n_cols):
    """The inverse on the kept columns: (n_rows * n_steps, 1, F, W) -> (n_rows, 1, F, n_steps * n_cols), spectral_gain's layout."""
    nw, _, f, w = y.shape
    n_steps = nw // n_rows
    return y.view(n_rows, n_steps, f, w)[..., col0:col0 + n_cols].permute(0, 2, 1, 3).reshape(n_rows, 1, f, n_steps * n_cols)


def _fresh(n, f, dev):
    return torch.full((n, 3, f), -1.0, dtype=torch.float32, device=dev)


def _mags(dev, n_rows, t, f, seed):
    return torch.from_numpy(sc.magnitudes(n_rows, t, f, seed)).to(dev)


def _offline(m):
    """adn_spectral_gain on (m, 0): -> ((n_rows, 1, F, T), state (n_rows, 3, F))."""
    from audiodenoiser_amd.baseline import spectral_gain
    return spectral_gain(torch.complex(m, torch.zeros_like(m)))


# ---- 1. bit equality with the frame-major kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,col0,n_cols,n_steps", sc.KERNEL_PLANS)
@pytest.mark.parametrize("n_rows", sc.KERNEL_ROWS)
@pytest.mark.parametrize("f", sc.KERNEL_BINS)
def test_equals_spectral_gain_on_rearranged_input(dev, f, n_rows, w, col0, n_cols, n_steps):
    from audiodenoiser_amd.baseline import spectral_gain_windows
    m = _mags(dev, n_rows, n_steps * n_cols, f, 1)
    want, want_state = _offline(m)
    win = _windows(m, w, col0, n_cols, n_steps)
    state = _fresh(n_rows, f, dev)
    y = spectral_gain_windows(win, state, col0, n_cols, n_steps)
    assert y.shape == win.shape and y.dtype == torch.float32
    assert torch.equal(_frames(y, n_rows, col0, n_cols), want)
    assert torch.equal(state, want_state)
    assert bool(torch.isfinite(want).all()) and float(want.max()) > 0


# ---- 2. carry and rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,w,col0,n_cols,n_steps", ((257, 20, 7, 5, 7), (33, 16, 12, 4, 11), (513, 16, 15, 1, 40)))
def test_one_call_of_n_steps_equals_the_steps_one_call_each(dev, f, w, col0, n_cols, n_steps):
    from audiodenoiser_amd.baseline import spectral_gain_windows
    n_rows = 3
    win = _windows(_mags(dev, n_rows, n_steps * n_cols, f, 2), w, col0, n_cols, n_steps)
    state = _fresh(n_rows, f, dev)
    whole = spectral_gain_windows(win, state, col0, n_cols, n_steps)
    by_step = win.view(n_rows, n_steps, 1, f, w)
    st = _fresh(n_rows, f, dev)
    parts = [spectral_gain_windows(by_step[:, s].contiguous(), st, col0, n_cols, 1) for s in range(n_steps)]
    got = torch.stack(parts, dim=1).view(n_rows * n_steps, 1, f, w)
    assert torch.equal(got[..., col0:col0 + n_cols], whole[..., col0:col0 + n_cols]) and torch.equal(st, state)
    # and cut into calls of 3 steps, 1 step and the rest
    st = _fresh(n_rows, f, dev)
    parts, lo = [], 0
    for hi in (3, 4, n_steps):
        parts.append(spectral_gain_windows(by_step[:, lo:hi].contiguous().view(-1, 1, f, w), st, col0, n_cols, hi - lo)
                     .view(n_rows, hi - lo, 1, f, w))
        lo = hi
    got = torch.cat(parts, dim=1).view(n_rows * n_steps, 1, f, w)
    assert torch.equal(got[..., col0:col0 + n_cols], whole[..., col0:col0 + n_cols]) and torch.equal(st, state)


def test_row_table_permuted_slots_mixed_fresh_and_untouched_slots(dev):
    from audiodenoiser_amd.baseline import spectral_gain_windows
    f, w, col0, n_cols, n_steps, n_rows, n_slots = 257, 20, 7, 5, 4, 3, 6
    win = _windows(_mags(dev, n_rows, n_steps * n_cols, f, 3), w, col0, n_cols, n_steps)
    pre = _windows(_mags(dev, 2, 3 * n_cols, f, 4), w, col0, n_cols, 3)
    carried = _fresh(2, f, dev)
    spectral_gain_windows(pre, carried, col0, n_cols, 3)                  # row 1 continues from carried[0]; carried[1] is in the way
    # each row alone, on a state of one slot
    alone, alone_state = [], []
    for i, start in enumerate((_fresh(1, f, dev), carried[:1].clone(), _fresh(1, f, dev))):
        one = win.view(n_rows, n_steps, 1, f, w)[i].contiguous()
        alone.append(spectral_gain_windows(one, start, col0, n_cols, n_steps))
        alone_state.append(start)
    # together: row 0 -> slot 4 (forced fresh over NaN bits), row 1 -> slot 0 (continues), row 2 -> slot 2 (forced fresh over a
    # live state of another stream); slots 1, 3, 5 are named by no row
    state, h = fp.carve_tensor((n_slots, 3, f), 0xFF, dev)
    state[0] = carried[0]
    state[2] = carried[1]
    y, h_y = fp.carve_tensor(tuple(win.shape), 0xFF, dev)
    spectral_gain_windows(win, state, col0, n_cols, n_steps, rows=[(4, True), (0, False), (2, True)], out=y)
    torch.cuda.synchronize(dev)
    fp.assert_guards_intact(h, "state")
    fp.assert_guards_intact(h_y, "y")
    got = y.view(n_rows, n_steps, 1, f, w)
    for i, slot in enumerate((4, 0, 2)):
        assert torch.equal(got[i][..., col0:col0 + n_cols], alone[i][..., col0:col0 + n_cols]), i
        assert torch.equal(state[slot], alone_state[i][0]), i
    assert bool((state.view(torch.int32)[[1, 3, 5]] == -1).all()), "slots no row names keep their bytes"
    # rows=None on the same data: slot i, and a negative P starts fresh as before
    st = _fresh(n_rows, f, dev)
    st[1] = carried[0]
    plain = spectral_gain_windows(win, st, col0, n_cols, n_steps)
    assert torch.equal(plain[..., col0:col0 + n_cols], y[..., col0:col0 + n_cols])


# ---- 3. footprint ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,w,col0,n_cols,n_steps", ((257, 16, 12, 4, 1), (33, 20, 7, 5, 7), (513, 16, 0, 16, 3)))
def test_footprint_only_the_kept_columns(dev, f, w, col0, n_cols, n_steps):
    from audiodenoiser_amd.baseline import spectral_gain_windows
    n_rows = 2
    win = _windows(_mags(dev, n_rows, n_steps * n_cols, f, 5), w, col0, n_cols, n_steps)
    before = win.clone()
    y, h_y = fp.carve_tensor(tuple(win.shape), 0xFF, dev)
    state, h_s = fp.carve_tensor((n_rows, 3, f), 0xFF, dev)
    state.fill_(-1.0)
    spectral_gain_windows(win, state, col0, n_cols, n_steps, out=y)
    torch.cuda.synchronize(dev)
    fp.assert_guards_intact(h_y, "y")
    fp.assert_guards_intact(h_s, "state")
    assert torch.equal(win, before), "windows is read only when y is separate"
    bits = y.view(torch.int32)
    assert bool((bits[..., :col0] == -1).all()) and bool((bits[..., col0 + n_cols:] == -1).all())
    assert bool(torch.isfinite(y[..., col0:col0 + n_cols]).all())
    # in place: the same kept columns, the rest as it was
    inplace, h_w = fp.carve_copy(win, dev)
    st2 = _fresh(n_rows, f, dev)
    assert spectral_gain_windows(inplace, st2, col0, n_cols, n_steps, out=inplace) is inplace
    torch.cuda.synchronize(dev)
    fp.assert_guards_intact(h_w, "windows in place")
    assert torch.equal(inplace[..., col0:col0 + n_cols], y[..., col0:col0 + n_cols]) and torch.equal(st2, state)
    assert torch.equal(inplace[..., :col0], before[..., :col0]) and torch.equal(inplace[..., col0 + n_cols:], before[..., col0 + n_cols:])


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_a_non_finite_magnitude_poisons_its_own_row_and_bin_only(dev, bad):
    from audiodenoiser_amd.baseline import spectral_gain_windows
    f, w, col0, n_cols, n_steps, n_rows = 257, 20, 7, 5, 14, 3                     # 70 frames: the bad one sits in the second tile
    m = _mags(dev, n_rows, n_steps * n_cols, f, 6)
    clean_state = _fresh(n_rows, f, dev)
    clean = _frames(spectral_gain_windows(_windows(m, w, col0, n_cols, n_steps), clean_state, col0, n_cols, n_steps), n_rows, col0, n_cols)
    row, bin_, frame = 1, 130, 37
    m[row, frame, bin_] = bad
    state = _fresh(n_rows, f, dev)
    got = _frames(spectral_gain_windows(_windows(m, w, col0, n_cols, n_steps), state, col0, n_cols, n_steps), n_rows, col0, n_cols)
    keep = torch.ones((n_rows, f), dtype=torch.bool, device=dev)
    keep[row, bin_] = False
    assert torch.equal(got[:, 0][keep], clean[:, 0][keep])
    assert torch.equal(state.transpose(1, 2)[keep], clean_state.transpose(1, 2)[keep])
    assert torch.equal(got[row, 0, bin_, :frame], clean[row, 0, bin_, :frame])
    assert bool(torch.isnan(got[row, 0, bin_, frame:]).all()) and not bool(torch.isfinite(state[row, :, bin_]).any())


# ---- 5. StreamSpectralDenoiser --------------------------------------------------------------------------------------------------------
def _sd(dev, **kw):
    from audiodenoiser_amd.baseline import StreamSpectralDenoiser
    return StreamSpectralDenoiser(dev, **kw)


def _push_all(sd, xd, sizes):
    outs, pos = [], 0
    for size in sizes:
        outs.append(sd.push(xd[:, pos:pos + size]))
        pos += size
    assert pos >= xd.shape[1]
    outs.append(sd.flush())
    return torch.cat(outs, dim=1)


def _by_hand(sd, xd, gain):
    """Every step of a finished stream through analyze / emit themselves with `gain(windows, first_step, n_steps)` in between, in
    calls of up to max_steps steps: the running steps, then the rest with the final length.  -> windows as analysed
    (n_streams, K, F, W), audio (n_streams, L)."""
    n_fft, hop, w, b = sd.n_fft, sd.hop_length, sd.window_frames, sd.block_frames
    n, length = xd.shape
    running = stream_ref.steps_done(length, n_fft, hop, b, 0)
    total = stream_ref.n_steps(1 + length // hop, b)
    sd.reset()
    wins, outs, k = [], [], 0
    while k < total:
        final = -1 if k < running else length
        m = min(sd.max_steps, (running if k < running else total) - k)
        base = 0 if k == 0 else (k * b - 1) * hop + n_fft // 2            # e(k - 1): where the call's new samples start
        src = xd[:, base:] if base < length else xd
        win = sd.analyze(src, length, k, m, final)
        wins.append(win.view(n, m, sd.n_bins, w).clone())
        outs.append(sd.emit(gain(win, k, m), k, m, final))
        k += m
    sd.reset()
    return torch.cat(wins, dim=1), torch.cat(outs, dim=1)


_E2E = {}


def _e2e(dev, length):
    """One end-to-end case, computed once: the input, the pushed stream's output, the analysed windows and the by-hand output."""
    if length not in _E2E:
        from audiodenoiser_amd.baseline import spectral_gain_windows
        x = sc.e2e_audio(length)
        xd = torch.from_numpy(x.copy()).to(dev)[None]
        sd = _sd(dev)
        got = _push_all(sd, xd, [length])
        state = _fresh(1, sd.n_bins, dev)
        w, b = sd.window_frames, sd.block_frames
        wins, hand = _by_hand(sd, xd, lambda win, k, m: spectral_gain_windows(win, state, w - b, b, m, out=win))
        _E2E[length] = (x, xd, got, wins, hand)
    return _E2E[length]


@pytest.mark.parametrize("length", sc.LENGTHS)
def test_stream_returns_its_input_length_whatever_the_pushes(dev, length):
    x, xd, whole, _, hand = _e2e(dev, length)
    sd = _sd(dev)
    assert sd.latency_samples == 896 and sd.window_frames == 16 and sd.lookahead_frames == 0 and sd.input_rate == 8000
    assert whole.shape == (1, length) and whole.is_cuda and bool(torch.isfinite(whole).all())
    by_1000 = _push_all(sd, xd, [1000] * (-(-length // 1000)))
    rng = np.random.default_rng([length, 77])
    sizes = []
    while sum(sizes) < length:
        sizes.append(int(rng.integers(1, 8)) if len(sizes) % 3 == 1 else int(rng.integers(1, 3001)))
    rand = _push_all(sd, xd, sizes)
    assert torch.equal(whole, by_1000) and torch.equal(whole, rand)
    assert torch.equal(whole, hand), "analyze -> spectral_gain_windows -> emit composed by hand"
    assert sd.received == 0 and sd.emitted == 0
    # numpy in -> numpy out, (L,) in
    out = np.concatenate([sd.push(x), sd.flush()], axis=1)
    assert isinstance(out, np.ndarray) and np.array_equal(out, whole.cpu().numpy())


def test_three_streams_equal_three_solo_objects(dev):
    length = 5000
    x = np.stack([bc.white_mix(length, snr, 70 + c)[0] for c, snr in enumerate((8.0, 0.0, 15.0))])
    xd = torch.from_numpy(x).to(dev)
    three = _push_all(_sd(dev, n_streams=3), xd, [1700, 1, 2500, 799])
    for c in range(3):
        solo = _push_all(_sd(dev), xd[c:c + 1].contiguous(), [length])
        assert torch.equal(three[c:c + 1], solo), c
    # reset() forgets the noise estimate: a second run of the same object gives the same bits
    sd = _sd(dev, n_streams=3)
    first = _push_all(sd, xd, [length])
    sd.push(xd[:, :3000])
    sd.reset()
    assert torch.equal(_push_all(sd, xd, [length]), first) and torch.equal(first, three)


def test_input_rate_48000_equals_resample_stream_resample(dev):
    from audiodenoiser_amd.resample import _resample_device
    length = 30011
    x = torch.from_numpy(bc.white_mix(length, 8.0, 81)[0]).to(dev)[None]
    sd = _sd(dev, input_rate=48000)
    assert sd.input_rate == 48000 and sd.sample_rate == 8000
    got = _push_all(sd, x, [4800, 7, 12000, 13204])
    assert got.shape == (1, length)
    at_work = _resample_device(x, 48000, 8000)
    back = _resample_device(_push_all(_sd(dev), at_work, [at_work.shape[1]]), 8000, 48000)
    assert back.shape[1] >= length and torch.equal(got, back[:, :length])


# ---- 6. SpectralStreamPool --------------------------------------------------------------------------------------------------------------
def test_pool_streams_equal_solo_streams(dev):
    """Staggered opens, uneven pushes (numpy and device tensors), a slot reused without a reset, one stream at 48 kHz."""
    from audiodenoiser_amd.baseline import SpectralStreamPool
    pool = SpectralStreamPool(dev, max_streams=3, backlog_steps=16, input_rates=(48000,))
    assert pool.latency_samples == 896
    lengths, rates = (6000, 3100, 20000, 4000), (None, None, 48000, None)
    sig = [bc.white_mix(n, 8.0, 90 + i)[0] for i, n in enumerate(lengths)]
    want = [_push_all(_sd(dev, input_rate=rates[i]), torch.from_numpy(s.copy()).to(dev)[None], [len(s)])[0].cpu()
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
    pool.close(sid[0])
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


def test_pool_of_more_than_one_group_of_rows(dev):
    """300 streams: two kernel calls a tick (256 + 44 rows); the first, the 256th, the 257th and the last equal a solo stream."""
    from audiodenoiser_amd.baseline import SpectralStreamPool
    n, length = 300, 700
    pool = SpectralStreamPool(dev, max_streams=n, backlog_steps=12, n_fft=64, hop_length=16, block_frames=4)
    base = bc.white_mix(length + n, 8.0, 95)[0]
    sids = [pool.open() for _ in range(n)]
    for i, s in enumerate(sids):
        pool.push(s, base[i:i + length])
        pool.close(s)
    outs = {s: samples for s, samples, finished in pool.drain() if finished}
    assert len(outs) == n
    for i in (0, 255, 256, 299):
        x = torch.from_numpy(base[i:i + length].copy()).to(dev)[None]
        solo = _push_all(_sd(dev, n_fft=64, hop_length=16, block_frames=4), x, [length])[0]
        assert np.array_equal(outs[sids[i]], solo.cpu().numpy()), i


# ---- 7. end to end against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", sc.LENGTHS)
def test_end_to_end_against_float64(dev, length):
    from audiodenoiser_amd.griffin_lim import stft_complex
    x, xd, got, wins, _ = _e2e(dev, length)
    n_frames, b, w = 1 + length // sc.HOP, 4, 16
    k = stream_ref.n_steps(n_frames, b)
    assert wins.shape == (1, k, sc.F, w)
    # the device's own magnitudes: the kept columns of analyze, frame k B + i from column W - B + i of window k
    m = wins[0][..., w - b:].permute(0, 2, 1).reshape(k * b, sc.F)[:n_frames].cpu().numpy()
    assert m.dtype == np.float32 and bool((m >= 0).all())
    spec = stft_complex(xd, sc.N_FFT, sc.HOP)[0].cpu().numpy().astype(np.complex128)
    assert spec.shape == m.shape
    m64, _ = br.spectral_gain(m.astype(np.complex128))
    want = denoise_ref.istft(denoise_ref.rephase(m64, spec), sc.HOP, length)
    err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    bound = TOL * float(np.abs(want).max()) + 8 * 4 * sc.FLOOR_WINDOWS * float(m64.max())
    print(f"end to end L {length}: {err:.3g} (bound {bound:.3g}; max |want| {np.abs(want).max():.3g}, max M64 {m64.max():.3g})")
    assert err <= bound


# ---- 8. quality -------------------------------------------------------------------------------------------------------------------------
def test_si_sdr_gain_of_the_stream_on_the_8_db_white_mix(dev):
    from audiodenoiser_amd.metrics import evaluate
    noisy, clean = bc.quality_case(8.0)
    want_gain = br.si_sdr(br.denoise(noisy.astype(np.float64), 512, 128), clean) - br.si_sdr(noisy, clean)
    nd, cd = torch.from_numpy(noisy).to(dev), torch.from_numpy(clean).to(dev)
    out = _push_all(_sd(dev), nd[None], [1024] * 47)[0]
    before, after = float(evaluate(nd, cd, sr=8000)["si_sdr"][0]), float(evaluate(out, cd, sr=8000)["si_sdr"][0])
    print(f"SI-SDR of the stream: {before:.2f} -> {after:.2f} dB (gain {after - before:.2f}; the restatement's {want_gain:.2f})")
    assert want_gain >= 3.0 and after - before >= 0.5 * want_gain


# ---- 9. refusals, command line ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_carved_buffers_untouched(dev):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import SpectralParams, spectral_gain_windows
    L = _lib.load()
    f, w, n_rows, n_steps = 33, 16, 2, 3
    win, h_w = fp.carve_tensor((n_rows * n_steps, 1, f, w), 0xFF, dev)
    y, h_y = fp.carve_tensor((n_rows * n_steps, 1, f, w), 0xFF, dev)
    st, h_s = fp.carve_tensor((4, 3, f), 0xFF, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(windows=win.data_ptr(), out=y.data_ptr(), n=n_rows, steps=n_steps, bins=f, width=w, col0=12, n_cols=4, params=None,
             state=st.data_ptr(), n_slots=4, rows=None):
        return L.adn_spectral_gain_windows(windows, out, n, steps, bins, width, col0, n_cols, params, state, n_slots, rows, stream)

    def table(*pairs):
        return (_lib.SpectralRow * len(pairs))(*[_lib.SpectralRow(*p) for p in pairs])

    bad = SpectralParams().to_struct()
    bad.gamma = 1.0
    for kw in (dict(windows=None), dict(out=None), dict(state=None), dict(windows=win.data_ptr() + 2), dict(n=0), dict(steps=0),
               dict(bins=0), dict(n_cols=0), dict(col0=-1), dict(col0=13), dict(n=5), dict(rows=table((0, 0), (4, 1))),
               dict(rows=table((1, 0), (1, 0))), dict(params=ctypes.byref(bad))):
        assert call(**kw) == 1 and L.adn_last_error().startswith(b"adn_spectral_gain_windows:"), kw
    torch.cuda.synchronize(dev)
    for h, what in ((h_w, "windows"), (h_y, "y"), (h_s, "state")):
        assert fp.keeps_fill(h, 0xFF), what
        fp.assert_guards_intact(h, what)
    with pytest.raises(ValueError):
        spectral_gain_windows(win, st, 13, 4, n_steps)
    with pytest.raises(ValueError):
        spectral_gain_windows(win, st, 12, 4, 4)                          # 6 windows are no multiple of 4 steps
    with pytest.raises(ValueError):
        spectral_gain_windows(win, st, 12, 4, n_steps, rows=[(0, True)])  # one (slot, fresh) per row


def test_command_line_live(dev, tmp_path):
    import json
    import subprocess
    from audiodenoiser_amd.wav import read_wav, write_wav
    noisy, clean = bc.quality_case(8.0, seconds=2.0)
    src, ref, dst = (str(tmp_path / n) for n in ("noisy.wav", "clean.wav", "out.wav"))
    write_wav(src, noisy, 8000, "PCM_16")
    write_wav(ref, clean, 8000, "PCM_16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-m", "audiodenoiser_amd.baseline", src, dst, "--live", "--reference", ref], cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out, rate = read_wav(dst)
    assert rate == 8000 and out.shape[0] == 16000
    assert "latency 896 samples" in run.stdout
    row = json.loads(run.stdout.strip().splitlines()[-1])
    assert row["denoised"]["si_sdr"] > row["noisy"]["si_sdr"] + 1.0
