"""The cases of the quality-metric tests, built once and shared: tests/test_gpu_quality.py runs them on the device,
tests/test_quality_host.py through the restatement, and ``python tests/quality_cases.py`` measures the float32 floor that
tests/quality_ref.py::FLOOR records (worst |float32 restatement - float64 restatement| per metric).  A plain helper module.

Inputs are float32 arrays (what the device receives); seeds are fixed.
"""
import os

import numpy as np

import quality_ref as qr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIME_LENGTHS = (1, 255, 8191, 8192, 8193, 20000)          # the block edges of the partial sums (8192 samples)
SEG_FRAMES = (16, 240, 8192)


def _rng(seed):
    return np.random.default_rng(seed)


def _signal(rng, n, length):
    """Tonal + noise, rows at different levels: nothing special about any block of the sums."""
    t = np.arange(length) / 8000.0
    rows = []
    for i in range(n):
        f = 180.0 + 37.0 * i
        rows.append((0.3 / (1 + i % 5)) * (np.sin(2 * np.pi * f * t) + 0.5 * np.sin(2 * np.pi * 3.1 * f * t + i))
                    + 0.05 * rng.standard_normal(length))
    return np.stack(rows).astype(np.float32)


def _noisy(rng, ref, snr_db):
    out = np.empty_like(ref)
    for i in range(ref.shape[0]):
        nz = rng.standard_normal(ref.shape[1])
        s = np.sqrt(np.mean(ref[i].astype(np.float64) ** 2) / max(np.mean(nz ** 2), 1e-30)) * 10 ** (-snr_db[i % len(snr_db)] / 20)
        out[i] = (ref[i] + s * nz).astype(np.float32)
    return out


def time_cases():
    """[(name, est (n, L), ref (n, L), lengths or None)]; every case runs at every seg_frame of SEG_FRAMES."""
    cases = []
    snrs = (-7.0, 3.0, 18.0, 41.0)
    for n in (1, 3):
        for length in TIME_LENGTHS:
            rng = _rng(1000 * n + length)
            ref = _signal(rng, n, length)
            cases.append((f"n{n}_L{length}", _noisy(rng, ref, snrs), ref, None))
    rng = _rng(65)
    ref = _signal(rng, 65, 8193)
    cases.append(("n65_L8193", _noisy(rng, ref, snrs), ref, None))
    # every row its own length, one row of length 0, the block edges among them
    rng = _rng(7)
    ref = _signal(rng, 8, 20000)
    lengths = np.array([20000, 0, 1, 255, 8191, 8192, 8193, 16385], dtype=np.int64)
    cases.append(("lengths", _noisy(rng, ref, snrs), ref, lengths))
    return cases


def high_sdr_case():
    """est = 0.5 ref + 1e-4 noise: about 74 dB of SI-SDR, which the expanded form of the residual cannot resolve in float32."""
    rng = _rng(74)
    ref = _signal(rng, 2, 20000)
    est = (0.5 * ref.astype(np.float64) + 1e-4 * np.sqrt(np.mean(ref.astype(np.float64) ** 2, axis=1, keepdims=True))
           * rng.standard_normal(ref.shape)).astype(np.float32)
    return est, ref


# ---- STOI: audio at 10 kHz ---------------------------------------------------------------------------------------------------------
def _speechlike(rng, length):
    """Noise under a slow envelope that stays within a few dB: every frame far above the 40 dB threshold."""
    t = np.arange(length) / 10000.0
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + 0.7)
    x = rng.standard_normal(length)
    x = np.convolve(x, np.array([0.25, 0.5, 0.25]), mode="same") + 0.3 * np.sin(2 * np.pi * 440.0 * t)
    return 0.3 * env * x


def _with_levels(x, sections):
    """x scaled section by section: sections = [(start, stop, dB)]."""
    g = np.ones(len(x))
    for a, b, db in sections:
        g[a:b] = 10 ** (db / 20.0)
    return x * g


def _pair(rng, ref, snr_db):
    nz = rng.standard_normal(len(ref))
    s = np.sqrt(np.mean(ref ** 2) / np.mean(nz ** 2)) * 10 ** (-snr_db / 20)
    return (ref + s * nz).astype(np.float32), ref.astype(np.float32)


def real_audio_10k(resample):
    """The 3 s real-audio excerpt at 10 kHz; ``resample(x, 44100, 10000)`` is the caller's (the device's on the GPU, scipy's on the
    host).  None when the fixture is not in the tree."""
    path = os.path.join(GOLDEN, "real_audio_17480-2-0-24.npz")
    if not os.path.exists(path):
        return None
    fx = np.load(path)
    x = (fx["lr_sum_int16"].astype(np.float64) / 65536.0).astype(np.float32)
    return np.asarray(resample(x, int(fx["sample_rate"]), 10000), dtype=np.float64)


def stoi_cases(resample=None):
    """[(name, est (L,), ref (L,))] at 10 kHz.  The keep / drop decision is a threshold, so every case asserts here, in the float64
    restatement, that no frame's level lies within 0.1 dB of max - 40 dB: a condition on the input, not a tolerance."""
    cases = []
    rng = _rng(4097)
    cases.append(("L4097_one_segment", *_pair(rng, _speechlike(rng, 4097), 5.0)))
    cases.append(("L4096_too_short", *_pair(rng, _speechlike(rng, 4096), 5.0)))
    rng = _rng(20000)
    x = _speechlike(rng, 20000)
    # loud, -20 dB and -50 dB stretches; boundaries off the hop grid too, so that frames straddle them
    cases.append(("quiet_middle", *_pair(rng, _with_levels(x, [(3000, 5000, -20.0), (8229, 12890, -50.0)]), 5.0)))
    cases.append(("quiet_ends", *_pair(rng, _with_levels(x, [(0, 2341, -50.0), (9000, 9800, -20.0), (17000, 20000, -50.0)]), 0.0)))
    if resample is not None:
        real = real_audio_10k(resample)
        if real is not None:
            cases.append(("real_audio_5dB", *_pair(_rng(17480), real, 5.0)))
    for name, est, ref in cases:
        assert qr.threshold_margin_db(ref) > 0.1, (name, qr.threshold_margin_db(ref))
    return cases


def scipy_resample(x, src, dst):
    from math import gcd
    import scipy.signal
    g = gcd(src, dst)
    return scipy.signal.resample_poly(np.asarray(x, np.float64), dst // g, src // g)


def measure_floor():
    """Worst |float32 restatement - float64 restatement| per metric over all the cases above."""
    worst = {"snr": 0.0, "si_sdr": 0.0, "seg_snr": 0.0, "stoi": 0.0}

    def upd(key, a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        both = np.isfinite(a) & np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)])
        if both.any():
            worst[key] = max(worst[key], float(np.max(np.abs(a[both] - b[both]))))

    tc = time_cases() + [("high_sdr", *high_sdr_case(), None)]
    for name, est, ref, lengths in tc:
        lens = [est.shape[1]] * est.shape[0] if lengths is None else lengths
        for seg in SEG_FRAMES:
            for i, n in enumerate(lens):
                q64 = qr.quality_ref(est[i, :n], ref[i, :n], seg)
                q32 = qr.quality_ref(est[i, :n], ref[i, :n], seg, np.float32)
                for k, key in enumerate(("snr", "si_sdr", "seg_snr")):
                    upd(key, q32[k], q64[k])
    for name, est, ref in stoi_cases(scipy_resample):
        upd("stoi", qr.stoi_ref(est, ref, np.float32), qr.stoi_ref(est, ref))
    return worst


if __name__ == "__main__":
    for k, v in measure_floor().items():
        print(f"{k:8s} {v:.3e}")
