"""Restatement of the "quality" operators of include/adn.h (adn_quality, adn_stoi), written from the header text: the independent
second implementation the device kernels are compared with.  A plain helper module (no fixtures).

Everything takes a ``dtype``: ``numpy.float64`` (the default) is the reference; ``numpy.float32`` runs the SAME statements with
float32 data, float32 sums and scipy's float32 FFT -- the rounding floor of the number format, from which the GPU tests take their
bounds (see FLOOR below and profiles/bench_metrics.md).
"""
import numpy as np

EPS = 2.0 ** -52
FRAME, HOP, NFFT, BANDS, SEG = 256, 128, 512, 15, 30
BETA_DB, RANGE_DB = -15.0, 40.0
BAND_TABLE = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
              (109, 138), (138, 174), (174, 219))

# Worst |float32 restatement - float64 restatement| over the cases of tests/quality_cases.py, per metric (dB, dB, dB, STOI units),
# measured on the host by `python tests/quality_cases.py` (profiles/bench_metrics.md); the device bounds are 4 x these.
FLOOR = {"snr": 6.157e-06, "si_sdr": 1.700e-05, "seg_snr": 2.925e-06, "stoi": 7.054e-07}
BOUND = {k: 4.0 * v for k, v in FLOOR.items()}


# ---- time-domain metrics ---------------------------------------------------------------------------------------------------------
def quality_ref(est, ref, seg_frame, dtype=np.float64):
    """(SNR, SI-SDR, segmental SNR) in dB of one clip (1-D arrays of one length)."""
    e, r = np.asarray(est, dtype=dtype), np.asarray(ref, dtype=dtype)
    assert e.shape == r.shape and e.ndim == 1
    ten, tiny = dtype(10.0), dtype(1e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        srr = np.sum(r * r, dtype=dtype)
        sdd = np.sum((e - r) ** 2, dtype=dtype)
        snr = ten * np.log10(srr / sdd)
        alpha = np.sum(e * r, dtype=dtype) / srr
        t = alpha * r
        si_sdr = ten * np.log10(np.sum(t * t, dtype=dtype) / np.sum((e - t) ** 2, dtype=dtype))
        nfr = len(r) // seg_frame
        if nfr == 0:
            seg = dtype(np.nan)
        else:
            ef = e[:nfr * seg_frame].reshape(nfr, seg_frame)
            rf = r[:nfr * seg_frame].reshape(nfr, seg_frame)
            v = ten * np.log10((np.sum(rf * rf, axis=1, dtype=dtype) + tiny) / (np.sum((ef - rf) ** 2, axis=1, dtype=dtype) + tiny))
            seg = np.mean(np.clip(v, dtype(-10.0), dtype(35.0)), dtype=dtype)
    return np.array([snr, si_sdr, seg], dtype=dtype)


def si_sdr_expanded_f32(est, ref):
    """The form adn.h forbids: the residual as sum e^2 - Ser^2 / Srr, in float32 -- what the high-SDR test must tell apart."""
    e, r = np.asarray(est, np.float32), np.asarray(ref, np.float32)
    see, srr, ser = np.sum(e * e, dtype=np.float32), np.sum(r * r, dtype=np.float32), np.sum(e * r, dtype=np.float32)
    tgt = ser * ser / srr
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(10.0) * np.log10(tgt / (see - tgt))


# ---- STOI ------------------------------------------------------------------------------------------------------------------------
def band_table():
    """Step 5's bin ranges computed from their definition (tests/test_quality_host.py compares them with BAND_TABLE)."""
    f = np.linspace(0, 10000, NFFT + 1)[:NFFT // 2 + 1]
    out = []
    for b in range(BANDS):
        lo, hi = 150.0 * 2.0 ** ((2 * b - 1) / 6.0), 150.0 * 2.0 ** ((2 * b + 1) / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return tuple(out)


def window(dtype=np.float64):
    return np.hanning(FRAME + 2)[1:-1].astype(dtype)


def frame_starts(length):
    return list(range(0, length - FRAME, HOP))


def frame_levels(ref):
    """E_i of step 2 in float64 (what the fixtures check their threshold margin on)."""
    r = np.asarray(ref, np.float64)
    w = window()
    return np.array([20.0 * np.log10(np.linalg.norm(w * r[s:s + FRAME]) + EPS) for s in frame_starts(len(r))])


def threshold_margin_db(ref):
    """Smallest distance of a frame's level from the keep / drop threshold max - 40 dB (inf with no frame)."""
    lv = frame_levels(ref)
    return float(np.min(np.abs(lv - (lv.max() - RANGE_DB)))) if len(lv) else float("inf")


def _rfft(x, dtype):
    if dtype == np.float64:
        return np.fft.rfft(x, NFFT)
    import scipy.fft
    out = scipy.fft.rfft(np.asarray(x, np.float32), NFFT)
    assert out.dtype == np.complex64
    return out


def stoi_parts(est, ref, dtype=np.float64):
    """Steps 1-5: (kept frame indices, envelopes of ref (15, J), envelopes of est (15, J))."""
    e, r = np.asarray(est, dtype=dtype), np.asarray(ref, dtype=dtype)
    assert e.shape == r.shape and e.ndim == 1
    w = window(dtype)
    starts = frame_starts(len(r))
    if not starts:
        return np.zeros(0, int), np.zeros((BANDS, 0), dtype), np.zeros((BANDS, 0), dtype)
    xr = np.stack([w * r[s:s + FRAME] for s in starts])                       # 1.
    xe = np.stack([w * e[s:s + FRAME] for s in starts])
    norms = np.sqrt(np.sum(xr * xr, axis=1, dtype=dtype))
    lev = 20.0 * np.log10(norms.astype(np.float64) + EPS)                     # 2.
    idx = np.nonzero(lev > lev.max() - RANGE_DB)[0]
    K = len(idx)
    cr, ce = np.zeros(HOP * (K + 1), dtype), np.zeros(HOP * (K + 1), dtype)   # 3. explicit overlap-add, ascending j
    for j in range(K):
        cr[HOP * j:HOP * j + FRAME] += xr[idx[j]]
        ce[HOP * j:HOP * j + FRAME] += xe[idx[j]]
    cstarts = frame_starts(len(cr))                                           # 4.
    assert len(cstarts) == K - 1
    lo_hi = BAND_TABLE
    tr, te = np.zeros((BANDS, len(cstarts)), dtype), np.zeros((BANDS, len(cstarts)), dtype)
    for j, s in enumerate(cstarts):
        pr = np.abs(_rfft(w * cr[s:s + FRAME], dtype)) ** 2
        pe = np.abs(_rfft(w * ce[s:s + FRAME], dtype)) ** 2
        for b, (lo, hi) in enumerate(lo_hi):                                  # 5.
            tr[b, j] = np.sqrt(np.sum(pr[lo:hi], dtype=dtype))
            te[b, j] = np.sqrt(np.sum(pe[lo:hi], dtype=dtype))
    return idx, tr, te


def stoi_ref(est, ref, dtype=np.float64):
    """d of step 7 for one clip already at 10 kHz; NaN when fewer than 30 compacted frames remain."""
    _, tr, te = stoi_parts(est, ref, dtype)
    J = tr.shape[1]
    if J < SEG:
        return dtype(np.nan)
    clipf = dtype(1.0 + 10.0 ** (-BETA_DB / 20.0))
    eps = dtype(EPS)

    def norm(v):
        return np.sqrt(np.sum(v * v, dtype=dtype))

    total = dtype(0.0)
    for m in range(SEG, J + 1):                                               # 6.
        for b in range(BANDS):
            x, y = tr[b, m - SEG:m], te[b, m - SEG:m]
            a = norm(x) / (norm(y) + eps)
            yp = np.minimum(a * y, x * clipf)
            xm, ym = x - np.mean(x, dtype=dtype), yp - np.mean(yp, dtype=dtype)
            total += np.sum((xm / (norm(xm) + eps)) * (ym / (norm(ym) + eps)), dtype=dtype)
    return dtype(total / dtype(BANDS * (J - SEG + 1)))                        # 7.


def evaluate_ref(est, ref, seg_frame, lengths=None, dtype=np.float64):
    """Both operators over a batch (n, L) with optional per-row lengths: (n, 3) and (n,)."""
    est, ref = np.atleast_2d(est), np.atleast_2d(ref)
    n = est.shape[0]
    lens = [est.shape[1]] * n if lengths is None else [int(v) for v in lengths]
    q = np.stack([quality_ref(est[i, :lens[i]], ref[i, :lens[i]], seg_frame, dtype) for i in range(n)])
    s = np.array([stoi_ref(est[i, :lens[i]], ref[i, :lens[i]], dtype) for i in range(n)], dtype=dtype)
    return q, s
