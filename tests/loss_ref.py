"""CombinedPerceptualLoss per clip, written out: the float64 reference of the loss case table (tests/loss_cases.py), the two float32
restatements that measure the floor, and the mutation hooks of the host sensitivity test.  TEST INFRASTRUCTURE, CPU only.

``per_clip(pred, target)`` states the operator of csrc/loss_kernels.hip with no ``torch.stft``: the frequency-mean series, frames cut
from an explicitly padded series (zeros for the three |STFT| scales, the mirrored neighbours of each edge for the mel term),
explicit DFT matrices, the periodic Hann window, the HTK filterbank of ``oracle.loss_torch.mel_filterbank()`` and the four outputs
{total, stft, mel, l1}.  It runs in the dtype of its inputs and stays differentiable under torch autograd: float64 is the reference
(anchored on ``test_loss_grad_host.per_clip_autograd`` in tests/test_loss_cases_host.py), float32 is the LIBRARY-ORDER floor.

``per_clip_kernel_order`` is the KERNEL-ORDER float32 floor, the order of loss_colsum_kernel / loss_finish_kernel: row sums in slabs
of 32 and then across slabs, division by F, a float32 twiddle table indexed by (k i) mod n, one float32 accumulator per component
walked over the n window samples, |X|^2 as re re + im im, filterbank sums walked over the 32 bins.  What it does not restate: whether
the compiler contracts ``acc += a * c`` into a fused multiply-add, and the order of the final sums over (bin, frame) items (256
strided lanes and a shuffle tree on the device, torch's pairwise sum here); both stay inside the factor 4 of the bounds.

|X| is sqrt(re^2 + im^2) with derivative 0 at 0, the kernel's ``ap > 0 ? g / ap : 0`` and torch's abs'(0) = 0, so that frames that
are exactly zero (the far field of the burst cases) have a gradient of exactly 0 instead of NaN.

Mutations (``mut``, a dict; float64 host test only, never on a path the device is compared on):
  fb_row       (k, s)               filterbank row (frequency bin) k times s
  bin          (scale, k, s)        |X| of bin k of |STFT| scale 0..2 times s, both signals
  frame        (term, frames, s)    the |difference| of the listed frames of term 0..2 (|STFT| scales) or 3 (mel) times s; s = 0 drops
  edge_repeat  "left" | "right"     reflect WITH edge repeat on that side of the mel term
  stft_reflect True                 reflect instead of zero padding in the |STFT| term
  drop_grad    (term, frame, pos)   frame ``frame`` of term 0..3 reads series position pos as a constant: the forward value is
                                    unchanged, the gradient loses that frame's contribution to that position
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import loss_torch as L

SCALES = L.SCALES
MEL = 3                                    # term index of the mel transform (0..2 are the |STFT| scales)
EPS32 = 2.0 ** -23                         # no floor is below one unit in the last place of float32
MARGIN = 4.0                               # the project's standing margin over a measured float32 floor


def n_frames(T: int, n: int, hop: int) -> int:
    return 1 + (T + 2 * (n // 2) - n) // hop


def live_mels() -> np.ndarray:
    """Indices of the mel filters with any weight (the others are identically zero on 32 bins)."""
    return np.nonzero(L.mel_filterbank().sum(axis=0) > 0)[0]


def live_rows() -> np.ndarray:
    """Indices of the filterbank rows (frequency bins) with any weight: all but 0 and 31."""
    return np.nonzero(L.mel_filterbank().sum(axis=1) > 0)[0]


def _table(n: int, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """cos(2 pi j / n), -sin(2 pi j / n) for j < n, computed in float64 and rounded once."""
    j = np.arange(n, dtype=np.float64)
    return (torch.from_numpy(np.cos(2 * np.pi * j / n)).to(dtype), torch.from_numpy(-np.sin(2 * np.pi * j / n)).to(dtype))


def _dft(n: int, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """(n, n/2+1) matrices C[i, k] = cos(2 pi k i / n), S[i, k] = -sin(2 pi k i / n), the argument reduced as (k i) mod n."""
    c, s = _table(n, torch.float64)
    idx = (np.arange(n)[:, None] * np.arange(n // 2 + 1)[None, :]) % n
    return c[idx].to(dtype), s[idx].to(dtype)


def _hann(n: int, dtype) -> torch.Tensor:
    i = np.arange(n, dtype=np.float64)
    return torch.from_numpy(0.5 - 0.5 * np.cos(2 * np.pi * i / n)).to(dtype)


def _index(T: int, n: int, hop: int) -> np.ndarray:
    """(frames, n): position of window sample i of frame fr in the unpadded series, fr hop - n/2 + i."""
    return np.arange(n_frames(T, n, hop))[:, None] * hop - n // 2 + np.arange(n)[None, :]


def _reflect(idx: np.ndarray, T: int, edge_repeat=None) -> np.ndarray:
    left = -idx - 1 if edge_repeat == "left" else -idx
    right = 2 * T - 1 - idx if edge_repeat == "right" else 2 * (T - 1) - idx
    return np.where(idx < 0, left, np.where(idx >= T, right, idx))


def _frames(x: torch.Tensor, n: int, hop: int, reflect: bool, edge_repeat=None, drop=None) -> torch.Tensor:
    """(B, T) -> (B, frames, n).  The padding is explicit: n/2 zeros on each side, or the n/2 neighbours of each edge mirrored
    (without the edge sample itself; with it under the edge_repeat mutation); frame fr is xp[fr hop : fr hop + n]."""
    T, pad = x.shape[1], n // 2
    if reflect:
        left = x[:, :pad] if edge_repeat == "left" else x[:, 1:pad + 1]
        right = x[:, T - pad:] if edge_repeat == "right" else x[:, T - pad - 1:T - 1]
        xp = torch.cat([left.flip(1), x, right.flip(1)], dim=1)
    else:
        z = torch.zeros(x.shape[0], pad, dtype=x.dtype)
        xp = torch.cat([z, x, z], dim=1)
    fr = xp.unfold(1, n, hop)
    assert fr.shape[1] == n_frames(T, n, hop)
    if drop is not None:
        frame, pos = drop
        idx = _index(T, n, hop)
        src = _reflect(idx, T, edge_repeat) if reflect else np.where((idx >= 0) & (idx < T), idx, -1)
        mask = np.zeros(src.shape, dtype=bool)
        mask[frame] = src[frame] == pos
        assert mask.any(), ("frame does not read the position", frame, pos)
        fr = torch.where(torch.from_numpy(mask), fr.detach(), fr)
    return fr


def _mm(a: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """(B, frames, n) @ (n, k) as one 2-D product (a batch of 65537 small ones is slow on the host)."""
    return (a.reshape(-1, a.shape[2]) @ m).reshape(a.shape[0], a.shape[1], m.shape[1])


def _mag(re: torch.Tensor, im: torch.Tensor) -> torch.Tensor:
    p = re * re + im * im
    pos = p > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, p, torch.ones_like(p))), torch.zeros_like(p))


def _combine(stft, mel, l1, dtype):
    w = torch.tensor([L.W_STFT, L.W_MEL, L.W_L1], dtype=dtype)
    return torch.stack([w[0] * stft + w[1] * mel + w[2] * l1, stft, mel, l1], dim=1)


def per_clip(pred: torch.Tensor, target: torch.Tensor, mut: dict | None = None, gaps: list | None = None) -> torch.Tensor:
    """(B,1,F,T) x2 -> (B,4) = [total, stft, mel, l1] per clip in the inputs' dtype (library order).  ``gaps``, if a list, receives
    the detached quantities whose signs the gradient depends on: |Xp| - |Xq| per scale (B, frames, bins), Mp - Mq over the live mel
    filters (B, frames, live), pred - target."""
    mut = mut or {}
    dt = pred.dtype
    b, T = pred.shape[0], pred.shape[3]
    p = pred.mean(dim=2).squeeze(1)
    q = target.mean(dim=2).squeeze(1)
    drop = mut.get("drop_grad")
    stft = torch.zeros(b, dtype=dt)
    for sc, (n, hop) in enumerate(SCALES):
        C, S = _dft(n, dt)
        d = (drop[1], drop[2]) if drop is not None and drop[0] == sc else None
        fp = _frames(p, n, hop, bool(mut.get("stft_reflect")), drop=d)
        fq = _frames(q, n, hop, bool(mut.get("stft_reflect")), drop=d)
        pm = _mag(_mm(fp, C), _mm(fp, S))
        qm = _mag(_mm(fq, C), _mm(fq, S))
        if "bin" in mut and mut["bin"][0] == sc:
            s = torch.ones(n // 2 + 1, dtype=dt)
            s[mut["bin"][1]] = mut["bin"][2]
            pm, qm = pm * s, qm * s
        if gaps is not None:
            gaps.append((pm - qm).detach())
        diff = (pm - qm).abs()
        if "frame" in mut and mut["frame"][0] == sc:
            s = torch.ones(diff.shape[1], 1, dtype=dt)
            s[list(mut["frame"][1])] = mut["frame"][2]
            diff = diff * s
        stft = stft + diff.reshape(b, -1).mean(dim=1)
    stft = stft / len(SCALES)

    n, hop = L.MEL_NFFT, L.MEL_HOP
    fb = L.mel_filterbank().copy()
    if "fb_row" in mut:
        fb[mut["fb_row"][0]] *= mut["fb_row"][1]
    fb = torch.from_numpy(fb).to(dt)
    C, S = _dft(n, dt)
    win = _hann(n, dt)
    d = (drop[1], drop[2]) if drop is not None and drop[0] == MEL else None

    def mel(x):
        fr = _frames(x, n, hop, True, mut.get("edge_repeat"), drop=d) * win
        re, im = _mm(fr, C), _mm(fr, S)
        return _mm(re * re + im * im, fb)                  # (B, frames, 64)
    mp, mq = mel(p), mel(q)
    if gaps is not None:
        gaps.append((mp - mq).detach()[:, :, torch.from_numpy(live_mels())])
        gaps.append((pred - target).detach())
    diff = (mp - mq).abs()
    if "frame" in mut and mut["frame"][0] == MEL:
        s = torch.ones(diff.shape[1], 1, dtype=dt)
        s[list(mut["frame"][1])] = mut["frame"][2]
        diff = diff * s
    melv = diff.reshape(b, -1).mean(dim=1)
    l1 = (pred - target).abs().reshape(b, -1).mean(dim=1)
    return _combine(stft, melv, l1, dt)


# ---- kernel order, float32 -------------------------------------------------------------------------------------------------------
def _series_kernel_order(x: torch.Tensor) -> torch.Tensor:
    """(B,1,F,T) float32 -> (B,T): sums over slabs of 32 rows walked row by row, the slab partials walked slab by slab, / F."""
    b, _, F, T = x.shape
    nslab = (F + 31) // 32
    x = x[:, 0]
    if nslab * 32 != F:                                    # rows of zeros: x + 0 is x, the sums are unchanged
        x = torch.cat([x, torch.zeros(b, nslab * 32 - F, T, dtype=x.dtype)], dim=1)
    x = x.reshape(b, nslab, 32, T)
    part = torch.zeros(b, nslab, T, dtype=x.dtype)
    for row in x.unbind(2):
        part = part + row
    acc = torch.zeros(b, T, dtype=x.dtype)
    for slab in part.unbind(1):
        acc = acc + slab
    return acc / torch.tensor(float(F), dtype=x.dtype)


def _walk(fr: torch.Tensor, tc: torch.Tensor, ts: torch.Tensor, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(B, frames, n) -> re, im (B, frames, bins): one accumulator per component walked over the window samples."""
    nb = n // 2 + 1
    k = torch.arange(nb)
    re = torch.zeros(*fr.shape[:2], nb, dtype=fr.dtype)
    im = torch.zeros_like(re)
    for i, a in enumerate(fr.unsqueeze(3).unbind(2)):
        idx = (k * i) % n
        re = re + a * tc[idx]
        im = im + a * ts[idx]
    return re, im


def per_clip_kernel_order(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The float32 restatement in loss_finish_kernel's order (module docstring); differentiable, its autograd gradient is the
    kernel-order gradient floor."""
    assert pred.dtype == torch.float32 and target.dtype == torch.float32
    dt = torch.float32
    b, _, F, T = pred.shape
    p = _series_kernel_order(pred)
    q = _series_kernel_order(target)
    stft = torch.zeros(b, dtype=dt)
    for n, hop in SCALES:
        tc, ts = _table(n, dt)
        rp, ip = _walk(_frames(p, n, hop, False), tc, ts, n)
        rq, iq = _walk(_frames(q, n, hop, False), tc, ts, n)
        d = (_mag(rp, ip) - _mag(rq, iq)).abs()
        stft = stft + d.reshape(b, -1).sum(dim=1) / torch.tensor(float(d.shape[1] * d.shape[2]), dtype=dt)
    stft = stft / torch.tensor(3.0, dtype=dt)

    n, hop = L.MEL_NFFT, L.MEL_HOP
    tc, ts = _table(n, dt)
    win = torch.tensor(0.5, dtype=dt) - torch.tensor(0.5, dtype=dt) * tc      # 0.5f - 0.5f * tc[i]
    fb = torch.from_numpy(L.mel_filterbank()).to(dt)

    def mel(x):
        re, im = _walk(_frames(x, n, hop, True) * win, tc, ts, n)
        pw = re * re + im * im
        m = torch.zeros(*pw.shape[:2], fb.shape[1], dtype=dt)
        for f, col in enumerate(pw.unsqueeze(3).unbind(2)):
            m = m + fb[f] * col
        return m
    d = (mel(p) - mel(q)).abs()
    melv = d.reshape(b, -1).sum(dim=1) / torch.tensor(float(d.shape[1] * d.shape[2]), dtype=dt)
    l1 = (pred - target).abs().reshape(b, -1).sum(dim=1) / (torch.tensor(float(F), dtype=dt) * torch.tensor(float(T), dtype=dt))
    return _combine(stft, melv, l1, dt)


# ---- values, gradients, statistics -----------------------------------------------------------------------------------------------
def run(fn, pred: torch.Tensor, target: torch.Tensor, weights: torch.Tensor | None, dtype, **kw):
    """fn on CPU copies of the inputs in ``dtype``: (out, grad_pred, grad_target) as float64, the gradients those of
    sum(out * weights) (None without weights)."""
    p = pred.detach().cpu().to(dtype)
    q = target.detach().cpu().to(dtype)
    if weights is None:
        with torch.no_grad():
            return fn(p, q, **kw).double(), None, None
    p.requires_grad_()
    q.requires_grad_()
    out = fn(p, q, **kw)
    (out * weights.to(dtype)).sum().backward()
    return out.detach().double(), p.grad.double(), q.grad.double()


def _rel(err: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """err / ref element-wise; 0 where both are 0, inf where only the reference is."""
    safe = torch.where(ref > 0, ref, torch.ones_like(ref))
    return torch.where(ref > 0, err / safe, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


STATS = ("total", "stft", "mel", "l1", "pred_l2", "pred_max", "target_l2", "target_max")


def deviations(got, ref) -> dict[str, torch.Tensor]:
    """got, ref: (out, grad_pred, grad_target) in float64 -> statistic name -> (B,) relative deviation per clip: the four output
    columns |got - ref| / |ref|, and per gradient ||g - g_ref||_2 / ||g_ref||_2 and max|g - g_ref| / max|g_ref|."""
    d = {}
    rel = _rel((got[0] - ref[0]).abs(), ref[0].abs())
    for j, name in enumerate(STATS[:4]):
        d[name] = rel[:, j]
    for name, g, r in (("pred", got[1], ref[1]), ("target", got[2], ref[2])):
        if r is None:
            continue
        b = r.shape[0]
        e, r = (g - r).reshape(b, -1), r.reshape(b, -1)
        d[name + "_l2"] = _rel(e.norm(dim=1), r.norm(dim=1))
        d[name + "_max"] = _rel(e.abs().amax(dim=1), r.abs().amax(dim=1))
    return d


def floors(pred, target, weights, ref, kernel_every: int = 1) -> dict[str, dict[str, float]]:
    """{"library" | "kernel" | "floor": statistic -> largest deviation from ``ref`` over the clips}; "floor" is the larger of the two
    float32 restatements and never below 2^-23.  kernel_every = k runs the kernel-order restatement (a Python loop per window
    sample) on every k-th clip only: clips are independent, and a maximum over fewer clips can only lower the floor."""
    res = {}
    for key, fn, k in (("library", per_clip, 1), ("kernel", per_clip_kernel_order, kernel_every)):
        pick = lambda x: None if x is None else x[::k]       # noqa: E731
        dev = deviations(run(fn, pred[::k], target[::k], pick(weights), torch.float32), tuple(pick(r) for r in ref))
        res[key] = {k: float(v.max()) for k, v in dev.items()}
    res["floor"] = {k: max(res["library"][k], res["kernel"][k], EPS32) for k in res["library"]}
    return res


# ---- per_clip_l1 -----------------------------------------------------------------------------------------------------------------
def l1_float64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a.double() - b.double()).abs().reshape(a.shape[0], -1).mean(dim=1)


def l1_kernel_order(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """per_clip_l1_kernel in float32: 256 lanes each walk their stride-256 elements, a shuffle tree inside each wave of 64, the four
    waves added in order, / elems."""
    n = a.shape[0]
    d = (a - b).abs().reshape(n, -1)
    elems = d.shape[1]
    rows = (elems + 255) // 256
    if rows * 256 != elems:
        d = torch.cat([d, torch.zeros(n, rows * 256 - elems, dtype=d.dtype)], dim=1)
    d = d.reshape(n, rows, 256)
    s = torch.zeros(n, 256, dtype=torch.float32)
    for r in range(rows):
        s = s + d[:, r]
    s = s.reshape(n, 4, 64)
    o = 32
    while o > 0:
        s = torch.cat([s[:, :, :o] + s[:, :, o:2 * o], s[:, :, o:]], dim=2)
        o //= 2
    part = s[:, :, 0]
    return (((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]) / torch.tensor(float(elems), dtype=torch.float32)
