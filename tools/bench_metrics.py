#!/usr/bin/env python3
"""Device time of the quality metrics (adn_quality; resample to 10 kHz + adn_stoi) beside the same quantities composed from torch
ops on the device.  Buffers are allocated once; device events around a window of calls (at least `--window-ms` long, sized from a
calibration call) after a warm-up, median of `--groups` windows.  One JSON line per measurement:

    adn_quality        the C entry point; `bound_ms` = its four array reads (est and ref, twice) at 8 TB/s, `share_of_bound`
    torch_quality      SNR, SI-SDR and segmental SNR from torch reductions (fp32), same inputs
    resample+adn_stoi  adn_resample of both signals 8 kHz -> 10 kHz, then adn_stoi; `stoi_ms` is adn_stoi alone
    torch_stoi         the resampled signals through a torch restatement of adn.h's steps 1-7, clip by clip (the kept-frame count
                       differs per clip), fp32; the resampling is not repeated (it is the same call)
    agreement          max |library - torch| per metric over the clips: the torch forms are a scale for the time, not a reference

Workloads: one hour of 8 kHz audio as 60 clips of 60 s, and one clip of 3 s.

    python tools/bench_metrics.py [--cases 0,1]

Kernel-level numbers: rocprofv3 --kernel-trace --stats -- python tools/bench_metrics.py --cases 0 (a run of its own).
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import time_ms  # noqa: E402

HBM_BPS = 8.0e12
RATE = 8000
CASES = (("one_hour", 60, 60 * RATE), ("one_clip_3s", 1, 3 * RATE))
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))


def torch_quality(e, r, seg):
    import torch
    d = e - r
    srr = (r * r).sum(1)
    snr = 10 * torch.log10(srr / (d * d).sum(1))
    alpha = (e * r).sum(1) / srr
    t = alpha[:, None] * r
    res = e - t
    si = 10 * torch.log10((t * t).sum(1) / (res * res).sum(1))
    nfr = e.shape[1] // seg
    rf, df = r[:, :nfr * seg].reshape(-1, nfr, seg), d[:, :nfr * seg].reshape(-1, nfr, seg)
    v = 10 * torch.log10(((rf * rf).sum(2) + 1e-10) / ((df * df).sum(2) + 1e-10))
    return torch.stack([snr, si, v.clamp(-10, 35).mean(1)], 1)


def torch_stoi_clip(e, r, w, band):
    """Steps 1-7 of include/adn.h for one clip at 10 kHz (1-D tensors), fp32."""
    import torch
    eps = 2.0 ** -52
    nf = (len(r) - 256 + 127) // 128 if len(r) > 256 else 0
    if nf == 0:
        return torch.tensor(float("nan"), device=r.device)
    xr, xe = r.unfold(0, 256, 128)[:nf] * w, e.unfold(0, 256, 128)[:nf] * w
    lev = 20 * torch.log10(xr.norm(dim=1).double() + eps)
    keep = lev > lev.max() - 40
    xr, xe = xr[keep], xe[keep]
    k = xr.shape[0]
    if k < 31:
        return torch.tensor(float("nan"), device=r.device)
    env = []
    for x in (xr, xe):
        c = torch.zeros(128 * (k + 1), device=r.device)
        c[:128 * k] += x[:, :128].reshape(-1)
        c[128:] += x[:, 128:].reshape(-1)
        p = torch.fft.rfft(c.unfold(0, 256, 128)[:k - 1] * w, n=512).abs() ** 2
        env.append(torch.sqrt(p @ band))                                  # (J, 15)
    x, y = (v.unfold(0, 30, 1) for v in env)                              # (J - 29, 15, 30)
    a = x.norm(dim=2, keepdim=True) / (y.norm(dim=2, keepdim=True) + eps)
    y = torch.minimum(a * y, x * (1 + 10 ** (15 / 20)))
    x, y = x - x.mean(2, keepdim=True), y - y.mean(2, keepdim=True)
    rho = ((x / (x.norm(dim=2, keepdim=True) + eps)) * (y / (y.norm(dim=2, keepdim=True) + eps))).sum(2)
    return rho.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1", help="indices into CASES")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: no ROCm device is visible; nothing is measured without one")
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    w = torch.from_numpy(np.hanning(258)[1:-1].astype(np.float32)).to(dev)
    band = torch.zeros((257, 15), device=dev)
    for b, (lo, hi) in enumerate(BANDS):
        band[lo:hi, b] = 1.0
    _lib.check(L.adn_resample_prepare(0, RATE, 10000), "adn_resample_prepare")
    for k in (int(v) for v in args.cases.split(",")):
        name, n, length = CASES[k]
        g = torch.Generator(device=dev).manual_seed(k)
        t = torch.arange(length, device=dev) / RATE
        ref = 0.3 * (0.6 + 0.4 * torch.sin(2 * math.pi * 3.0 * t)) * torch.randn((n, length), generator=g, device=dev)
        est = ref + 0.05 * torch.randn((n, length), generator=g, device=dev)
        seg = int(0.03 * RATE)
        need = ctypes.c_size_t()
        _lib.check(L.adn_quality_workspace_bytes(n, length, ctypes.byref(need)), "adn_quality_workspace_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        out = torch.empty((n, 3), device=dev)

        def quality():
            _lib.check(L.adn_quality(est.data_ptr(), ref.data_ptr(), None, n, length, seg, ws.data_ptr(), need.value, out.data_ptr(), st),
                       "adn_quality")
        row = time_ms(quality, args.warmup, args.groups, args.window_ms)
        nbytes = 4 * n * length * 4
        bound = nbytes / HBM_BPS * 1e3
        print(json.dumps({"case": name, "what": "adn_quality", "shape": [n, length], "seg_frame": seg, **row, "bytes": nbytes,
                          "GBps": round(nbytes / (row["ms"] * 1e-3) / 1e9, 1), "bound": "memory (4 array reads at 8 TB/s)",
                          "bound_ms": round(bound, 4), "share_of_bound": round(bound / row["ms"], 3)}), flush=True)
        row = time_ms(lambda: torch_quality(est, ref, seg), args.warmup, args.groups, args.window_ms)
        print(json.dumps({"case": name, "what": "torch_quality", "shape": [n, length], **row}), flush=True)
        tq = torch_quality(est, ref, seg)

        m = ctypes.c_long()
        _lib.check(L.adn_resample_length(length, RATE, 10000, ctypes.byref(m)), "adn_resample_length")
        e10, r10 = torch.empty((n, m.value), device=dev), torch.empty((n, m.value), device=dev)
        _lib.check(L.adn_stoi_workspace_bytes(n, m.value, ctypes.byref(need)), "adn_stoi_workspace_bytes")
        ws2 = torch.empty(need.value, dtype=torch.uint8, device=dev)
        d = torch.empty((n,), device=dev)

        def stoi_only():
            _lib.check(L.adn_stoi(e10.data_ptr(), r10.data_ptr(), None, n, m.value, ws2.data_ptr(), need.value, d.data_ptr(), st), "adn_stoi")

        def stoi_all():
            _lib.check(L.adn_resample(est.data_ptr(), n, length, RATE, 10000, e10.data_ptr(), st), "adn_resample")
            _lib.check(L.adn_resample(ref.data_ptr(), n, length, RATE, 10000, r10.data_ptr(), st), "adn_resample")
            stoi_only()
        row = time_ms(stoi_all, args.warmup, args.groups, args.window_ms)
        alone = time_ms(stoi_only, args.warmup, args.groups, args.window_ms)
        print(json.dumps({"case": name, "what": "resample+adn_stoi", "shape": [n, length], "shape_10k": [n, m.value], **row,
                          "stoi_ms": alone["ms"], "workspace_bytes": need.value}), flush=True)
        row = time_ms(lambda: torch.stack([torch_stoi_clip(e10[i], r10[i], w, band) for i in range(n)]), 1, 3, args.window_ms)
        print(json.dumps({"case": name, "what": "torch_stoi", "shape_10k": [n, m.value], **row}), flush=True)
        ts = torch.stack([torch_stoi_clip(e10[i], r10[i], w, band) for i in range(n)])
        torch.cuda.synchronize()
        print(json.dumps({"case": name, "what": "agreement",
                          "max_abs_diff": {"snr": float((out[:, 0] - tq[:, 0]).abs().max()), "si_sdr": float((out[:, 1] - tq[:, 1]).abs().max()),
                                           "seg_snr": float((out[:, 2] - tq[:, 2]).abs().max()), "stoi": float((d - ts).abs().max())},
                          "first_clip": {"snr": float(out[0, 0]), "si_sdr": float(out[0, 1]), "seg_snr": float(out[0, 2]),
                                         "stoi": float(d[0])}}), flush=True)
        del est, ref, e10, r10
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
