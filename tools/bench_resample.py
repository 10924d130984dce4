#!/usr/bin/env python3
"""Device time of the resampler (adn_resample) and the SNR mixer (adn_mix_snr) through the C ABI, buffers allocated once.
Device events around a window of calls (at least `--window-ms` long, sized from a calibration run) after a warm-up, median
of `--groups` windows.  One JSON line per case:

    bytes   algorithmic HBM traffic: input read once + output written once (mix_snr: clean and noise read twice, out written)
    fmas    multiply-adds of the definition in include/adn.h: outputs x (2 * half + 1) / up taps (mix_snr: 2 per sample for the
            sums + 1 for the mix)
    bound   the larger of bytes / 8 TB/s and 2 * fmas / 157.3 TFLOP/s (fp32 vector peak, packed FMA), and which one it is
    share   bound_ms / ms

    python tools/bench_resample.py                      # the four device cases
    python tools/bench_resample.py --host-baseline      # scipy.signal.resample_poly (or the float64 test reference) on the
                                                        # 64-clip case over 16 processes: a scale, not a target; no GPU used

Kernel-level numbers: rocprofv3 --kernel-trace --stats -- python tools/bench_resample.py --cases 0 (a run of its own).
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12
FP32_FLOPS = 157.3e12
CASES = (("resample", 64, 176400, 44100, 8000), ("resample", 10000, 176400, 44100, 8000),
         ("resample", 10000, 32000, 8000, 44100), ("mix_snr", 10000, 16000, 0, 0))


def taps_per_output(src, dst):
    g = math.gcd(src, dst)
    up, down = dst // g, src // g
    return (2 * 32 * max(up, down) + 1) / up


def time_ms(fn, warmup, groups, window_ms):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    steps = max(3, int(math.ceil(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    out = []
    for _ in range(groups):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return statistics.median(out), min(out), max(out), steps


def report(name, shape, rates, nbytes, fmas, ms, lo, hi, steps):
    t_mem, t_fma = nbytes / HBM_BPS * 1e3, 2 * fmas / FP32_FLOPS * 1e3
    bound = max(t_mem, t_fma)
    print(json.dumps({"case": name, "shape": shape, "rates": rates, "bytes": nbytes, "fmas": int(fmas), "ms": round(ms, 4),
                      "ms_min": round(lo, 4), "ms_max": round(hi, 4), "steps_per_window": steps,
                      "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1), "GFMAps": round(fmas / (ms * 1e-3) / 1e9, 1),
                      "bound": "memory" if t_mem >= t_fma else "fp32", "bound_ms": round(bound, 4),
                      "share_of_bound": round(bound / ms, 3)}), flush=True)


def _host_one(x):
    from scipy import signal
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_ref
    return signal.resample_poly(x, 80, 441, window=resample_ref.design(80, 441) / 80)


def _host_one_ref(x):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_ref
    return resample_ref.resample_ref(x, 44100, 8000)[0]


def host_baseline():
    import multiprocessing
    import numpy as np
    try:
        import scipy.signal  # noqa: F401
        fn, what = _host_one, "scipy.signal.resample_poly (float64)"
    except ImportError:
        fn, what = _host_one_ref, "tests/resample_ref.resample_ref (float64 numpy)"
    x = np.random.default_rng(0).uniform(-1, 1, (64, 176400))
    with multiprocessing.Pool(16) as pool:
        pool.map(fn, list(x[:16]))                         # warm the workers
        t0 = time.perf_counter()
        pool.map(fn, list(x))
        dt = time.perf_counter() - t0
    print(json.dumps({"case": "host_baseline", "what": what, "processes": 16, "shape": [64, 176400], "rates": [44100, 8000],
                      "ms": round(dt * 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2,3", help="indices into CASES")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--host-baseline", action="store_true")
    args = ap.parse_args()
    if args.host_baseline:
        return host_baseline()
    import torch
    from audiodenoiser_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for k in (int(v) for v in args.cases.split(",")):
        name, n, length, src, dst = CASES[k]
        g = torch.Generator(device=dev).manual_seed(k)
        x = torch.rand((n, length), generator=g, device=dev) * 2 - 1
        if name == "resample":
            m = ctypes.c_long()
            _lib.check(L.adn_resample_length(length, src, dst, ctypes.byref(m)), "adn_resample_length")
            y = torch.empty((n, m.value), device=dev)
            _lib.check(L.adn_resample_prepare(0, src, dst), "adn_resample_prepare")

            def fn():
                _lib.check(L.adn_resample(x.data_ptr(), n, length, src, dst, y.data_ptr(), st), "adn_resample")
            ms, lo, hi, steps = time_ms(fn, args.warmup, args.groups, args.window_ms)
            report(name, [n, length], [src, dst], 4 * n * (length + m.value), n * m.value * taps_per_output(src, dst), ms, lo, hi, steps)
        else:
            noise = torch.randn((n, length), generator=g, device=dev)
            out = torch.empty_like(x)
            need = ctypes.c_size_t()
            _lib.check(L.adn_mix_snr_workspace_bytes(n, length, ctypes.byref(need)), "adn_mix_snr_workspace_bytes")
            ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=dev)

            def fn():
                _lib.check(L.adn_mix_snr(x.data_ptr(), noise.data_ptr(), n, length, 8.0, ws.data_ptr(), need.value, out.data_ptr(), st),
                           "adn_mix_snr")
            ms, lo, hi, steps = time_ms(fn, args.warmup, args.groups, args.window_ms)
            report(name, [n, length], None, 4 * n * length * 5, 3 * n * length, ms, lo, hi, steps)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
