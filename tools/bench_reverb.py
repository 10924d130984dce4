#!/usr/bin/env python3
"""Device time of the reverb (adn_reverb) through the C ABI, buffers allocated once.  Device events around a window of calls
(at least `--window-ms` long, sized from a calibration run) after a warm-up, median of `--groups` windows.  One JSON line per
case:

    ms                  one launch over the whole batch
    clip_s_per_s        seconds of audio rendered per second (n_clips * length / rate / time)
    chunks              serial steps of the kernel's walk per clip: ceil(length / shortest delay)
    us_per_chunk        ms / chunks: what one step of the walk costs while the batch shares the chip

    python tools/bench_reverb.py                    # the five device cases
    python tools/bench_reverb.py --dataset          # a 256-item all-reverb NoiseMixDataset.load_batch_to_device: wall time of
                                                    # the call, device time of its reverb launch and of its two STFT launches
    python tools/bench_reverb.py --host-baseline    # tests/reverb_ref.py in float32 on one 2 s clip at 8 kHz: an INTERPRETED
                                                    # per-sample Python loop, a scale for the numbers above and not a tuned
                                                    # CPU baseline; no GPU used
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = ((1, 16000, 8000), (16, 16000, 8000), (256, 16000, 8000), (2048, 16000, 8000), (256, 176400, 44100))
PARAMS = (0.9, 0.9, 0.33, 0.4, 1.0)


def host_baseline():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import reverb_ref
    x = np.random.default_rng(0).uniform(-0.5, 0.5, 16000).astype(np.float32)
    t0 = time.perf_counter()
    reverb_ref.reverb_ref(x, 8000, dtype=np.float32)
    dt = time.perf_counter() - t0
    print(json.dumps({"case": "host_baseline", "what": "tests/reverb_ref.reverb_ref (float32, interpreted per-sample loop, one process)",
                      "shape": [1, 16000], "rate": 8000, "ms": round(dt * 1e3, 1), "clip_s_per_s": round(2.0 / dt, 3)}), flush=True)


def dataset_share(args):
    import numpy as np
    import torch
    from bench_resample import time_ms
    from audiodenoiser_amd.data_loader import NoiseMixDataset
    from audiodenoiser_amd.reverb import reverb
    from audiodenoiser_amd.stft import stft_magnitude_fit
    from audiodenoiser_amd.wav import write_wav
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        clean_dir, noise_dir = os.path.join(tmp, "clean"), os.path.join(tmp, "noise")
        os.makedirs(clean_dir)
        os.makedirs(noise_dir)
        rng = np.random.default_rng(0)
        write_wav(os.path.join(clean_dir, "a.wav"), rng.uniform(-0.5, 0.5, 256 * 16000).astype(np.float32), 8000, "FLOAT")
        ds = NoiseMixDataset(clean_dir, noise_dir, noise_types=("reverb",), reverb=True, device=dev)
        idx = list(range(256))
        assert len(ds) == 256
        noisy, clean = ds.audio_batch(idx)                     # decodes and caches the file
        ds.load_batch_to_device(idx)
        torch.cuda.synchronize()
        wall = []
        for _ in range(args.groups):
            t0 = time.perf_counter()
            ds.load_batch_to_device(idx)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        rv, _, _, _ = time_ms(lambda: reverb(clean, 8000), args.warmup, args.groups, args.window_ms)
        st, _, _, _ = time_ms(lambda: (stft_magnitude_fit(noisy, (256, 64), 512, 128, False),
                                       stft_magnitude_fit(clean, (256, 64), 512, 128, False)), args.warmup, args.groups, args.window_ms)
        print(json.dumps({"case": "dataset_256_all_reverb", "wall_ms_load_batch_to_device": round(sorted(wall)[len(wall) // 2], 3),
                          "reverb_launch_ms": round(rv, 4), "two_stft_launches_ms": round(st, 4),
                          "reverb_share_of_device_ms": round(rv / (rv + st), 3),
                          "note": "device ms include torch's output allocation; wall ms include the host-side gather of the chunks"}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2,3,4", help="indices into CASES")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--host-baseline", action="store_true")
    ap.add_argument("--dataset", action="store_true")
    args = ap.parse_args()
    if args.host_baseline:
        return host_baseline()
    if args.dataset:
        return dataset_share(args)
    import torch
    from bench_resample import time_ms
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.reverb import delay_lengths
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for k in (int(v) for v in args.cases.split(",")):
        n, length, rate = CASES[k]
        g = torch.Generator(device=dev).manual_seed(k)
        x = torch.rand((n, length), generator=g, device=dev) - 0.5
        y = torch.empty_like(x)

        def fn():
            _lib.check(L.adn_reverb(x.data_ptr(), n, length, rate, *PARAMS, 1, y.data_ptr(), st), "adn_reverb")
        ms, lo, hi, steps = time_ms(fn, args.warmup, args.groups, args.window_ms)
        chunk = min(sum(delay_lengths(rate), []))
        chunks = -(-length // chunk)
        print(json.dumps({"case": "reverb", "shape": [n, length], "rate": rate, "ms": round(ms, 4), "ms_min": round(lo, 4),
                          "ms_max": round(hi, 4), "steps_per_window": steps,
                          "clip_s_per_s": round(n * length / rate / (ms * 1e-3), 1), "chunks": chunks,
                          "us_per_chunk": round(ms * 1e3 / chunks, 3), "GBps": round(8 * n * length / (ms * 1e-3) / 1e9, 1)}),
              flush=True)
        del x, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
