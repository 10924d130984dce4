#!/usr/bin/env python3
"""Device time of one tick of StreamPool (audiodenoiser_amd/stream.py) for 1 / 4 / 16 / 64 / 256 ready streams at the defaults (n_fft
512, hop 128, window 192, block 16, look-ahead 0), against what a caller had before the pool: the same number of
StreamDenoiser(n_streams=1) objects, each running one step.  Same process, same model.

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows, as tools/bench_stream.py.  The step that is timed is a steady-state one (step 32: every frame of its window
exists); calling it again and again reads the same ring samples and writes the same ring rows and tail slot, so the state stays
what it was.  Each time is split into analysis / U-Net / emit; `tick` is the three in sequence (for the pool: adn_stream_pool_analyze,
the U-Net over `batch_windows` windows at a time, adn_stream_pool_emit; per group of 256 rows).  One JSON line per record:

    tick   per n_streams and dtype: pool {analyze_ms, unet_ms, emit_ms, tick_ms}, separate {...} (n objects, one step each),
           speedup = separate tick / pool tick, feeds = n_streams * (block * hop / sample_rate) / tick: the live feeds one card
           carries in real time

    python tools/bench_stream_pool.py [--write profiles] [--commit ID]

Synthetic weights (seed 1234): times do not depend on the weights' values.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEP = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16,64,256")
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--sample-rate", type=int, default=8000, help="the network's working rate (for the feeds-per-card figure)")
    ap.add_argument("--write", default=None, help="directory for bench_stream_pool.jsonl")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import StreamDenoiser, StreamPool, _lib, build
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.weights import make_state_dict
    from bench_denoise import time_ms
    assert torch.cuda.is_available(), "bench_stream_pool.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    weights = make_state_dict(1234)
    records = []
    lib = _lib.load()

    for dtype in args.dtypes.split(","):
        net = UNet(1, 1)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights.items()}, strict=True)
        net = net.to(dev).eval().set_compute_dtype(dtype)
        for n in (int(s) for s in args.streams.split(",")):
            pool = StreamPool(net, max_streams=n)
            book = pool.book
            per, keep = book.block_frames * book.hop_length, book.keep
            g = torch.Generator(device=dev).manual_seed(n)
            # what step 32 of every stream reads: the block it brings and the n_fft - hop samples before it, at their ring positions
            start = book.end_of(STEP - 1) - keep
            audio = torch.rand((n, keep + per), generator=g, device=dev) - 0.5
            st = torch.cuda.current_stream(dev).cuda_stream
            for slot in range(n):
                _lib.check(lib.adn_stream_pool_write(pool._state.data_ptr(), pool._state.numel(), *pool._args, slot,
                                                     audio[slot].data_ptr(), keep + per, start, st), "adn_stream_pool_write")
            rows = [(slot, STEP, -1) for slot in range(n)]
            groups = [rows[i:i + 256] for i in range(0, n, 256)]

            def p_analyze():
                return torch.cat([pool.analyze(r) for r in groups]) if len(groups) > 1 else pool.analyze(rows)

            def p_emit(y):
                return [pool.emit(y[i * 256:i * 256 + len(r)], r) for i, r in enumerate(groups)]

            win = p_analyze()
            y = pool.network(win)

            # the baseline: n objects of one stream each, the same step of the same audio
            sds = [StreamDenoiser(net, n_streams=1) for _ in range(n)]
            blocks = [audio[i:i + 1, keep:] for i in range(n)]
            wins = [sd.analyze(b, per, STEP, 1) for sd, b in zip(sds, blocks)]
            ys = [sd.network(w) for sd, w in zip(sds, wins)]

            def s_analyze():
                return [sd.analyze(b, per, STEP, 1) for sd, b in zip(sds, blocks)]

            def s_unet():
                return [sd.network(w) for sd, w in zip(sds, wins)]

            def s_emit():
                return [sd.emit(v, STEP, 1) for sd, v in zip(sds, ys)]

            def s_tick():
                return [sd.emit(sd.network(sd.analyze(b, per, STEP, 1)), STEP, 1) for sd, b in zip(sds, blocks)]

            times = time_ms([p_analyze, lambda: pool.network(win), lambda: p_emit(y), lambda: p_emit(pool.network(p_analyze())),
                             s_analyze, s_unet, s_emit, s_tick], args.warmup, args.groups, args.window_ms)
            med = [round(t[0], 4) for t in times]
            block_s = per / args.sample_rate
            rec = {"record": "tick", "dtype": dtype, "n_streams": n, "block_s": block_s,
                   "pool": dict(zip(("analyze_ms", "unet_ms", "emit_ms", "tick_ms"), med[:4])),
                   "separate": dict(zip(("analyze_ms", "unet_ms", "emit_ms", "tick_ms"), med[4:])),
                   "pool_tick_ms_min_max": [round(times[3][1], 4), round(times[3][2], 4)],
                   "separate_tick_ms_min_max": [round(times[7][1], 4), round(times[7][2], 4)],
                   "calls_per_window": [times[3][3], times[7][3]],
                   "speedup": round(med[7] / med[3], 2),
                   "feeds_pool": int(n * block_s / (med[3] * 1e-3)), "feeds_separate": int(n * block_s / (med[7] * 1e-3))}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del pool, sds, blocks, wins, ys, win, y, audio
            net._workspace = None
            torch.cuda.empty_cache()
    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_stream_pool.jsonl"), "w") as fh:
            for rec in records:
                fh.write(json.dumps(dict(rec, commit=args.commit, library_digest=digest[:16])) + "\n")


if __name__ == "__main__":
    main()
