#!/usr/bin/env python3
"""Device time of one step of the streaming denoiser (audiodenoiser_amd/stream.py) for 1 / 16 / 64 / 256 streams in lockstep at the
defaults (n_fft 512, hop 128, window 192, block 16, look-ahead 0): analysis (adn_stream_analyze, two launches), U-Net, emit
(adn_stream_emit), and StreamDenoiser.push of one block (the three plus the pending-buffer copies and the allocations).

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows, as tools/bench_denoise.py.  The step that is timed is a steady-state one (step 32: every frame of its window
exists); calling it again and again writes the same ring rows and slots, so the state stays what it was.  One JSON line per record:

    step     per n_streams and dtype: analyze_ms, unet_ms, emit_ms, push_ms; realtime_factor = (block * hop / sample_rate) /
             push_ms; streams_at_factor_1 = n_streams * realtime_factor
    kernels  per n_streams: the bytes the analysis and the emit must move, their bounds at 8 TB/s and at the 6.3 TB/s
             profiles/NOTES.md calls achievable, and the share of the 8 TB/s bound they reach
               analysis: new samples in; X and |X| of the B new frames out; |X| of W frames in, the network input out
               emit:     B frames of y and of X in, the carried tail in and out, B * hop samples out
    offline  the same seconds of audio through Denoiser.denoise (a finished recording, for scale)

    python tools/bench_stream.py [--write profiles] [--commit ID]

Synthetic weights (seed 1234): times do not depend on the weights' values.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_BPS, HBM_ACHIEVABLE_BPS = 8.0e12, 6.3e12
STEP = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,64,256")
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--offline-seconds", type=float, default=60.0, help="audio per stream of the offline comparison")
    ap.add_argument("--write", default=None, help="directory for bench_stream.jsonl")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import Denoiser, StreamDenoiser, build
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.weights import make_state_dict
    from bench_denoise import time_ms
    assert torch.cuda.is_available(), "bench_stream.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    weights = make_state_dict(1234)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    first_dtype = args.dtypes.split(",")[0]
    for dtype in args.dtypes.split(","):
        net = UNet(1, 1)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights.items()}, strict=True)
        net = net.to(dev).eval().set_compute_dtype(dtype)
        for n in (int(s) for s in args.streams.split(",")):
            sd = StreamDenoiser(net, n_streams=n)
            per = sd.block_frames * sd.hop_length                     # samples a step brings
            f, w, b, keep = sd.n_bins, sd.window_frames, sd.block_frames, sd.n_fft - sd.hop_length
            g = torch.Generator(device=dev).manual_seed(n)
            block = torch.rand((n, per), generator=g, device=dev) - 0.5
            win = sd.analyze(block, per, STEP, 1)
            y = sd.network(win)

            live = StreamDenoiser(net, n_streams=n)                   # push runs on a stream of its own, in full swing

            def push():
                live.push(block)

            live.push(torch.rand((n, sd.latency_samples + 40 * per), generator=g, device=dev) - 0.5)     # a stream in full swing
            (t_an, *_), (t_net, *_), (t_em, *_), (t_push, lo, hi, calls) = time_ms(
                [lambda: sd.analyze(block, per, STEP, 1), lambda: sd.network(win), lambda: sd.emit(y, STEP, 1), push],
                args.warmup, args.groups, args.window_ms)
            sd.reset()
            rtf = per / sd.sample_rate / (t_push * 1e-3)
            emit({"record": "step", "dtype": dtype, "n_streams": n, "analyze_ms": round(t_an, 4), "unet_ms": round(t_net, 4),
                  "emit_ms": round(t_em, 4), "push_ms": round(t_push, 4), "push_ms_min": round(lo, 4), "push_ms_max": round(hi, 4),
                  "calls_per_window": calls, "block_s": per / sd.sample_rate, "realtime_factor": round(rtf, 1),
                  "streams_at_factor_1": int(n * rtf), "latency_samples": sd.latency_samples})
            if dtype == first_dtype:                                  # the two kernels do not depend on the model's dtype
                an_bytes = n * 4 * (per + 3 * b * f + 2 * w * f)
                em_bytes = n * 4 * (b * f + 2 * b * f + 2 * keep + per)
                emit({"record": "kernels", "n_streams": n,
                      "analyze_bytes": an_bytes, "analyze_ms": round(t_an, 4), "analyze_bound_ms_8TBps": round(an_bytes / HBM_BPS * 1e3, 5),
                      "analyze_bound_ms_6p3TBps": round(an_bytes / HBM_ACHIEVABLE_BPS * 1e3, 5),
                      "analyze_share_of_8TBps": round(an_bytes / HBM_BPS * 1e3 / t_an, 4),
                      "emit_bytes": em_bytes, "emit_ms": round(t_em, 4), "emit_bound_ms_8TBps": round(em_bytes / HBM_BPS * 1e3, 5),
                      "emit_bound_ms_6p3TBps": round(em_bytes / HBM_ACHIEVABLE_BPS * 1e3, 5),
                      "emit_share_of_8TBps": round(em_bytes / HBM_BPS * 1e3 / t_em, 4)})
            length = int(args.offline_seconds * sd.sample_rate)
            x = torch.rand((n, length), generator=g, device=dev) - 0.5
            dn = Denoiser(net)
            ((t_off, *_),) = time_ms([lambda: dn.denoise(x)], 1, 3, args.window_ms)
            emit({"record": "offline", "dtype": dtype, "n_streams": n, "seconds_per_stream": args.offline_seconds, "denoise_ms": round(t_off, 3),
                  "ms_per_block_of_audio": round(t_off / (length / per), 4), "audio_s_per_s": round(n * args.offline_seconds / (t_off * 1e-3), 1)})
            del sd, live, dn, x, win, y, block
            net._workspace = None
            torch.cuda.empty_cache()
    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_stream.jsonl"), "w") as fh:
            for rec in records:
                fh.write(json.dumps(dict(rec, commit=args.commit, library_digest=digest[:16])) + "\n")


if __name__ == "__main__":
    main()
