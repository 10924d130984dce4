#!/usr/bin/env python3
"""Device time per push of the resampler inside a stream (audiodenoiser_amd.resample.StreamResampler, adn_resample_stream) for a
10 ms block at 48 -> 8, 44.1 -> 8 and 8 -> 48 kHz and 1 / 16 / 256 streams in lockstep, beside what a caller can compose from the
offline pieces: torch.cat([history, block], 1) -> resample -> slice.  The composition is a time baseline only: its edge samples
are not the stream's (the offline resampler zero-extends at both ends of what it is given).

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows, the two forms alternating group by group (tools/bench_denoise.py's time_ms).  One JSON line per record:

    push     per rate pair and n_streams: stream_ms (StreamResampler.push of one block: one launch plus the output allocation),
             call_ms (adn_resample_stream alone into a buffer that exists), composed_ms (cat + resample + slice + the new
             history), and composed_ms / stream_ms
    denoise  StreamDenoiser.push of one step's worth of audio (block 16 x hop 128 samples at 8 kHz = 0.256 s) at 8 kHz and, through
             input_rate=48000, the same 0.256 s as 12 288 samples at 48 kHz: push_ms and the real-time factor of each

    python tools/bench_stream_resample.py [--write profiles] [--commit ID]

Synthetic weights (seed 1234) and uniform noise: times do not depend on the values.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PAIRS = ((48000, 8000), (44100, 8000), (8000, 48000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,256")
    ap.add_argument("--block-ms", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--denoise-streams", default="1,16")
    ap.add_argument("--write", default=None, help="directory for bench_stream_resample.jsonl")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import StreamDenoiser, StreamResampler, _lib, build
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.resample import prepare_resample, resample, resample_stream_plan
    from audiodenoiser_amd.weights import make_state_dict
    from bench_denoise import time_ms
    assert torch.cuda.is_available(), "bench_stream_resample.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for src, dst in PAIRS:
        prepare_resample(src, dst, dev)
        m = int(round(src * args.block_ms * 1e-3))
        _, hist_len, latency = resample_stream_plan(0, src, dst)
        for n in (int(s) for s in args.streams.split(",")):
            g = torch.Generator(device=dev).manual_seed(n)
            block = torch.rand((n, m), generator=g, device=dev) - 0.5
            rs = StreamResampler(src, dst, n_streams=n)
            rs.push(torch.rand((n, 4 * hist_len), generator=g, device=dev) - 0.5)        # a stream in full swing

            def stream_push():
                if rs.received > 1 << 30:
                    rs.reset()
                rs.push(block)

            # the entry point alone: the same steady-state call again and again (it reads slot 0 and writes slot 1)
            need = ctypes.c_size_t()
            lib.adn_resample_stream_state_bytes(n, src, dst, ctypes.byref(need))
            state = torch.zeros(need.value, dtype=torch.uint8, device=dev)
            before = 1000 * m
            n_out = resample_stream_plan(before + m, src, dst)[0] - resample_stream_plan(before, src, dst)[0]
            out = torch.empty((n, n_out), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream

            def call():
                rc = lib.adn_resample_stream(state.data_ptr(), need.value, block.data_ptr(), m, n, 1001, before, m, 0, src, dst,
                                             out.data_ptr(), n_out, stream)
                assert rc == 0, lib.adn_last_error()

            # what the parent commit's pieces allow: carry the history by hand, resample history ++ block, keep the middle
            carried = [torch.rand((n, hist_len), generator=g, device=dev) - 0.5]
            lo = resample_stream_plan(hist_len, src, dst)[0]

            def composed():
                both = torch.cat([carried[0], block], dim=1)
                y = resample(both, src, dst)[:, lo:lo + n_out]
                carried[0] = both[:, -hist_len:]
                return y

            (t_s, s_lo, s_hi, calls), (t_call, *_), (t_c, c_lo, c_hi, _) = time_ms([stream_push, call, composed], args.warmup,
                                                                                  args.groups, args.window_ms)
            emit({"record": "push", "src_rate": src, "dst_rate": dst, "n_streams": n, "block_samples": m, "outputs_per_push": n_out,
                  "history_samples": hist_len, "latency_samples": latency, "stream_ms": round(t_s, 5), "stream_ms_min": round(s_lo, 5),
                  "stream_ms_max": round(s_hi, 5), "call_ms": round(t_call, 5), "composed_ms": round(t_c, 5),
                  "composed_ms_min": round(c_lo, 5), "composed_ms_max": round(c_hi, 5), "composed_over_stream": round(t_c / t_s, 2),
                  "calls_per_window": calls})
            del rs, state, out, block
    weights = make_state_dict(1234)
    net = UNet(1, 1)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in weights.items()}, strict=True)
    net = net.to(dev).eval()
    for n in (int(s) for s in args.denoise_streams.split(",")):
        g = torch.Generator(device=dev).manual_seed(100 + n)
        fns, meta = [], []
        for rate in (8000, 48000):
            sd = StreamDenoiser(net, n_streams=n, input_rate=rate)
            per = sd.block_frames * sd.hop_length * rate // sd.sample_rate             # one step's worth of audio at `rate`
            block = torch.rand((n, per), generator=g, device=dev) - 0.5
            sd.push(torch.rand((n, sd.latency_input_samples + 40 * per), generator=g, device=dev) - 0.5)
            fns.append(lambda sd=sd, block=block: sd.push(block))
            meta.append((rate, per, sd.latency_input_samples))
        for (rate, per, lat), (t, lo, hi, calls) in zip(meta, time_ms(fns, 2, args.groups, args.window_ms)):
            emit({"record": "denoise", "input_rate": rate, "n_streams": n, "block_samples": per, "block_s": per / rate,
                  "push_ms": round(t, 4), "push_ms_min": round(lo, 4), "push_ms_max": round(hi, 4), "calls_per_window": calls,
                  "realtime_factor": round(per / rate / (t * 1e-3), 1), "latency_input_samples": lat})
        net._workspace = None
        torch.cuda.empty_cache()
    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_stream_resample.jsonl"), "w") as fh:
            for rec in records:
                fh.write(json.dumps(dict(rec, commit=args.commit, library_digest=digest[:16])) + "\n")


if __name__ == "__main__":
    main()
