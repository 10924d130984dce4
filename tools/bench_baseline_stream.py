#!/usr/bin/env python3
"""Device time of the streaming spectral baseline (adn_spectral_gain_windows; SpectralStreamPool): one tick of 1 / 64 / 256 feeds at
block 4 and block 16 (n_fft 512, hop 128, window 16), against the only form the operator had for stream windows before the
kernel: torch gather of the kept columns -> frame-major (m, 0) -> adn_spectral_gain -> scatter back.  Same process, both forms
alternating window by window.

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows (tools/bench_denoise.py's time_ms).  The step that is timed is a steady-state one (step 32) of seeded uniform
audio; calling it again and again reads the same ring samples and writes the same ring rows and tail slot.  The gain's state does
move from call to call (it is a recurrence); its time does not depend on the values.  Before timing, the two forms are compared
on the same windows from the same fresh state: the kept columns and the state must be equal bit for bit.  One JSON line per record:

    tick   per (feeds, block): kernel_ms (spectral_gain_windows in place, rows = (slot, 0): the Python entry point, which builds the
           row table per call), kernel_c_call_ms (adn_spectral_gain_windows itself, the table built once), composed_ms (the torch form),
           analyze_ms, emit_ms, tick_ms (analyse, gain, emit in sequence, through the pool's own methods),
           real_time_factor = feeds x (block hop / sample_rate) / tick

    python tools/bench_baseline_stream.py [--write profiles] [--commit ID]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEP = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feeds", default="1,64,256")
    ap.add_argument("--blocks", default="4,16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--sample-rate", type=int, default=8000)
    ap.add_argument("--write", default=None, help="directory for bench_baseline_stream.jsonl")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import torch
    from audiodenoiser_amd import _lib, build
    from audiodenoiser_amd.baseline import SpectralStreamPool, spectral_gain, spectral_gain_windows
    from bench_denoise import time_ms
    if not torch.cuda.is_available():
        raise SystemExit("bench_baseline_stream: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    records = []
    for block in (int(v) for v in args.blocks.split(",")):
        for n in (int(v) for v in args.feeds.split(",")):
            pool = SpectralStreamPool(dev, max_streams=n, block_frames=block, sample_rate=args.sample_rate)
            book = pool.book
            per, keep, w, f = block * book.hop_length, book.keep, book.window_frames, pool.n_bins
            g = torch.Generator(device=dev).manual_seed(1000 * block + n)
            start = book.end_of(STEP - 1) - keep
            audio = torch.rand((n, keep + per), generator=g, device=dev) - 0.5
            for slot in range(n):
                _lib.check(lib.adn_stream_pool_write(pool._state.data_ptr(), pool._state.numel(), *pool._args, slot,
                                                     audio[slot].data_ptr(), keep + per, start, st), "adn_stream_pool_write")
            rows = [(slot, STEP, -1) for slot in range(n)]
            table = [(slot, False) for slot in range(n)]
            win = pool.analyze(rows)
            col0 = w - block

            def kernel(x=None, state=None):
                x = win if x is None else x
                return spectral_gain_windows(x, pool._gain_state if state is None else state, col0, block, 1, pool.params, table, x)

            ctable = (_lib.SpectralRow * n)(*[_lib.SpectralRow(slot, 0) for slot in range(n)])
            params = ctypes.byref(pool.params.to_struct())

            def kernel_c():                                                  # the C call alone: the table built once
                _lib.check(lib.adn_spectral_gain_windows(win.data_ptr(), win.data_ptr(), n, 1, f, w, col0, block, params,
                                                         pool._gain_state.data_ptr(), n, ctable, st), "adn_spectral_gain_windows")

            cstate = torch.full((n, 3, f), -1.0, device=dev)

            def composed(x=None, state=None):
                x = win if x is None else x
                state = cstate if state is None else state
                m = x[:, 0, :, col0:].permute(0, 2, 1)                       # (n, B, F): frame-major
                out, new = spectral_gain(torch.complex(m, torch.zeros_like(m)), pool.params, state)
                x[:, 0, :, col0:] = out[:, 0]
                state.copy_(new)
                return x

            # the two forms on the same windows from the same fresh state: the same bits
            a, b = win.clone(), win.clone()
            sa, sb = torch.full((n, 3, f), -1.0, device=dev), torch.full((n, 3, f), -1.0, device=dev)
            for _ in range(3):
                kernel(a, sa)
                composed(b, sb)
            same = bool(torch.equal(a, b) and torch.equal(sa, sb))

            y = kernel(win.clone())

            def tick():
                x = pool.analyze(rows)
                return pool.emit(pool._net(x, rows), rows)

            times = time_ms([kernel, composed, lambda: pool.analyze(rows), lambda: pool.emit(y, rows), tick, kernel_c],
                            args.warmup, args.groups, args.window_ms)
            med = [round(t[0], 4) for t in times]
            block_s = per / args.sample_rate
            rec = {"record": "tick", "feeds": n, "block": block, "window": w, "n_bins": f, "waves": n * -(-f // 64),
                   "kernel_ms": med[0], "kernel_ms_min_max": [round(times[0][1], 4), round(times[0][2], 4)],
                   "kernel_c_call_ms": med[5], "kernel_c_call_ms_min_max": [round(times[5][1], 4), round(times[5][2], 4)],
                   "composed_ms": med[1], "composed_ms_min_max": [round(times[1][1], 4), round(times[1][2], 4)],
                   "speedup": round(med[1] / med[0], 2), "same_bits": same,
                   "c_call_us_per_frame": round(med[5] * 1e3 / block, 4),
                   "analyze_ms": med[2], "emit_ms": med[3], "tick_ms": med[4],
                   "tick_ms_min_max": [round(times[4][1], 4), round(times[4][2], 4)],
                   "calls_per_window": [t[3] for t in times], "groups": args.groups, "block_s": block_s,
                   "real_time_factor": round(n * block_s / (med[4] * 1e-3), 1)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del pool, win, y, a, b, audio
            torch.cuda.empty_cache()
    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_baseline_stream.jsonl"), "w") as fh:
            for rec in records:
                fh.write(json.dumps(dict(rec, commit=args.commit, library_digest=digest[:16])) + "\n")


if __name__ == "__main__":
    main()
