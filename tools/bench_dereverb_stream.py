#!/usr/bin/env python3
"""Device time of the streaming dereverberator (adn_wpe_stream_pool; DereverbStreamPool): one step of 1 / 64 / 256 feeds at block 4
(n_fft 512, hop 128, window 16, the default parameters), against its state-traffic bound and against the same step composed from
torch ops batched over (feed, bin); the whole tick (analyse, WPE, emit) through the pool's own methods; SI-SDR of
StreamDereverberator on tests/dereverb_cases.py's clip.

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows (tools/bench_denoise.py's time_ms).  The step that is timed is a steady-state one (step 32) of seeded uniform
audio; calling it again and again reads the same ring rows.  The WPE state and the ring rows it rewrites do move from call to call
(it is a recursion, and d goes back in place); its time does not depend on the values.  Before timing, the torch form and
adn_wpe_online are compared on the same 40 frames from a fresh start: the largest difference relative to the largest |d| is
reported (two float32 evaluations of one recursion: a floor of its own, not a bound).  One JSON line per record:

    step    per feeds: c_call_ms (adn_wpe_stream_pool itself, the row table built once), state_bytes (read + written),
            state_bound_ms (those bytes at 8 TB/s), share_of_bound, composed_ms (the torch form of the same block of frames),
            analyze_ms, emit_ms, tick_ms, real_time_factor = feeds x (block hop / sample_rate) / tick
    si_sdr  reverberant input, the stream, the stream with the gain, on the device (metrics.evaluate) and from the restatement

    python tools/bench_dereverb_stream.py [--write profiles] [--commit ID]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_common import write_marked_block  # noqa: E402

STEP = 32
HBM_BPS = 8.0e12


class TorchRls:
    """The recursion of adn.h ("dereverb stream") from torch ops, batched over rows (feed x bin): state g (R, K), P (R, K, K),
    s (R,), past (R, D + K - 1)."""

    def __init__(self, rows, params, dev):
        import torch
        self.K, self.D = params.taps, params.delay
        self.alpha, self.rho, self.beta = params.forget, params.power_floor, params.smooth
        self.g = torch.zeros((rows, self.K), dtype=torch.complex64, device=dev)
        self.P = torch.eye(self.K, dtype=torch.complex64, device=dev).repeat(rows, 1, 1) / params.loading
        self.s = torch.zeros(rows, device=dev)
        self.past = torch.zeros((rows, self.D + self.K - 1), dtype=torch.complex64, device=dev)
        self.low = torch.tril(torch.ones((self.K, self.K), dtype=torch.bool, device=dev))
        self.first = True

    def block(self, x):
        """x (R, B) complex64, the next B frames of every row -> d (R, B)."""
        import torch
        out = torch.empty_like(x)
        for t in range(x.shape[1]):
            xt = x[:, t]
            p = xt.real * xt.real + xt.imag * xt.imag
            self.s = p if self.first else self.beta * self.s + (1.0 - self.beta) * p
            self.first = False
            phi = torch.clamp(self.rho * self.s, min=1e-30)
            taps = self.past[:, :self.K].flip(1)                 # past is X_{t-D-K+1} ... X_{t-1}: column j = X_{t-D-j}
            e = xt - (self.g.conj() * taps).sum(1)
            lam = torch.maximum(e.real * e.real + e.imag * e.imag, phi)
            u = torch.einsum("rjk,rk->rj", self.P, taps)
            den = self.alpha * lam + (taps.conj() * u).sum(1).real
            k = u / den[:, None]
            Pn = (self.P - k[:, :, None] * u.conj()[:, None, :]) / self.alpha
            Pn = torch.where(self.low, Pn, Pn.transpose(1, 2).conj())
            d = torch.diagonal(Pn, dim1=1, dim2=2)
            d.copy_(torch.complex(d.real, torch.zeros_like(d.real)))
            self.P = Pn
            self.g = self.g + k * e.conj()[:, None]
            self.past = torch.cat([self.past[:, 1:], xt[:, None]], dim=1)
            out[:, t] = e
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feeds", default="1,64,256")
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--sample-rate", type=int, default=8000)
    ap.add_argument("--write", default=None, help="directory for bench_dereverb_stream.jsonl and the device block of bench_dereverb_stream.md")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import _lib, build
    from audiodenoiser_amd.dereverb import (DereverbStreamPool, StreamDereverberator, WpeStreamParams, wpe_online,
                                            wpe_stream_state_bytes)
    from audiodenoiser_amd.metrics import evaluate
    from bench_denoise import time_ms
    import dereverb_cases as dc
    import dereverb_stream_cases as sc
    if not torch.cuda.is_available():
        raise SystemExit("bench_dereverb_stream: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    records = []
    block = args.block
    defaults = WpeStreamParams()

    # the torch form against adn_wpe_online: 40 frames of three rows from a fresh start
    from audiodenoiser_amd.griffin_lim import stft_complex
    spec = stft_complex(torch.from_numpy(sc.parity_audio(512, 40).copy()).to(dev), 512, 128)
    d_dev, _, _ = wpe_online(spec)
    rls = TorchRls(3 * 257, defaults, dev)
    d_torch = rls.block(spec.permute(0, 2, 1).reshape(3 * 257, 40)).reshape(3, 257, 40).permute(0, 2, 1)
    composed_diff = float((d_torch - d_dev).abs().max() / d_dev.abs().max())

    for n in (int(v) for v in args.feeds.split(",")):
        pool = DereverbStreamPool(dev, max_streams=n, block_frames=block, sample_rate=args.sample_rate)
        book = pool.book
        per, keep, w, f = block * book.hop_length, book.keep, book.window_frames, pool.n_bins
        g = torch.Generator(device=dev).manual_seed(1000 * block + n)
        start = book.end_of(STEP - 1) - keep
        audio = torch.rand((n, keep + per), generator=g, device=dev) - 0.5
        for slot in range(n):
            _lib.check(lib.adn_stream_pool_write(pool._state.data_ptr(), pool._state.numel(), *pool._args, slot,
                                                 audio[slot].data_ptr(), keep + per, start, st), "adn_stream_pool_write")
        rows = [(slot, STEP, -1) for slot in range(n)]
        pool._wpe_state.zero_()                                  # step 32 continues a row: a defined state to continue from
        win = pool.analyze(rows)
        ctable = pool._rows(rows)
        params = ctypes.byref(pool.params.to_struct())

        def kernel_c():                                          # the C call alone: the table built once
            _lib.check(lib.adn_wpe_stream_pool(pool._state.data_ptr(), pool._state.numel(), *pool._args, ctable, n, win.data_ptr(),
                                               params, pool._wpe_state.data_ptr(), pool._wpe_state.numel(), st), "adn_wpe_stream_pool")

        rls = TorchRls(n * f, defaults, dev)
        frames = (torch.rand((n * f, block), generator=g, device=dev) - 0.5).to(torch.complex64)

        def composed():
            return rls.block(frames)

        y = win.clone()

        def tick():
            x = pool.analyze(rows)
            return pool.emit(pool._net(x, rows), rows)

        times = time_ms([kernel_c, composed, lambda: pool.analyze(rows), lambda: pool.emit(y, rows), tick],
                        args.warmup, args.groups, args.window_ms)
        med = [round(t[0], 4) for t in times]
        block_s = per / args.sample_rate
        state_bytes = 2 * wpe_stream_state_bytes(n, f)
        bound_ms = state_bytes / HBM_BPS * 1e3
        rec = {"record": "step", "feeds": n, "block": block, "window": w, "n_bins": f, "workgroups": n * -(-f // 8),
               "c_call_ms": med[0], "c_call_ms_min_max": [round(times[0][1], 4), round(times[0][2], 4)],
               "state_bytes": state_bytes, "state_bound_ms": round(bound_ms, 5), "share_of_bound": round(bound_ms / med[0], 4),
               "composed_ms": med[1], "composed_ms_min_max": [round(times[1][1], 4), round(times[1][2], 4)],
               "composed_over_c_call": round(med[1] / med[0], 1), "composed_max_rel_diff": composed_diff,
               "analyze_ms": med[2], "emit_ms": med[3], "tick_ms": med[4],
               "tick_ms_min_max": [round(times[4][1], 4), round(times[4][2], 4)],
               "calls_per_window": [t[3] for t in times], "groups": args.groups, "block_s": block_s,
               "real_time_factor": round(n * block_s / (med[4] * 1e-3), 1)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del pool, win, y, audio, rls, frames
        torch.cuda.empty_cache()

    wet, dry = dc.quality_case()
    wd, dd = torch.from_numpy(wet.copy()).to(dev)[None], torch.from_numpy(dry.copy()).to(dev)

    def live(gain):
        sd = StreamDereverberator(dev, gain=gain)
        outs = [sd.push(wd[:, i:i + 1024]) for i in range(0, wd.shape[1], 1024)]
        outs.append(sd.flush())
        return float(evaluate(torch.cat(outs, dim=1)[0], dd, sr=args.sample_rate)["si_sdr"][0])

    r_in, r_stream, r_gain, r_offline = sc.restatement_si_sdr()
    rec = {"record": "si_sdr", "input": round(float(evaluate(wd[0], dd, sr=args.sample_rate)["si_sdr"][0]), 3), "stream": round(live(False), 3),
           "stream_gain": round(live(True), 3), "restatement": [round(v, 3) for v in (r_in, r_stream, r_gain, r_offline)]}
    records.append(rec)
    print(json.dumps(rec), flush=True)

    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_dereverb_stream.jsonl"), "w") as fh:
            for r in records:
                fh.write(json.dumps(dict(r, commit=args.commit, library_digest=digest[:16])) + "\n")
        steps = [r for r in records if r["record"] == "step"]
        head = "| measurement | " + " | ".join(f"{r['feeds']} feed{'s' if r['feeds'] > 1 else ''}" for r in steps) + " |\n"
        head += "|---|" + "---|" * len(steps) + "\n"

        def line(name, fn):
            return f"| {name} | " + " | ".join(fn(r) for r in steps) + " |\n"

        text = (f"Written by `tools/bench_dereverb_stream.py` on one MI355X (device events, windows after a warm-up, median of "
                f"{args.groups}); K 20, D 3, n_fft 512, hop 128, block {block}: one step is {block} frames of every feed.\n\n" + head
                + line("`adn_wpe_stream_pool` (1 launch)", lambda r: f"{r['c_call_ms']:.4f} ms")
                + line("workgroups", lambda r: str(r["workgroups"]))
                + line("state read + written", lambda r: f"{r['state_bytes'] / 1e6:.2f} MB")
                + line("its bound at 8 TB/s; share of it", lambda r: f"{r['state_bound_ms']:.5f} ms; {r['share_of_bound']:.3f}")
                + line("the same block of frames from torch ops", lambda r: f"{r['composed_ms']:.3f} ms ({r['composed_over_c_call']} x)")
                + line("analyse / emit", lambda r: f"{r['analyze_ms']:.4f} / {r['emit_ms']:.4f} ms")
                + line("whole tick (analyse, WPE, emit; host included)", lambda r: f"{r['tick_ms']:.4f} ms = {r['real_time_factor']} x real time")
                + f"\nTorch form against `adn_wpe_online`, 40 frames from a fresh start, largest difference over the largest |d|: "
                  f"{composed_diff:.3g}.\n\n"
                  "SI-SDR against the dry signal on the device (`metrics.evaluate`), `StreamDereverberator` fed 1024 samples at a time, "
                  "the clip of the host block:\n\n| path | device | float64 restatement |\n|---|---|---|\n"
                  f"| reverberant input | {rec['input']:.3f} dB | {r_in:.3f} dB |\n| stream | {rec['stream']:.3f} dB | {r_stream:.3f} dB |\n"
                  f"| stream, then the spectral gain | {rec['stream_gain']:.3f} dB | {r_gain:.3f} dB |\n")
        write_marked_block(os.path.join(args.write, "bench_dereverb_stream.md"), text)


if __name__ == "__main__":
    main()
