#!/usr/bin/env python3
"""Device time of the multi-reference echo canceller (adn_aec_mr_stream, adn_aec_mr_online of include/adn_call.h).

    step    one adn_aec_mr_stream step of `--block` frames for 1 / 64 / 256 groups at refs x taps 2 x 8, 4 x 4 and 2 x 16 (n_fft 512,
            hop 128, the other parameters the defaults; forget 0.985 at N = 32), beside two yardsticks from the same build:
            adn_aec_stream at taps = N on the same number of rows -- the same P, the same chain length, code unchanged from the
            parent commit (tools/kernel_isa_digest.py) -- and the same block of frames from torch ops; the state-traffic bound
            (8 N^2 + 16 N + 8 Q D bytes per row and direction at 8 TB/s) and the FMA bound (8 N^2 + 12 N fp32 FMAs per row-frame at
            78.6 T FMA/s) with the share of each
    hour    one hour of 8 kHz audio (60 rows of 60 s, two references) through adn_aec_mr_online at the default 2 x 8, beside
            adn_aec_online at taps 16 on the same rows

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up: the median,
the least and the most of `--groups` windows (tools/bench_common.py), as tools/bench_echo.py measures.  The step that is timed is a
steady-state one (the last step the object ran) of seeded uniform audio.  One JSON line per record.

    python tools/bench_echo_mr.py [--write profiles] [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import time_ms, write_marked_block  # noqa: E402

HBM_BPS = 8.0e12
FMA_PER_S = 157.3e12 / 2


class TorchMrRls:
    """The recursion of adn_call.h ("echo stream multireference") from torch ops, batched over rows (group x bin)."""

    def __init__(self, rows, refs, params, dev):
        import torch
        self.Q, self.K, self.D, self.alpha, self.quiet = refs, params.taps, params.delay, params.forget, params.quiet
        n = refs * self.K
        self.h = torch.zeros((rows, n), dtype=torch.complex64, device=dev)
        self.P = torch.eye(n, dtype=torch.complex64, device=dev).repeat(rows, 1, 1) / params.loading
        self.past = torch.zeros((rows, refs, self.D + self.K), dtype=torch.complex64, device=dev)     # R_{t-D-K+1} ... R_t per channel
        self.low = torch.tril(torch.ones((n, n), dtype=torch.bool, device=dev))

    def block(self, y, r):
        """y (R, B), r (R, Q, B) complex64, the next B frames of every row -> e (R, B)."""
        import torch
        out = torch.empty_like(y)
        for t in range(y.shape[1]):
            self.past = torch.cat([self.past[:, :, 1:], r[:, :, t:t + 1]], dim=2)
            taps = self.past[:, :, :self.K].flip(2).reshape(y.shape[0], -1)      # column q K + j = R_{t-D-j, q}
            e = y[:, t] - (self.h.conj() * taps).sum(1)
            adapt = ~((taps.real ** 2 + taps.imag ** 2).sum(1) <= self.quiet)
            u = torch.einsum("rjk,rk->rj", self.P, taps)
            k = u / (self.alpha + (taps.conj() * u).sum(1).real)[:, None]
            Pn = (self.P - k[:, :, None] * u.conj()[:, None, :]) / self.alpha
            Pn = torch.where(self.low, Pn, Pn.transpose(1, 2).conj())
            d = torch.diagonal(Pn, dim1=1, dim2=2)
            d.copy_(torch.complex(d.real, torch.zeros_like(d.real)))
            self.P = torch.where(adapt[:, None, None], Pn, self.P)
            self.h = torch.where(adapt[:, None], self.h + k * e.conj()[:, None], self.h)
            out[:, t] = e
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups-of", default="1,64,256", help="groups (one microphone and its references) per step")
    ap.add_argument("--shapes", default="2x8,4x4,2x16", help="refs x taps")
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--no-hour", action="store_true")
    ap.add_argument("--write", default=None, help="directory for bench_echo_mr.jsonl and the device block of bench_echo_mr.md")
    ap.add_argument("--commit", default=None, help="recorded with every line when given")
    args = ap.parse_args()
    import torch
    from audiodenoiser_amd import build
    from audiodenoiser_amd.echo import AecParams, StreamEchoCanceller, aec_mr_online, aec_mr_state_bytes, aec_online
    from audiodenoiser_amd.griffin_lim import stft_complex
    if not torch.cuda.is_available():
        raise SystemExit("bench_echo_mr: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    records, block, f = [], args.block, 257
    steps = 8
    length = steps * block * 128                                     # `steps` whole steps and the look of a running stream
    timing = (args.warmup, args.groups, args.window_ms)

    for refs, taps in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        n_stack = refs * taps
        forget = AecParams.forget if n_stack <= 16 else 0.985
        p, parent = AecParams(taps=taps, forget=forget), AecParams(taps=n_stack, forget=forget)
        for n in (int(v) for v in args.groups_of.split(",")):
            g = torch.Generator(device=dev).manual_seed(1000 * n_stack + 10 * refs + n)
            se = StreamEchoCanceller(dev, pairs=n, refs=refs, block_frames=block, params=p)
            se.push(torch.rand(((refs + 1) * n, length), generator=g, device=dev) - 0.5)
            last = se._done - 1
            assert last >= 1
            win = torch.zeros(((refs + 1) * n, 1, f, se.window_frames), device=dev)
            sp = StreamEchoCanceller(dev, pairs=n, block_frames=block, params=parent)
            sp.push(torch.rand((2 * n, length), generator=g, device=dev) - 0.5)
            pwin = torch.zeros((2 * n, 1, f, sp.window_frames), device=dev)
            rls = TorchMrRls(n * f, refs, p, dev)
            y = (torch.rand((n * f, block), generator=g, device=dev) - 0.5).to(torch.complex64)
            r = (torch.rand((n * f, refs, block), generator=g, device=dev) - 0.5).to(torch.complex64)
            t_mr = time_ms(lambda: se._cancel(win, last, 1), *timing)
            t_parent = time_ms(lambda: sp._cancel(pwin, sp._done - 1, 1), *timing)
            t_again = time_ms(lambda: sp._cancel(pwin, sp._done - 1, 1), *timing)      # the yardstick's own run-to-run spread
            t_torch = time_ms(lambda: rls.block(y, r), *timing)
            state_bytes = 2 * aec_mr_state_bytes(n, f, refs, p)
            bound_ms = state_bytes / HBM_BPS * 1e3
            fma_ms = n * f * block * (8 * n_stack * n_stack + 12 * n_stack) / FMA_PER_S * 1e3
            lanes = 8 if n_stack <= 8 else 16 if n_stack <= 16 else 32
            rec = {"record": "step", "refs": refs, "taps": taps, "stacked": n_stack, "forget": forget, "groups": n, "block": block,
                   "lanes_per_row": lanes, "workgroups": n * -(-f // (256 // lanes)), "aec_mr_stream": t_mr,
                   "aec_stream_taps_n_same_rows": t_parent, "aec_stream_again": t_again,
                   "mr_over_parent": round(t_mr["ms"] / t_parent["ms"], 3),
                   "parent_spread": round(max(t_parent["ms_max"], t_again["ms_max"]) / min(t_parent["ms_min"], t_again["ms_min"]), 3),
                   "torch_ops": t_torch, "torch_over_mr": round(t_torch["ms"] / t_mr["ms"], 1), "state_bytes": state_bytes,
                   "state_bound_ms": round(bound_ms, 6), "share_of_state_bound": round(bound_ms / t_mr["ms"], 4),
                   "fma_bound_ms": round(fma_ms, 6), "share_of_fma_bound": round(fma_ms / t_mr["ms"], 4)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del se, sp, rls, win, pwin, y, r
            torch.cuda.empty_cache()

    if not args.no_hour:
        rows, seconds, refs = 60, 60, 2
        g = torch.Generator(device=dev).manual_seed(7)
        mic = torch.rand((rows, seconds * 8000), generator=g, device=dev) - 0.5
        far = torch.rand((rows * refs, seconds * 8000), generator=g, device=dev) - 0.5
        ms, fs = stft_complex(mic, 512, 128), stft_complex(far, 512, 128)
        fs = fs.view(rows, refs, *fs.shape[1:])
        one, wide = fs[:, 0].contiguous(), AecParams(taps=16)
        hour = (args.warmup, args.groups, 1.0)
        t_mr = time_ms(lambda: aec_mr_online(ms, fs, refs), *hour)
        t_parent = time_ms(lambda: aec_online(ms, one, params=wide), *hour)
        rec = {"record": "hour", "rows": rows, "seconds": seconds, "refs": refs, "frames": int(ms.shape[1]), "aec_mr_online": t_mr,
               "aec_online_taps_16": t_parent, "mr_over_parent": round(t_mr["ms"] / t_parent["ms"], 3),
               "real_time_factor": round(rows * seconds / (t_mr["ms"] * 1e-3), 0)}
        records.append(rec)
        print(json.dumps(rec), flush=True)

    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_echo_mr.jsonl"), "w") as fh:
            for r in records:
                fh.write(json.dumps(dict(r, library_digest=digest[:16], **({"commit": args.commit} if args.commit else {}))) + "\n")
        text = (f"Written by `tools/bench_echo_mr.py` on one MI355X (device events, windows after a warm-up, median [least, most] of "
                f"{args.groups}); n_fft 512, hop 128, block {block}: one step is {block} frames of every group.\n\n"
                "| refs x taps | groups | lanes | `adn_aec_mr_stream` | `adn_aec_stream`, taps = N, same rows | ratio | the yardstick's own most / least | torch ops | state bound; share | FMA bound; share |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        span = lambda t: f"{t['ms']:.4f} [{t['ms_min']:.4f}, {t['ms_max']:.4f}] ms"  # noqa: E731
        for r in records:
            if r["record"] == "step":
                text += (f"| {r['refs']} x {r['taps']} | {r['groups']} | {r['lanes_per_row']} | {span(r['aec_mr_stream'])} | "
                         f"{span(r['aec_stream_taps_n_same_rows'])} | {r['mr_over_parent']:.2f} | {r['parent_spread']:.2f} | "
                         f"{r['torch_ops']['ms']:.2f} ms ({r['torch_over_mr']} x) | {r['state_bound_ms']:.5f} ms; "
                         f"{r['share_of_state_bound']:.3f} | {r['fma_bound_ms']:.5f} ms; {r['share_of_fma_bound']:.3f} |\n")
        for r in records:
            if r["record"] == "hour":
                text += (f"\nOne hour of 8 kHz audio with {r['refs']} references ({r['rows']} rows of {r['seconds']} s, {r['frames']} frames "
                         f"each): `adn_aec_mr_online` at the default 2 x 8 {span(r['aec_mr_online'])}, {r['real_time_factor']:.0f} x real "
                         f"time; `adn_aec_online` at taps 16 on the same rows {span(r['aec_online_taps_16'])}, ratio {r['mr_over_parent']:.2f}.\n")
        write_marked_block(os.path.join(args.write, "bench_echo_mr.md"), text)


if __name__ == "__main__":
    main()
