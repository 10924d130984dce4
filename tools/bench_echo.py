#!/usr/bin/env python3
"""Device time of the echo canceller (adn_aec_stream, adn_aec_online; StreamEchoCanceller, EchoCanceller).

    step    one adn_aec_stream step of `--block` frames for 1 / 64 / 256 pairs at taps 8 / 16 / 32 (n_fft 512, hop 128, the other
            parameters the defaults; forget 0.985 at taps 32, the lowest its window rule allows is 0.984375), beside adn_wpe_stream at
            the same taps on the same number of rows -- the only comparable kernel -- and beside the same block of frames from
            torch ops; the state-traffic bound (8 K^2 + 16 K + 8 D bytes per row and direction at 8 TB/s) and the FMA bound
            (8 K^2 + 12 K fp32 FMAs per row-frame, the figure of adn_echo.h, at 78.6 T FMA/s) with the share of each
    hour    one hour of 8 kHz audio (60 rows of 60 s) through adn_aec_online and through the whole EchoCanceller.cancel

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up: the median,
the least and the most of `--groups` windows (tools/bench_common.py).  The step that is timed is a steady-state one (the last step
the object ran) of seeded uniform audio; calling it again reads the same ring rows, and the values move (e goes back into the ring in
place) while the time does not depend on them.  One JSON line per record.

    python tools/bench_echo.py [--write profiles] [--commit ID]
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


class TorchRls:
    """The recursion of adn_echo.h ("echo stream") from torch ops, batched over rows (pair x bin)."""

    def __init__(self, rows, params, dev):
        import torch
        self.K, self.D, self.alpha, self.quiet = params.taps, params.delay, params.forget, params.quiet
        self.h = torch.zeros((rows, self.K), dtype=torch.complex64, device=dev)
        self.P = torch.eye(self.K, dtype=torch.complex64, device=dev).repeat(rows, 1, 1) / params.loading
        self.past = torch.zeros((rows, self.D + self.K), dtype=torch.complex64, device=dev)      # R_{t-D-K+1} ... R_t
        self.low = torch.tril(torch.ones((self.K, self.K), dtype=torch.bool, device=dev))

    def block(self, y, r):
        """y, r (R, B) complex64, the next B frames of every row -> e (R, B)."""
        import torch
        out = torch.empty_like(y)
        for t in range(y.shape[1]):
            self.past = torch.cat([self.past[:, 1:], r[:, t:t + 1]], dim=1)
            taps = self.past[:, :self.K].flip(1)                     # column j = R_{t-D-j}
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
    ap.add_argument("--pairs", default="1,64,256")
    ap.add_argument("--taps", default="8,16,32")
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--no-hour", action="store_true")
    ap.add_argument("--write", default=None, help="directory for bench_echo.jsonl and the device block of bench_echo.md")
    ap.add_argument("--commit", default=None, help="recorded with every line when given")
    args = ap.parse_args()
    import torch
    from audiodenoiser_amd import build
    from audiodenoiser_amd.dereverb import StreamDereverberator, WpeStreamParams, _wpe_then_gain
    from audiodenoiser_amd.echo import AecParams, EchoCanceller, StreamEchoCanceller, aec_online, aec_stream_state_bytes
    from audiodenoiser_amd.griffin_lim import stft_complex
    if not torch.cuda.is_available():
        raise SystemExit("bench_echo: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    records, block, f = [], args.block, 257
    steps = 8
    length = steps * block * 128                                     # `steps` whole steps and the look of a running stream
    timing = (args.warmup, args.groups, args.window_ms)

    for taps in (int(v) for v in args.taps.split(",")):
        forget = max(AecParams.forget if taps <= 16 else 0.985, 0.95)
        p = AecParams(taps=taps, forget=forget)
        for n in (int(v) for v in args.pairs.split(",")):
            g = torch.Generator(device=dev).manual_seed(1000 * taps + n)
            se = StreamEchoCanceller(dev, pairs=n, block_frames=block, params=p)
            se.push(torch.rand((2 * n, length), generator=g, device=dev) - 0.5)
            last = se._done - 1
            assert last >= 1
            win = torch.zeros((2 * n, 1, f, se.window_frames), device=dev)
            sd = StreamDereverberator(dev, n_streams=n, block_frames=block, params=WpeStreamParams(taps=taps, forget=max(forget, 0.99)))
            sd.push(torch.rand((n, length), generator=g, device=dev) - 0.5)
            wwin = torch.zeros((n, 1, f, sd.window_frames), device=dev)
            rls = TorchRls(n * f, p, dev)
            y, r = ((torch.rand((n * f, block), generator=g, device=dev) - 0.5).to(torch.complex64) for _ in range(2))
            t_aec = time_ms(lambda: se._cancel(win, last, 1), *timing)
            t_wpe = time_ms(lambda: _wpe_then_gain(sd, wwin, None, 1, sd._done - 1, -1), *timing)
            t_torch = time_ms(lambda: rls.block(y, r), *timing)
            state_bytes = 2 * aec_stream_state_bytes(n, f, p)
            bound_ms = state_bytes / HBM_BPS * 1e3
            fma_ms = n * f * block * (8 * taps * taps + 12 * taps) / FMA_PER_S * 1e3
            lanes = 8 if taps <= 8 else 16 if taps <= 16 else 32
            rec = {"record": "step", "taps": taps, "forget": forget, "pairs": n, "block": block, "lanes_per_row": lanes,
                   "workgroups": n * -(-f // (256 // lanes)), "aec_stream": t_aec, "wpe_stream_same_taps_and_rows": t_wpe,
                   "aec_over_wpe": round(t_aec["ms"] / t_wpe["ms"], 3), "torch_ops": t_torch,
                   "torch_over_aec": round(t_torch["ms"] / t_aec["ms"], 1), "state_bytes": state_bytes,
                   "state_bound_ms": round(bound_ms, 6), "share_of_state_bound": round(bound_ms / t_aec["ms"], 4),
                   "fma_bound_ms": round(fma_ms, 6), "share_of_fma_bound": round(fma_ms / t_aec["ms"], 4)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del se, sd, rls, win, wwin, y, r
            torch.cuda.empty_cache()

    if not args.no_hour:
        rows, seconds = 60, 60
        g = torch.Generator(device=dev).manual_seed(7)
        mic, far = (torch.rand((rows, seconds * 8000), generator=g, device=dev) - 0.5 for _ in range(2))
        ms, fs = stft_complex(mic, 512, 128), stft_complex(far, 512, 128)
        ec = EchoCanceller(dev)
        hour = (args.warmup, args.groups, 1.0)
        t_online = time_ms(lambda: aec_online(ms, fs), *hour)
        t_cancel = time_ms(lambda: ec.cancel(mic, far), *hour)
        rec = {"record": "hour", "rows": rows, "seconds": seconds, "frames": int(ms.shape[1]), "aec_online": t_online,
               "cancel": t_cancel, "real_time_factor_cancel": round(rows * seconds / (t_cancel["ms"] * 1e-3), 0)}
        records.append(rec)
        print(json.dumps(rec), flush=True)

    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_echo.jsonl"), "w") as fh:
            for r in records:
                fh.write(json.dumps(dict(r, library_digest=digest[:16], **({"commit": args.commit} if args.commit else {}))) + "\n")
        text = (f"Written by `tools/bench_echo.py` on one MI355X (device events, windows after a warm-up, median [least, most] of "
                f"{args.groups}); n_fft 512, hop 128, block {block}: one step is {block} frames of every pair.\n\n"
                "| taps | pairs | lanes | `adn_aec_stream` | `adn_wpe_stream`, same taps and rows | ratio | torch ops | state bound; share | FMA bound; share |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        span = lambda t: f"{t['ms']:.4f} [{t['ms_min']:.4f}, {t['ms_max']:.4f}] ms"  # noqa: E731
        for r in records:
            if r["record"] == "step":
                text += (f"| {r['taps']} | {r['pairs']} | {r['lanes_per_row']} | {span(r['aec_stream'])} | {span(r['wpe_stream_same_taps_and_rows'])} | "
                         f"{r['aec_over_wpe']:.2f} | {r['torch_ops']['ms']:.2f} ms ({r['torch_over_aec']} x) | {r['state_bound_ms']:.5f} ms; "
                         f"{r['share_of_state_bound']:.3f} | {r['fma_bound_ms']:.5f} ms; {r['share_of_fma_bound']:.3f} |\n")
        for r in records:
            if r["record"] == "hour":
                text += (f"\nOne hour of 8 kHz audio ({r['rows']} rows of {r['seconds']} s, {r['frames']} frames each): `adn_aec_online` "
                         f"{span(r['aec_online'])}; the whole `EchoCanceller.cancel` {span(r['cancel'])}, "
                         f"{r['real_time_factor_cancel']:.0f} x real time.\n")
        write_marked_block(os.path.join(args.write, "bench_echo.md"), text)


if __name__ == "__main__":
    main()
