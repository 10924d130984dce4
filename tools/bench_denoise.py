#!/usr/bin/env python3
"""Device time of the long-form denoiser (audiodenoiser_amd/denoise.py) stage by stage, and of adn_denoise_resynth against its
memory bound and against the same step composed from what the tree offered before it (torch ops for the stitch, clamp,
transposition and rescale, then adn_istft) -- same process, same tensors, alternating.

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows.  One JSON line per record:

    stage    stft | windows | unet | resynth | denoise (Denoiser.denoise on a resident tensor, allocations included)
    resynth  bytes = y + X read once + audio written once; bound_ms at 8 TB/s and at the 6.3 TB/s profiles/NOTES.md calls
             achievable; composed_ms and the ratio; max |fused - composed| over the samples both produce

    python tools/bench_denoise.py [--write profiles] [--commit ID]

Synthetic weights (seed 1234): times do not depend on the weights' values.  Kernel-level figures:
rocprofv3 --kernel-trace --stats -- python tools/bench_denoise.py --cases 1 (a run of its own).
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS, HBM_ACHIEVABLE_BPS = 8.0e12, 6.3e12
CASES = ((60, 480000), (1, 24000))           # one hour of 8 kHz audio as 60 clips x 60 s; one 3 s clip


def time_ms(fns, warmup, groups, window_ms):
    """Median / min / max milliseconds per call of every fn in `fns`, their windows alternating group by group."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps = []
    for fn in fns:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        steps.append(max(3, int(math.ceil(window_ms / max(e0.elapsed_time(e1), 1e-3)))))
    out = [[] for _ in fns]
    for _ in range(groups):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps[i]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / steps[i])
    return [(statistics.median(o), min(o), max(o), s) for o, s in zip(out, steps)]


def composed_resynth(dn, y, spec, n_clips, n_frames):
    """The step a user had to write before adn_denoise_resynth: cross-fade in torch, clamp, transpose, rescale, istft."""
    import torch
    from audiodenoiser_amd.griffin_lim import istft
    k, width = dn.plan(n_frames)
    f, v, stride = y.shape[2], dn.overlap_frames, dn.window_frames - dn.overlap_frames
    yk = y.view(n_clips, k, f, width)
    ramp = torch.arange(1, v + 1, device=y.device, dtype=torch.float32) / (v + 1)
    out = torch.zeros((n_clips, f, n_frames), device=y.device)
    for i in range(k):
        n = min(width, n_frames - i * stride)
        a = torch.ones(width, device=y.device)
        if i > 0:
            a[:v] = ramp
        if i < k - 1:
            a[width - v:] = ramp.flip(0)
        out[:, :, i * stride:i * stride + n] += a[:n] * yk[:, i, :, :n]
    m = out.clamp_(min=0).transpose(1, 2)
    mag = spec.abs()
    s_hat = torch.where(mag > 0, m * spec / torch.where(mag > 0, mag, torch.ones_like(mag)), m.to(torch.complex64))
    return istft(s_hat.contiguous(), dn.hop_length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1", help="indices into CASES")
    ap.add_argument("--dtypes", default="f32,f16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--write", default=None, help="directory for bench_denoise.jsonl / bench_denoise.md")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import Denoiser, build
    from audiodenoiser_amd.griffin_lim import stft_complex
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.weights import make_state_dict
    assert torch.cuda.is_available(), "bench_denoise.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    sd = make_state_dict(1234)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for dtype in args.dtypes.split(","):
        net = UNet(1, 1)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        net = net.to(dev).eval().set_compute_dtype(dtype)
        dn = Denoiser(net)
        for case in (int(c) for c in args.cases.split(",")):
            n, length = CASES[case]
            g = torch.Generator(device=dev).manual_seed(case)
            x = torch.rand((n, length), generator=g, device=dev) - 0.5
            t = 1 + length // dn.hop_length
            k, width = dn.plan(t)
            spec = stft_complex(x, dn.n_fft, dn.hop_length)
            win = dn.windows(spec)
            y = dn.network(win)
            seconds = n * length / dn.sample_rate
            stages = (("stft", lambda: stft_complex(x, dn.n_fft, dn.hop_length)), ("windows", lambda: dn.windows(spec)),
                      ("unet", lambda: dn.network(win)), ("resynth", lambda: dn.resynth(y, spec, length)),
                      ("denoise", lambda: dn.denoise(x)))
            times = time_ms([fn for _, fn in stages], args.warmup, args.groups, args.window_ms)
            total = sum(tm[0] for (name, _), tm in zip(stages, times) if name != "denoise")
            for (name, _), (ms, lo, hi, steps) in zip(stages, times):
                emit({"record": "stage", "dtype": dtype, "clips": n, "samples": length, "windows": n * k, "stage": name, "ms": round(ms, 4),
                      "ms_min": round(lo, 4), "ms_max": round(hi, 4), "steps_per_window": steps,
                      "audio_s_per_s": round(seconds / (ms * 1e-3), 1), "share_of_stage_sum": round(ms / total, 4) if name != "denoise" else None})
            if dtype != args.dtypes.split(",")[0]:
                continue                                          # the resynthesis step does not depend on the model's dtype
            nbytes = y.numel() * 4 + spec.numel() * 8 + n * length * 4
            (fused, f_lo, f_hi, _), (comp, c_lo, c_hi, _) = time_ms(
                [lambda: dn.resynth(y, spec, length), lambda: composed_resynth(dn, y, spec, n, t)], args.warmup, args.groups, args.window_ms)
            a, b = dn.resynth(y, spec, length), composed_resynth(dn, y, spec, n, t)
            diff = float((a[:, :b.shape[1]] - b).abs().max() / b.abs().max())
            emit({"record": "resynth", "clips": n, "samples": length, "frames": t, "bytes": nbytes, "fused_ms": round(fused, 4),
                  "fused_ms_min": round(f_lo, 4), "fused_ms_max": round(f_hi, 4), "GBps": round(nbytes / (fused * 1e-3) / 1e9, 1),
                  "bound_ms_8TBps": round(nbytes / HBM_BPS * 1e3, 4), "bound_ms_6p3TBps": round(nbytes / HBM_ACHIEVABLE_BPS * 1e3, 4),
                  "share_of_8TBps": round(nbytes / HBM_BPS * 1e3 / fused, 3), "composed_ms": round(comp, 4), "composed_ms_min": round(c_lo, 4),
                  "composed_ms_max": round(c_hi, 4), "composed_over_fused": round(comp / fused, 2), "max_rel_diff_fused_vs_composed": diff})
            del x, spec, win, y, a, b
            net._workspace = None
            torch.cuda.empty_cache()
    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_denoise.jsonl"), "w") as fh:
            for rec in records:
                fh.write(json.dumps(dict(rec, commit=args.commit, library_digest=digest[:16])) + "\n")
        with open(os.path.join(args.write, "bench_denoise.md"), "w") as fh:
            fh.write("# Long-form denoiser on one MI355X (`tools/bench_denoise.py`)\n\n")
            fh.write(f"Commit `{args.commit}`, library code digest `{digest[:16]}`.  Raw lines: `bench_denoise.jsonl` (device events, windows of at "
                     f"least {args.window_ms / 1e3:g} s after warm-up, median of {args.groups}).  Synthetic weights; defaults n_fft 512, hop 128, "
                     "window 256, overlap 32, batch_windows 64.\n\n## Stages\n\n")
            fh.write("| model | clips x samples | windows | stage | ms | audio s / s | share of the four stages |\n|---|---|---|---|---|---|---|\n")
            for r in records:
                if r["record"] == "stage":
                    share = "" if r["share_of_stage_sum"] is None else f"{r['share_of_stage_sum']:.4f}"
                    fh.write(f"| {r['dtype']} | {r['clips']} x {r['samples']} | {r['windows']} | {r['stage']} | {r['ms']} | {r['audio_s_per_s']} | {share} |\n")
            fh.write("\n`denoise` is `Denoiser.denoise` on a resident tensor (the four stages plus their allocations).\n\n## adn_denoise_resynth\n\n")
            fh.write("| clips x samples | bytes | fused ms (min-max) | GB/s | bound at 8 TB/s | bound at 6.3 TB/s | share of 8 TB/s | composed ms (min-max) | composed / fused | max rel. diff |\n"
                     "|---|---|---|---|---|---|---|---|---|---|\n")
            for r in records:
                if r["record"] == "resynth":
                    fh.write(f"| {r['clips']} x {r['samples']} | {r['bytes']} | {r['fused_ms']} ({r['fused_ms_min']}-{r['fused_ms_max']}) | {r['GBps']} | "
                             f"{r['bound_ms_8TBps']} ms | {r['bound_ms_6p3TBps']} ms | {r['share_of_8TBps']} | {r['composed_ms']} "
                             f"({r['composed_ms_min']}-{r['composed_ms_max']}) | {r['composed_over_fused']} | {r['max_rel_diff_fused_vs_composed']:.3g} |\n")
            fh.write("\nComposed = the cross-fade, clamp, transposition and rescale as torch ops, then `istft` (the form a user had before "
                     "the fused kernel), timed in the same process on the same tensors, windows alternating.\n"
                     "Per-kernel `rocprofv3` figures and hardware counters: not measured.\n")


if __name__ == "__main__":
    main()
