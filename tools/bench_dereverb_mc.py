#!/usr/bin/env python3
"""Device time of multichannel dereverberation (adn_wpe_mc; Dereverberator(channels="joint").denoise as a whole) beside the
parent's path on the same clips (adn_wpe at K = 20, every channel alone) and the same steps composed from torch ops
(torch.linalg batched over bins), and the kernel's time against its FMA bound.  Buffers are allocated once; device events around a
window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of `--groups` windows.

Every step is a child process of its own under its own time limit, and the tool ends at the first step that fails or runs out of
time: nothing is started on a device after a failure.  One JSON line per measurement, and the same figures as a table into the
marked device block of `--out` (default profiles/bench_dereverb_mc.md):

    kernel   adn_wpe_mc at (C, K) = (2, 10) and (2, 16), and adn_wpe at K = 20 on the same 2 n clips.  `fma_bound_ms`: per (group, bin)
             and iteration 4 T (N (N + 1) / 2 + N C + N C) FMAs -- the correlation R, P and the filter -- at the chip's 78.6 T fp32
             FMA/s (adn_wpe: 4 T (K (K + 1) / 2 + 2 K) per (clip, bin))
    denoise  Dereverberator.denoise with channels="joint" and with channels="separate", device tensor in, device tensor out
    torch    the definition's steps at (2, 16) as torch ops on the device: unfold, batched matmuls, torch.linalg.cholesky,
             torch.cholesky_solve; its difference from adn_wpe_mc's result

Workloads: one hour of 8 kHz audio as 30 two-channel recordings of 60 s, and one two-channel recording of 3 s; the burst signal of
tests/baseline_cases.py through the device's Freeverb (audiodenoiser_amd.reverb) at the rate arguments 8000 and 8600 -- two rooms.

    python tools/bench_dereverb_mc.py [--cases 0,1] [--out profiles/bench_dereverb_mc.md]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import time_ms, write_marked_block  # noqa: E402

FMA_PER_S = 157.3e12 / 2           # peak fp32 vector rate of the MI355X, two flops per FMA
RATE = 8000
N_FFT, HOP = 512, 128
CHANNELS = 2
MIC_RATES = (8000, 8600)
JOINT_TAPS = (10, 16)
ALONE_TAPS = 20
CASES = (("one_hour", 30, 60 * RATE), ("one_recording_3s", 1, 3 * RATE))
STEPS = ("kernel", "denoise", "torch")
STEP_LIMIT_S = 300


def torch_wpe_mc(spec, channels, taps, delay=3, iterations=3, loading=1e-3, power_floor=1e-3):
    """The definition of include/adn.h ("dereverb multichannel") composed from torch ops, every (group, bin) a batch entry."""
    import torch
    n, t, f = spec.shape
    g, c, nn = n // channels, channels, channels * taps
    x = spec.reshape(g, c, t, f).permute(0, 3, 1, 2).reshape(g * f, c, t)         # (B, C, T)
    xp = torch.nn.functional.pad(torch.view_as_real(x), (0, 0, delay + taps - 1, 0))
    xp = torch.view_as_complex(xp.contiguous())                                  # zeros in front of every channel
    past = xp[:, :, :t + taps - 1].unfold(2, taps, 1).flip(-1)                   # (B, C, T, K): X_{t - delay - j, c}
    past = past.permute(0, 2, 1, 3).reshape(g * f, t, nn)                        # stacked r = c K + j
    p = x.real * x.real + x.imag * x.imag
    phi = (power_floor * p.sum((1, 2)) / (t * c)).clamp_min(1e-30)
    d = x
    eye = torch.eye(nn, dtype=torch.float32, device=spec.device)
    for _ in range(iterations):
        lam = torch.maximum((d.real * d.real + d.imag * d.imag).sum(1) / c, phi[:, None])
        u = (past / lam[:, :, None]).transpose(1, 2)                             # (B, N, T)
        r = u @ past.conj()
        pv = u @ x.conj().transpose(1, 2)                                        # (B, N, C)
        tr = torch.diagonal(r, dim1=1, dim2=2).real.sum(1)
        a = r + ((loading * tr / nn + 1e-30)[:, None, None] * eye).to(r.dtype)
        taps_g = torch.cholesky_solve(pv, torch.linalg.cholesky(a))
        d = x - (past @ taps_g.conj()).transpose(1, 2)
        d = torch.cat([x[:, :, :delay], d[:, :, delay:]], dim=2)
    return d.reshape(g, f, c, t).permute(0, 2, 3, 1).reshape(n, t, f).contiguous()


def run_step(step, case, args):
    """One step in this process: JSON lines on stdout."""
    import numpy as np
    import torch
    import baseline_cases as bc
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams
    from audiodenoiser_amd.griffin_lim import stft_complex
    from audiodenoiser_amd.reverb import reverb
    if not torch.cuda.is_available():
        raise SystemExit("bench_dereverb_mc: no ROCm device is visible; nothing is measured without one")
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.adn_prepare(0, N_FFT), "adn_prepare")
    name, n_rec, length = CASES[case]
    emit = lambda row: print(json.dumps({"case": name, **row}), flush=True)  # noqa: E731
    dry = torch.from_numpy(np.stack([bc.speech_like(length, 100 + i).astype(np.float32) for i in range(n_rec)])).to(dev)
    x = torch.stack([reverb(dry, r) for r in MIC_RATES], dim=1).reshape(n_rec * CHANNELS, length).contiguous()   # channels consecutive
    n = n_rec * CHANNELS
    t, f = 1 + length // HOP, N_FFT // 2 + 1
    D, I = WpeParams().delay, WpeParams().iterations
    if step == "denoise":
        for mode in ("joint", "separate"):
            dn = Dereverberator(dev, channels=mode)
            audio = x.reshape(n_rec, CHANNELS, length) if mode == "joint" else x
            row = time_ms(lambda: dn.denoise(audio), args.warmup, args.groups, args.window_ms)
            emit({"what": f"denoise_{mode}", "shape": list(audio.shape), **row,
                  "audio_s_per_s": round(n_rec * length / RATE / (row["ms"] * 1e-3), 1)})
        return
    spec = stft_complex(x, N_FFT, HOP)
    s = torch.view_as_real(spec)
    out = torch.empty_like(s)
    mag = torch.zeros((n, 1, f, max(t, 16)), device=dev)
    if step == "kernel":
        for taps in JOINT_TAPS:
            ps = ctypes_params(WpeParams(taps=taps))

            def kernel():
                _lib.check(L.adn_wpe_mc(s.data_ptr(), n_rec, CHANNELS, t, f, ps, None, 0, out.data_ptr(), mag.data_ptr(), int(mag.shape[3]), st),
                           "adn_wpe_mc")
            row = time_ms(kernel, args.warmup, args.groups, args.window_ms)
            nn = CHANNELS * taps
            fma = n_rec * f * I * 4 * t * (nn * (nn + 1) // 2 + 2 * nn * CHANNELS)
            fma_ms = fma / FMA_PER_S * 1e3
            emit({"what": f"adn_wpe_mc_k{taps}", "shape": [n_rec, CHANNELS, t, f], "params": [taps, D, I], **row, "fma": fma,
                  "fma_bound_ms": round(fma_ms, 4), "share_of_bound": round(fma_ms / row["ms"], 4)})
        ps = ctypes_params(WpeParams(taps=ALONE_TAPS))

        def alone():
            _lib.check(L.adn_wpe(s.data_ptr(), n, t, f, ps, None, 0, out.data_ptr(), mag.data_ptr(), int(mag.shape[3]), st), "adn_wpe")
        row = time_ms(alone, args.warmup, args.groups, args.window_ms)
        fma = n * f * I * 4 * t * (ALONE_TAPS * (ALONE_TAPS + 1) // 2 + 2 * ALONE_TAPS)
        fma_ms = fma / FMA_PER_S * 1e3
        emit({"what": "adn_wpe_k20", "shape": [n, t, f], "params": [ALONE_TAPS, D, I], **row, "fma": fma,
              "fma_bound_ms": round(fma_ms, 4), "share_of_bound": round(fma_ms / row["ms"], 4)})
        return
    taps = JOINT_TAPS[-1]
    ps = ctypes_params(WpeParams(taps=taps))
    _lib.check(L.adn_wpe_mc(s.data_ptr(), n_rec, CHANNELS, t, f, ps, None, 0, out.data_ptr(), mag.data_ptr(), int(mag.shape[3]), st), "adn_wpe_mc")
    ref = torch_wpe_mc(spec, CHANNELS, taps, D, I)
    diff = float((torch.view_as_complex(out) - ref).abs().max() / ref.abs().max())
    del ref
    row = time_ms(lambda: torch_wpe_mc(spec, CHANNELS, taps, D, I), 1, 3, min(args.window_ms, 100.0))
    emit({"what": f"torch_wpe_mc_k{taps}", **row, "max_rel_diff_from_adn_wpe_mc": diff})


def ctypes_params(p):
    import ctypes
    return ctypes.byref(p.to_struct())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1", help="indices into CASES")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_dereverb_mc.md"))
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run one step of one case in this process")
    args = ap.parse_args()
    cases = [int(v) for v in args.cases.split(",")]
    if args.step is not None:
        run_step(args.step, cases[0], args)
        return 0
    lines = []
    for case in cases:
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--cases", str(case), "--warmup", str(args.warmup),
                   "--groups", str(args.groups), "--window-ms", str(args.window_ms)]
            try:
                run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"bench_dereverb_mc: step {step} of case {CASES[case][0]} ran past {STEP_LIMIT_S} s; nothing more is started", file=sys.stderr)
                return 1
            sys.stdout.write(run.stdout)
            sys.stdout.flush()
            if run.returncode != 0:
                sys.stderr.write(run.stderr[-4000:])
                print(f"bench_dereverb_mc: step {step} of case {CASES[case][0]} ended with status {run.returncode}; nothing more is started",
                      file=sys.stderr)
                return 1
            lines += [json.loads(v) for v in run.stdout.splitlines() if v.startswith("{")]
    by = {(r["case"], r["what"]): r for r in lines}
    cell = lambda c, w, key, fmt="{}": fmt.format(by[(c, w)][key]) if (c, w) in by and key in by[(c, w)] else "not measured"  # noqa: E731
    hour, clip = CASES[0][0], CASES[1][0]

    def kernel_rows(what, label):
        return (f"| {label} (1 launch) | {cell(hour, what, 'ms')} ms | {cell(clip, what, 'ms')} ms |\n"
                f"| its FMA bound at 78.6 T FMA/s; share of it | {cell(hour, what, 'fma_bound_ms')} ms; {cell(hour, what, 'share_of_bound')} | "
                f"{cell(clip, what, 'fma_bound_ms')} ms; {cell(clip, what, 'share_of_bound')} |\n")

    def ratio(c, a, b):
        return f"{by[(c, a)]['ms'] / by[(c, b)]['ms']:.2f}" if (c, a) in by and (c, b) in by else "not measured"

    block = ("Written by `tools/bench_dereverb_mc.py` on one MI355X (device events, windows after a warm-up, median of "
             f"{args.groups}; every step a process of its own); D 3, I 3, n_fft {N_FFT}, hop {HOP}, two channels.\n\n"
             "| measurement | one hour (30 x 2 x 480 000) | one recording (2 x 24 000) |\n|---|---|---|\n"
             + kernel_rows("adn_wpe_mc_k10", "`adn_wpe_mc` (2, 10), stacked size 20")
             + kernel_rows("adn_wpe_mc_k16", "`adn_wpe_mc` (2, 16), stacked size 32")
             + kernel_rows("adn_wpe_k20", "`adn_wpe` K = 20 on the same 2 n clips: the parent's path")
             + f"| `adn_wpe_mc` (2, 10) / `adn_wpe` K = 20 | {ratio(hour, 'adn_wpe_mc_k10', 'adn_wpe_k20')} | {ratio(clip, 'adn_wpe_mc_k10', 'adn_wpe_k20')} |\n"
             f"| `adn_wpe_mc` (2, 16) / `adn_wpe` K = 20 | {ratio(hour, 'adn_wpe_mc_k16', 'adn_wpe_k20')} | {ratio(clip, 'adn_wpe_mc_k16', 'adn_wpe_k20')} |\n"
             f"| `Dereverberator(channels=\"joint\").denoise`, taps 16 | {cell(hour, 'denoise_joint', 'ms')} ms = {cell(hour, 'denoise_joint', 'audio_s_per_s')} s of recording per s | "
             f"{cell(clip, 'denoise_joint', 'ms')} ms = {cell(clip, 'denoise_joint', 'audio_s_per_s')} s/s |\n"
             f"| `Dereverberator().denoise` on the same clips, taps 20 | {cell(hour, 'denoise_separate', 'ms')} ms | {cell(clip, 'denoise_separate', 'ms')} ms |\n"
             f"| (2, 16) from torch ops (`torch.linalg` batched over bins) | {cell(hour, 'torch_wpe_mc_k16', 'ms')} ms ({ratio(hour, 'torch_wpe_mc_k16', 'adn_wpe_mc_k16')} x `adn_wpe_mc`) | "
             f"{cell(clip, 'torch_wpe_mc_k16', 'ms')} ms ({ratio(clip, 'torch_wpe_mc_k16', 'adn_wpe_mc_k16')} x) |\n"
             f"| torch composition against `adn_wpe_mc`, max relative difference | {cell(hour, 'torch_wpe_mc_k16', 'max_rel_diff_from_adn_wpe_mc', '{:.3g}')} | "
             f"{cell(clip, 'torch_wpe_mc_k16', 'max_rel_diff_from_adn_wpe_mc', '{:.3g}')} |\n")
    write_marked_block(args.out, block)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
