#!/usr/bin/env python3
"""Device time of the beamformer (adn_mvdr; Beamformer.denoise as a whole) beside the same steps composed from torch ops (einsum,
torch.linalg.solve batched over bins), the kernel's time against its memory bound and its FMA bound, and the SI-SDR table on the
device beside the restatement's.  Buffers are allocated once; device events around a window of calls (at least `--window-ms` long,
sized from a calibration call) after a warm-up, median of `--groups` windows.

Every step is a child process of its own under its own time limit, and the tool ends at the first step that fails or runs out of
time: nothing is started on a device after a failure.  One JSON line per measurement, and the same figures as tables into the
marked device block of `--out` (default profiles/bench_beamform.md):

    kernel   adn_mvdr.  `mem_bound_ms`: (2 x 8 C + 4 C + 8 + 4) T F bytes per group -- spec read twice, the mask magnitudes once, both
             outputs written -- at 8 TB/s; `fma_bound_ms`: 4 T (C (C + 1) + C) FMAs per (group, bin) at the chip's 78.6 T fp32 FMA/s
    denoise  Beamformer.denoise, device tensor in, device tensor out (STFT, spectral gain per channel, adn_mvdr, resynthesis)
    torch    the definition's steps as torch ops on the device; its difference from adn_mvdr's result
    quality  (once) SI-SDR of Beamformer.denoise on the 8 dB recordings of tests/beamform_cases.py beside the restatement's

Workloads: one hour of 8 kHz audio as 30 two-channel and as 15 four-channel recordings of 60 s, and one four-channel recording of
3 s; the burst signal of tests/baseline_cases.py through the device's Freeverb at one rate argument per microphone, plus white
noise at 8 dB per microphone.

    python tools/bench_beamform.py [--cases 0,1,2] [--out profiles/bench_beamform.md]
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
BYTES_PER_S = 8.0e12               # peak HBM rate of the MI355X
RATE = 8000
N_FFT, HOP = 512, 128
MIC_RATES = (8000, 8600, 7500, 9100)
CASES = (("one_hour_2ch", 30, 2, 60 * RATE), ("one_hour_4ch", 15, 4, 60 * RATE), ("one_recording_3s_4ch", 1, 4, 3 * RATE))
STEPS = ("kernel", "denoise", "torch")
STEP_LIMIT_S = 300
QUALITY_ROWS = (("MVDR, mask from the spectral gain", dict()), ("MVDR, then the spectral gain", dict(gain=True)),
                ("joint WPE, then MVDR", dict(wpe=True)), ("joint WPE, then MVDR, then gain", dict(wpe=True, gain=True)))


def torch_mvdr(spec, mag, channels, ref=0, loading=1e-3, rho=1e-3):
    """The definition of include/adn.h ("beamform") composed from torch ops, every (group, bin) a batch entry."""
    import torch
    n, t, f = spec.shape
    g, c = n // channels, channels
    x = spec.reshape(g, c, t, f)
    m2 = (mag[:, 0, :, :t] ** 2).reshape(g, c, f, t).sum(1).transpose(1, 2)      # (g, t, f)
    q = (x.real * x.real + x.imag * x.imag).sum(1)
    m = torch.where(q > 0, (m2 / q).clamp(rho, 1.0 - rho), torch.full_like(q, rho))
    xc = x.conj()
    phi_s = torch.einsum("grtf,gktf->gfrk", x * m[:, None], xc)
    phi_n = torch.einsum("grtf,gktf->gfrk", x * (1.0 - m)[:, None], xc)
    tr = torch.diagonal(phi_n, dim1=2, dim2=3).real.sum(-1)
    a = phi_n + ((loading * tr / c + 1e-30)[..., None, None] * torch.eye(c, device=spec.device)).to(phi_n.dtype)
    gm = torch.linalg.solve(a, phi_s)
    tau = torch.diagonal(gm, dim1=2, dim2=3).real.sum(-1).clamp_min(1e-30)
    w = gm[..., ref] / tau[..., None]                                            # (g, f, c)
    return torch.einsum("gfc,gctf->gtf", w.conj(), x).contiguous()


def recordings(dev, n_rec, channels, length, seed=100):
    """(n_rec * channels, length) on the device, the channels of a recording consecutive."""
    import numpy as np
    import torch
    import baseline_cases as bc
    from audiodenoiser_amd.reverb import reverb
    dry = torch.from_numpy(np.stack([bc.speech_like(length, seed + i).astype(np.float32) for i in range(n_rec)])).to(dev)
    x = torch.stack([reverb(dry, r) for r in MIC_RATES[:channels]], dim=1).reshape(n_rec * channels, length)
    gen = torch.Generator(device=dev).manual_seed(seed)
    noise = torch.randn(x.shape, generator=gen, device=dev)
    scale = (x.pow(2).mean(1, keepdim=True) / noise.pow(2).mean(1, keepdim=True)).sqrt() * 10.0 ** (-8.0 / 20.0)
    return (x + scale * noise).contiguous()


def run_quality():
    """SI-SDR of Beamformer.denoise on the 8 dB recordings beside the restatement's: JSON lines on stdout."""
    import torch
    import beamform_cases as bcs
    from audiodenoiser_amd.beamform import Beamformer
    from audiodenoiser_amd.metrics import evaluate
    dev = torch.device("cuda", 0)
    for label, kw in QUALITY_ROWS:
        for c in bcs.TABLE_CHANNELS:
            want = bcs.restatement_si_sdr(label, c)
            if want is None:
                continue
            noisy, dry = bcs.recording(c)
            out = Beamformer(dev, **kw).denoise(torch.from_numpy(noisy.copy()).to(dev))
            got = float(evaluate(out[None], torch.from_numpy(dry.copy()).to(dev)[None], sr=RATE)["si_sdr"][0])
            print(json.dumps({"case": "quality", "what": label, "channels": c, "si_sdr_device": round(got, 2),
                              "si_sdr_restatement": round(want, 2)}), flush=True)


def run_step(step, case, args):
    """One step in this process: JSON lines on stdout."""
    import torch
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import spectral_gain
    from audiodenoiser_amd.beamform import Beamformer
    from audiodenoiser_amd.griffin_lim import stft_complex
    if not torch.cuda.is_available():
        raise SystemExit("bench_beamform: no ROCm device is visible; nothing is measured without one")
    if step == "quality":
        return run_quality()
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.adn_prepare(0, N_FFT), "adn_prepare")
    name, n_rec, c, length = CASES[case]
    emit = lambda row: print(json.dumps({"case": name, **row}), flush=True)  # noqa: E731
    x = recordings(dev, n_rec, c, length)
    t, f = 1 + length // HOP, N_FFT // 2 + 1
    if step == "denoise":
        bf, audio = Beamformer(dev), x.reshape(n_rec, c, length)
        row = time_ms(lambda: bf.denoise(audio), args.warmup, args.groups, args.window_ms)
        emit({"what": "denoise", "shape": list(audio.shape), **row, "audio_s_per_s": round(n_rec * length / RATE / (row["ms"] * 1e-3), 1)})
        return
    spec = stft_complex(x, N_FFT, HOP)
    mag, _ = spectral_gain(spec)
    s = torch.view_as_real(spec)
    out = torch.empty((n_rec, t, f, 2), device=dev)
    out_mag = torch.zeros((n_rec, 1, f, max(t, 16)), device=dev)

    def kernel():
        _lib.check(L.adn_mvdr(s.data_ptr(), mag.data_ptr(), int(mag.shape[3]), n_rec, c, t, f, None, None, 0, out.data_ptr(),
                              out_mag.data_ptr(), int(out_mag.shape[3]), st), "adn_mvdr")
    if step == "kernel":
        row = time_ms(kernel, args.warmup, args.groups, args.window_ms)
        fma = n_rec * f * 4 * t * (c * (c + 1) + c)
        nbytes = n_rec * (2 * 8 * c + 4 * c + 8 + 4) * t * f
        fma_ms, mem_ms = fma / FMA_PER_S * 1e3, nbytes / BYTES_PER_S * 1e3
        emit({"what": "adn_mvdr", "shape": [n_rec, c, t, f], **row, "fma": fma, "bytes": nbytes, "fma_bound_ms": round(fma_ms, 4),
              "share_of_fma_bound": round(fma_ms / row["ms"], 4), "mem_bound_ms": round(mem_ms, 4),
              "share_of_mem_bound": round(mem_ms / row["ms"], 4)})
        return
    kernel()
    ref = torch_mvdr(spec, mag, c)
    diff = float((torch.view_as_complex(out) - ref).abs().max() / ref.abs().max())
    del ref
    row = time_ms(lambda: torch_mvdr(spec, mag, c), 1, 3, min(args.window_ms, 100.0))
    emit({"what": "torch_mvdr", **row, "max_rel_diff_from_adn_mvdr": diff})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2", help="indices into CASES")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--no-quality", action="store_true", help="leave the SI-SDR table out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_beamform.md"))
    ap.add_argument("--step", choices=STEPS + ("quality",), default=None, help="(internal) run one step of one case in this process")
    args = ap.parse_args()
    cases = [int(v) for v in args.cases.split(",")]
    if args.step is not None:
        run_step(args.step, cases[0], args)
        return 0
    jobs = [(step, case) for case in cases for step in STEPS] + ([] if args.no_quality else [("quality", cases[0])])
    lines = []
    for step, case in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--cases", str(case), "--warmup", str(args.warmup),
               "--groups", str(args.groups), "--window-ms", str(args.window_ms)]
        try:
            run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"bench_beamform: step {step} of case {CASES[case][0]} ran past {STEP_LIMIT_S} s; nothing more is started", file=sys.stderr)
            return 1
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if run.returncode != 0:
            sys.stderr.write(run.stderr[-4000:])
            print(f"bench_beamform: step {step} of case {CASES[case][0]} ended with status {run.returncode}; nothing more is started",
                  file=sys.stderr)
            return 1
        lines += [json.loads(v) for v in run.stdout.splitlines() if v.startswith("{")]
    by = {(r["case"], r["what"]): r for r in lines if r["case"] != "quality"}
    cell = lambda c, w, key, fmt="{}": fmt.format(by[(c, w)][key]) if (c, w) in by and key in by[(c, w)] else "not measured"  # noqa: E731
    names = [c[0] for c in CASES]

    def line(label, what, key, fmt="{}", unit=""):
        return f"| {label} | " + " | ".join(cell(n, what, key, fmt) + (unit if (n, what) in by else "") for n in names) + " |\n"

    def ratio(n):
        return f"{by[(n, 'torch_mvdr')]['ms'] / by[(n, 'adn_mvdr')]['ms']:.1f}" if (n, "torch_mvdr") in by and (n, "adn_mvdr") in by else "not measured"

    block = ("Written by `tools/bench_beamform.py` on one MI355X (device events, windows after a warm-up, median of "
             f"{args.groups}; every step a process of its own); n_fft {N_FFT}, hop {HOP}, every parameter at its default.\n\n"
             "| measurement | one hour, 30 x 2 x 480 000 | one hour, 15 x 4 x 480 000 | one recording, 4 x 24 000 |\n|---|---|---|---|\n"
             + line("`adn_mvdr` (1 launch)", "adn_mvdr", "ms", unit=" ms")
             + line("its memory bound at 8 TB/s (spec read twice)", "adn_mvdr", "mem_bound_ms", unit=" ms")
             + line("share of the memory bound reached", "adn_mvdr", "share_of_mem_bound")
             + line("its FMA bound at 78.6 T FMA/s", "adn_mvdr", "fma_bound_ms", unit=" ms")
             + line("share of the FMA bound reached", "adn_mvdr", "share_of_fma_bound")
             + line("`Beamformer.denoise` (STFT, gain per channel, `adn_mvdr`, resynthesis)", "denoise", "ms", unit=" ms")
             + line("... in seconds of recording per second", "denoise", "audio_s_per_s")
             + line("the operator from torch ops (`einsum`, `torch.linalg.solve`)", "torch_mvdr", "ms", unit=" ms")
             + "| ... as a multiple of `adn_mvdr` | " + " | ".join(ratio(n) for n in names) + " |\n"
             + line("torch composition against `adn_mvdr`, max relative difference", "torch_mvdr", "max_rel_diff_from_adn_mvdr", "{:.3g}"))
    quality = [r for r in lines if r["case"] == "quality"]
    if quality:
        block += ("\nSI-SDR (dB) of `Beamformer.denoise` on the device on the 8 dB recordings of the host block, beside the restatement's "
                  "(device / restatement):\n\n| form | " + " | ".join(f"C = {c}" for c in (2, 4, 8)) + " |\n|---|---|---|---|\n")
        for label, _ in QUALITY_ROWS:
            got = {r["channels"]: r for r in quality if r["what"] == label}
            block += f"| {label} | " + " | ".join(f"{got[c]['si_sdr_device']:.2f} / {got[c]['si_sdr_restatement']:.2f}" if c in got else "–"
                                                   for c in (2, 4, 8)) + " |\n"
    else:
        block += "\nSI-SDR on the device: not measured.\n"
    write_marked_block(args.out, block)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
