#!/usr/bin/env python3
"""Device time of the dereverberation baseline (adn_wpe; Dereverberator.denoise as a whole), the same steps composed from torch
ops on the device (torch.linalg batched over bins) beside them, the kernel's time against its derived bound, and the four SI-SDR
figures on the device.  Buffers are allocated once; device events around a window of calls (at least `--window-ms` long, sized
from a calibration call) after a warm-up, median of `--groups` windows.  One JSON line per measurement, and the same figures as a
table into the marked device block of `--out` (default profiles/bench_dereverb.md):

    adn_wpe             the C entry point on the device's own STFT of reverberant clips.  Bounds: `fma_bound_ms` = the FMAs of the
                        definition, per row I x 4 T (K (K + 1) / 2 + K) for the correlation, I x 4 T K for the filter and
                        I x 4 (K^3 / 6 + K^2) for the solve, at the chip's 78.6 T fp32 FMA/s; `byte_bound_ms` = 20 n T F bytes
                        (8 read once, 8 + 4 written) at 8 TB/s.  Whichever is larger binds; `share_of_bound` is against it.
    denoise             Dereverberator.denoise, device tensor in, device tensor out; `audio_s_per_s`
    torch_wpe           the definition's steps as torch ops on the device: unfold, two batched matmuls, torch.linalg.cholesky,
                        torch.cholesky_solve, one batched matmul per iteration; its difference from adn_wpe's result
    si_sdr              reverberant input, WPE, SpectralDenoiser, WPE then the spectral gain on tests/dereverb_cases.py's clip

Workloads: one hour of 8 kHz audio as 60 clips of 60 s, and one clip of 3 s; the burst signal of tests/baseline_cases.py through
the device's Freeverb (audiodenoiser_amd.reverb).

    python tools/bench_dereverb.py [--cases 0,1] [--out profiles/bench_dereverb.md]

Kernel-level numbers: rocprofv3 --kernel-trace --stats -- python tools/bench_dereverb.py --cases 0 (a run of its own).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import time_ms, write_marked_block  # noqa: E402

HBM_BPS = 8.0e12
FMA_PER_S = 157.3e12 / 2           # peak fp32 vector rate of the MI355X, two flops per FMA
RATE = 8000
N_FFT, HOP = 512, 128
CASES = (("one_hour", 60, 60 * RATE), ("one_clip_3s", 1, 3 * RATE))


def torch_wpe(spec, taps=20, delay=3, iterations=3, loading=1e-3, power_floor=1e-3):
    """The definition of include/adn.h ("dereverb") composed from torch ops, every (clip, bin) row a batch entry."""
    import torch
    n, t, f = spec.shape
    x = spec.transpose(1, 2).reshape(n * f, t)                                   # (B, T)
    xp = torch.nn.functional.pad(torch.view_as_real(x), (0, 0, delay + taps - 1, 0))
    xp = torch.view_as_complex(xp.contiguous())                                  # (B, delay + taps - 1 + T), zeros in front
    # past[b, t, j] = X_{t - delay - j}: window t of the padded row holds X_{t-delay-taps+1} ... X_{t-delay}
    past = xp[:, :t + taps - 1].unfold(1, taps, 1).flip(-1)                      # (B, T, K)
    p = x.real * x.real + x.imag * x.imag
    phi = (power_floor * p.sum(1) / t).clamp_min(1e-30)
    d = x
    eye = torch.eye(taps, dtype=torch.float32, device=spec.device)
    for _ in range(iterations):
        w = 1.0 / torch.maximum(d.real * d.real + d.imag * d.imag, phi[:, None])
        u = (past * w[:, :, None]).transpose(1, 2)                               # (B, K, T)
        r = u @ past.conj()
        pv = u @ x.conj()[:, :, None]
        tr = torch.diagonal(r, dim1=1, dim2=2).real.sum(1)
        a = r + ((loading * tr / taps + 1e-30)[:, None, None] * eye).to(r.dtype)
        g = torch.cholesky_solve(pv, torch.linalg.cholesky(a))
        d = x - (past @ g.conj())[:, :, 0]
        d = torch.cat([x[:, :delay], d[:, delay:]], dim=1)
    return d.reshape(n, f, t).transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1", help="indices into CASES")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_dereverb.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import baseline_cases as bc
    import dereverb_cases as dc
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.baseline import SpectralDenoiser
    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams
    from audiodenoiser_amd.griffin_lim import stft_complex
    from audiodenoiser_amd.metrics import evaluate
    from audiodenoiser_amd.reverb import reverb
    if not torch.cuda.is_available():
        raise SystemExit("bench_dereverb: no ROCm device is visible; nothing is measured without one")
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.adn_prepare(0, N_FFT), "adn_prepare")
    prm = WpeParams()
    K, D, I = prm.taps, prm.delay, prm.iterations
    dn = Dereverberator(dev)
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    wet, dry = dc.quality_case()
    wd, dd = torch.from_numpy(wet.copy()).to(dev), torch.from_numpy(dry.copy()).to(dev)
    score = lambda a: round(float(evaluate(a, dd, sr=RATE)["si_sdr"][0]), 3)  # noqa: E731
    sdr = {"what": "si_sdr", "input": score(wd), "wpe": score(dn.denoise(wd)), "spectral_baseline": score(SpectralDenoiser(dev).denoise(wd)),
           "wpe_then_spectral_baseline": score(Dereverberator(dev, gain=True).denoise(wd)),
           "restatement_float64": [round(float(v), 3) for v in dc.restatement_si_sdr()]}
    emit(sdr)

    for k in (int(v) for v in args.cases.split(",")):
        name, n, length = CASES[k]
        dry_x = torch.from_numpy(np.stack([bc.speech_like(length, 100 + c).astype(np.float32) for c in range(n)])).to(dev)
        x = reverb(dry_x, RATE)
        t, f = 1 + length // HOP, N_FFT // 2 + 1
        spec = stft_complex(x, N_FFT, HOP)
        s = torch.view_as_real(spec)
        out = torch.empty_like(s)
        mag = torch.zeros((n, 1, f, max(t, 16)), device=dev)

        def kernel():
            _lib.check(L.adn_wpe(s.data_ptr(), n, t, f, None, None, 0, out.data_ptr(), mag.data_ptr(), int(mag.shape[3]), st), "adn_wpe")
        row = time_ms(kernel, args.warmup, args.groups, args.window_ms)
        rows = n * f
        fma = rows * I * (4 * t * (K * (K + 1) // 2 + K) + 4 * t * K + 4 * (K ** 3 // 6 + K * K))
        nbytes = 20 * n * t * f
        fma_ms, byte_ms = fma / FMA_PER_S * 1e3, nbytes / HBM_BPS * 1e3
        bound = max(fma_ms, byte_ms)
        emit({"case": name, "what": "adn_wpe", "shape": [n, t, f], "params": [K, D, I], **row, "fma": fma, "fma_bound_ms": round(fma_ms, 4),
              "bytes": nbytes, "byte_bound_ms": round(byte_ms, 4), "binds": "fma" if fma_ms >= byte_ms else "bytes",
              "share_of_bound": round(bound / row["ms"], 4), "workgroups": n * -(-f // 16)})
        whole = time_ms(lambda: dn.denoise(x), args.warmup, args.groups, args.window_ms)
        emit({"case": name, "what": "denoise", "shape": [n, length], **whole, "audio_s_per_s": round(n * length / RATE / (whole["ms"] * 1e-3), 1)})
        try:
            ref = torch_wpe(spec, K, D, I, prm.loading, prm.power_floor)
            got = torch.view_as_complex(out)
            diff = float((got - ref).abs().max() / ref.abs().max())
            del ref
            trow = time_ms(lambda: torch_wpe(spec, K, D, I, prm.loading, prm.power_floor), 1, 3, min(args.window_ms, 100.0))
            emit({"case": name, "what": "torch_wpe", **trow, "max_rel_diff_from_adn_wpe": diff,
                  "times_adn_wpe": round(trow["ms"] / row["ms"], 2)})
        except Exception as exc:  # noqa: BLE001 - reported, the other measurements stand
            emit({"case": name, "what": "torch_wpe", "failed": f"{type(exc).__name__}: {str(exc)[:300]}"})
        del x, dry_x, spec, s, out, mag
        torch.cuda.empty_cache()

    by = {(r.get("case"), r["what"]): r for r in lines}
    cell = lambda c, w, key, fmt="{}": fmt.format(by[(c, w)][key]) if (c, w) in by and key in by[(c, w)] else "not measured"  # noqa: E731
    hour, clip = CASES[0][0], CASES[1][0]
    block = ("Written by `tools/bench_dereverb.py` on one MI355X (device events, windows after a warm-up, median of "
             f"{args.groups}); K {K}, D {D}, I {I}, n_fft {N_FFT}, hop {HOP}.\n\n"
             "| measurement | one hour (60 x 480 000) | one clip (24 000) |\n|---|---|---|\n"
             f"| `adn_wpe` (1 launch) | {cell(hour, 'adn_wpe', 'ms')} ms | {cell(clip, 'adn_wpe', 'ms')} ms |\n"
             f"| its FMA bound (definition's FMAs at 78.6 T FMA/s) | {cell(hour, 'adn_wpe', 'fma_bound_ms')} ms | {cell(clip, 'adn_wpe', 'fma_bound_ms')} ms |\n"
             f"| its byte bound (20 n T F bytes at 8 TB/s) | {cell(hour, 'adn_wpe', 'byte_bound_ms')} ms | {cell(clip, 'adn_wpe', 'byte_bound_ms')} ms |\n"
             f"| what binds; share of that bound | {cell(hour, 'adn_wpe', 'binds')}; {cell(hour, 'adn_wpe', 'share_of_bound')} | {cell(clip, 'adn_wpe', 'binds')}; {cell(clip, 'adn_wpe', 'share_of_bound')} |\n"
             f"| workgroups | {cell(hour, 'adn_wpe', 'workgroups')} | {cell(clip, 'adn_wpe', 'workgroups')} |\n"
             f"| `Dereverberator.denoise`, device tensor in and out | {cell(hour, 'denoise', 'ms')} ms = {cell(hour, 'denoise', 'audio_s_per_s')} s of audio per s | {cell(clip, 'denoise', 'ms')} ms = {cell(clip, 'denoise', 'audio_s_per_s')} s/s |\n"
             f"| the same steps from torch ops (`torch.linalg` batched over bins) | {cell(hour, 'torch_wpe', 'ms')} ms ({cell(hour, 'torch_wpe', 'times_adn_wpe')} x `adn_wpe`) | {cell(clip, 'torch_wpe', 'ms')} ms ({cell(clip, 'torch_wpe', 'times_adn_wpe')} x) |\n"
             f"| torch composition against `adn_wpe`, max relative difference | {cell(hour, 'torch_wpe', 'max_rel_diff_from_adn_wpe', '{:.3g}')} | {cell(clip, 'torch_wpe', 'max_rel_diff_from_adn_wpe', '{:.3g}')} |\n\n"
             + "".join(f"torch composition, {c}: {by[(c, 'torch_wpe')]['failed']}\n\n" for c in (hour, clip)
                       if (c, "torch_wpe") in by and "failed" in by[(c, "torch_wpe")])
             + "SI-SDR against the dry signal on the device (`metrics.evaluate`), the clip of the host block:\n\n"
             "| path | device | float64 restatement |\n|---|---|---|\n"
             + "".join(f"| {label} | {sdr[key]} dB | {sdr['restatement_float64'][i]} dB |\n" for i, (label, key) in enumerate(
                 (("reverberant input", "input"), ("WPE", "wpe"), ("spectral baseline alone", "spectral_baseline"),
                  ("WPE, then spectral baseline", "wpe_then_spectral_baseline")))))
    write_marked_block(args.out, block)


if __name__ == "__main__":
    main()
