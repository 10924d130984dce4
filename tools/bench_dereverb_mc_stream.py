#!/usr/bin/env python3
"""Device time of the streaming multichannel dereverberator (adn_wpe_mc_stream; StreamDereverberator(channels=C)): one step of four
frames of 1 / 64 / 128 recordings at (C, K) = (2, 16) and (4, 8) (n_fft 512, hop 128, window 16, the default parameters), beside
the single-channel adn_wpe_stream at K = 20 on the SAME number of streams (the yardstick: what those microphones cost today), and
beside the same block composed from torch ops batched over (recording, bin); the whole tick (analyse, WPE, emit) of
StreamDereverberator(channels=2); SI-SDR of the rows of tests/dereverb_mc_stream_cases.TABLE on the device beside the restatement's.

Device events around a window of calls (at least `--window-ms` long, sized from a calibration call) after a warm-up, median of
`--groups` windows, the calls that are compared alternating group by group (tools/bench_denoise.py's time_ms).  The step that is
timed is a steady-state one (step 32) of seeded uniform audio; calling it again and again reads the same ring cells.  The WPE state
and the ring cells it rewrites do move from call to call (it is a recursion, and d goes back in place); its time does not depend
on the values.  Before timing, the torch form and adn_wpe_mc_online are compared on the same 40 frames from a fresh start: the
largest difference relative to the largest |d| is reported (two float32 evaluations of one recursion: a floor of its own, not a
bound).  One JSON line per record:

    step    per (C, K) and recordings: c_call_ms (adn_wpe_mc_stream itself), single_ms (adn_wpe_stream, K = 20, the same streams),
            state_bytes (read + written), state_bound_ms (those bytes at 8 TB/s), chain (the per-lane dependent FMAs of a frame by
            the kernel's cost model, and the single-channel kernel's), composed_ms (the torch form of the same block)
    tick    per recordings at C = 2: analyze_ms, emit_ms, tick_ms, real_time_factor = recordings x (block hop / sample_rate) / tick
    si_sdr  per row of the table: the device's and the restatement's SI-SDR per channel

    python tools/bench_dereverb_mc_stream.py [--write profiles] [--commit ID]
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


def chain_fmas(channels, taps):
    """The dependent complex FMAs one lane runs per frame (the cost model in the kernel's header): u, e (lanes c < C; not at C = 1,
    where every lane forms e: K), q, both sides of the branch of the P update, the G update."""
    n = channels * taps
    return n + n + n + 2 * n + channels


class TorchRlsJoint:
    """The recursion of adn.h ("dereverb stream multichannel") from torch ops, batched over rows (recording x bin): state G (R, C, N),
    P (R, N, N), s (R,), past (R, C, D + K - 1)."""

    def __init__(self, rows, channels, params, dev):
        import torch
        self.C, self.K, self.D = channels, params.taps, params.delay
        self.N = channels * params.taps
        self.alpha, self.rho, self.beta = params.forget, params.power_floor, params.smooth
        self.G = torch.zeros((rows, channels, self.N), dtype=torch.complex64, device=dev)
        self.P = torch.eye(self.N, dtype=torch.complex64, device=dev).repeat(rows, 1, 1) / params.loading
        self.s = torch.zeros(rows, device=dev)
        self.past = torch.zeros((rows, channels, self.D + self.K - 1), dtype=torch.complex64, device=dev)
        self.low = torch.tril(torch.ones((self.N, self.N), dtype=torch.bool, device=dev))
        self.first = True

    def block(self, x):
        """x (R, C, B) complex64, the next B frames of every row -> d (R, C, B)."""
        import torch
        out = torch.empty_like(x)
        for t in range(x.shape[2]):
            xt = x[:, :, t]
            p = (xt.real * xt.real + xt.imag * xt.imag).sum(1) / self.C
            self.s = p if self.first else self.beta * self.s + (1.0 - self.beta) * p
            self.first = False
            phi = torch.clamp(self.rho * self.s, min=1e-30)
            taps = self.past[:, :, :self.K].flip(2).reshape(-1, self.N)      # r = c K + j: X_{t-D-j, c}
            e = xt - torch.einsum("rcn,rn->rc", self.G.conj(), taps)
            lam = torch.maximum((e.real * e.real + e.imag * e.imag).sum(1) / self.C, phi)
            u = torch.einsum("rjk,rk->rj", self.P, taps)
            den = self.alpha * lam + (taps.conj() * u).sum(1).real
            k = u / den[:, None]
            Pn = (self.P - k[:, :, None] * u.conj()[:, None, :]) / self.alpha
            Pn = torch.where(self.low, Pn, Pn.transpose(1, 2).conj())
            d = torch.diagonal(Pn, dim1=1, dim2=2)
            d.copy_(torch.complex(d.real, torch.zeros_like(d.real)))
            self.P = Pn
            self.G = self.G + k[:, None, :] * e.conj()[:, :, None]
            self.past = torch.cat([self.past[:, :, 1:], xt[:, :, None]], dim=2)
            out[:, :, t] = e
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", default="1,64,128")
    ap.add_argument("--shapes", default="2x16,4x8", help="(C, K) pairs as CxK")
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--sample-rate", type=int, default=8000)
    ap.add_argument("--write", default=None, help="directory for bench_dereverb_mc_stream.jsonl and the device block of bench_dereverb_mc_stream.md")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import torch
    from audiodenoiser_amd import _lib, build
    from audiodenoiser_amd.dereverb import (StreamDereverberator, WpeStreamParams, wpe_online_joint, wpe_stream_state_bytes,
                                            wpe_stream_state_bytes_joint)
    from audiodenoiser_amd.griffin_lim import stft_complex
    from audiodenoiser_amd.metrics import evaluate
    from audiodenoiser_amd.stream import end_of
    from bench_denoise import time_ms
    import dereverb_mc_cases as mc
    import dereverb_mc_stream_cases as msc
    if not torch.cuda.is_available():
        raise SystemExit("bench_dereverb_mc_stream: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    records = []
    block = args.block
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

    def at_step(n_streams, channels, params, seed):
        """A lockstep object whose steps 0 ... STEP - 1 have run on seeded audio, and the analysed windows of step STEP."""
        sd = StreamDereverberator(dev, n_streams=n_streams, channels=channels, block_frames=block, params=params,
                                  sample_rate=args.sample_rate)
        g = torch.Generator(device=dev).manual_seed(seed)
        base, total = end_of(sd._plan, STEP - 1), end_of(sd._plan, STEP)
        audio = torch.rand((n_streams, total), generator=g, device=dev) - 0.5
        sd.push(audio[:, :base].contiguous())
        assert sd._done == STEP and sd._fill == 0, (sd._done, sd._fill)
        rest = audio[:, base:].contiguous()
        return sd, rest, sd.analyze(rest, total - base, STEP, 1)

    for channels, taps in shapes:
        params = WpeStreamParams(taps=taps)
        # the torch form against adn_wpe_mc_online: 40 frames of three recordings from a fresh start
        spec = stft_complex(torch.from_numpy(msc.parity_audio(512, 40, channels).copy()).to(dev), 512, 128)
        d_dev, _, _ = wpe_online_joint(spec, channels, params=params)
        rls = TorchRlsJoint(3 * 257, channels, params, dev)
        x = spec.view(3, channels, 40, 257).permute(0, 3, 1, 2).reshape(3 * 257, channels, 40)
        d_torch = rls.block(x).reshape(3, 257, channels, 40).permute(0, 2, 3, 1).reshape(3 * channels, 40, 257)
        composed_diff = float((d_torch - d_dev).abs().max() / d_dev.abs().max())
        for n in (int(v) for v in args.recordings.split(",")):
            streams = n * channels
            sd, _, win = at_step(streams, channels, params, 1000 * channels + n)
            single, _, win1 = at_step(streams, 1, None, 1000 * channels + n)
            f = sd.n_bins
            pj, p1 = ctypes.byref(sd.params.to_struct()), ctypes.byref(single.params.to_struct())

            def joint_c():
                _lib.check(lib.adn_wpe_mc_stream(sd._state.data_ptr(), sd._state.numel(), win.data_ptr(), streams, channels, STEP, 1, -1,
                                                 *sd._plan, sd.max_steps, pj, sd._wpe_state.data_ptr(), sd._wpe_state.numel(), st),
                           "adn_wpe_mc_stream")

            def single_c():
                _lib.check(lib.adn_wpe_stream(single._state.data_ptr(), single._state.numel(), win1.data_ptr(), streams, STEP, 1, -1,
                                              *single._plan, single.max_steps, p1, single._wpe_state.data_ptr(),
                                              single._wpe_state.numel(), st), "adn_wpe_stream")

            rls = TorchRlsJoint(n * f, channels, params, dev)
            g = torch.Generator(device=dev).manual_seed(7 + n)
            frames = (torch.rand((n * f, channels, block), generator=g, device=dev) - 0.5).to(torch.complex64)
            times = time_ms([joint_c, single_c, lambda: rls.block(frames)], args.warmup, args.groups, args.window_ms)
            med = [round(t[0], 4) for t in times]
            state_bytes = 2 * wpe_stream_state_bytes_joint(n, channels, f, params)
            single_bytes = 2 * wpe_stream_state_bytes(streams, f)
            rec = {"record": "step", "channels": channels, "taps": taps, "recordings": n, "streams": streams, "block": block,
                   "workgroups": n * -(-f // 8), "single_workgroups": streams * -(-f // 8),
                   "c_call_ms": med[0], "c_call_ms_min_max": [round(times[0][1], 4), round(times[0][2], 4)],
                   "single_ms": med[1], "single_ms_min_max": [round(times[1][1], 4), round(times[1][2], 4)],
                   "joint_over_single": round(med[0] / med[1], 2),
                   "us_per_frame": round(med[0] * 1e3 / block, 2), "single_us_per_frame": round(med[1] * 1e3 / block, 2),
                   "chain_fmas": chain_fmas(channels, taps), "single_chain_fmas": 5 * 20 + 1,
                   "state_bytes": state_bytes, "state_bound_ms": round(state_bytes / HBM_BPS * 1e3, 5),
                   "share_of_bound": round(state_bytes / HBM_BPS * 1e3 / med[0], 4), "single_state_bytes": single_bytes,
                   "composed_ms": med[2], "composed_over_c_call": round(med[2] / med[0], 1), "composed_max_rel_diff": composed_diff,
                   "calls_per_window": [t[3] for t in times], "groups": args.groups}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            if channels == 2:
                y = win.clone()
                rest = at_step(streams, channels, params, 1000 * channels + n)      # an object of its own: emit moves the tail
                sd2, audio2 = rest[0], rest[1]

                def tick():
                    xw = sd2.analyze(audio2, audio2.shape[1], STEP, 1)
                    return sd2.emit(sd2._net(xw, STEP, 1), STEP, 1)

                tt = time_ms([lambda: sd2.analyze(audio2, audio2.shape[1], STEP, 1), lambda: sd2.emit(y, STEP, 1), tick],
                             args.warmup, args.groups, args.window_ms)
                block_s = block * sd2.hop_length / args.sample_rate
                rec = {"record": "tick", "channels": channels, "taps": taps, "recordings": n, "streams": streams,
                       "analyze_ms": round(tt[0][0], 4), "emit_ms": round(tt[1][0], 4), "tick_ms": round(tt[2][0], 4),
                       "tick_ms_min_max": [round(tt[2][1], 4), round(tt[2][2], 4)], "block_s": block_s,
                       "real_time_factor": round(n * block_s / (tt[2][0] * 1e-3), 1)}
                records.append(rec)
                print(json.dumps(rec), flush=True)
                del sd2, audio2, y
            del sd, single, win, win1, rls, frames
            torch.cuda.empty_cache()

    # SI-SDR of the table's rows on the device, fed 1024 samples at a time
    dry = None
    for label, channels, taps, gain in (("input", 2, None, False),) + msc.TABLE:
        wet, dry = mc.recording(channels or 1)
        xd = torch.from_numpy(wet.copy()).to(dev)
        dd = torch.from_numpy(dry.copy()).to(dev)[None].expand(xd.shape[0], -1).contiguous()
        if label == "input":
            out = xd
        else:
            sd = StreamDereverberator(dev, n_streams=xd.shape[0], channels=channels or 1, params=WpeStreamParams(taps=taps), gain=gain)
            outs = [sd.push(xd[:, i:i + 1024]) for i in range(0, xd.shape[1], 1024)]
            outs.append(sd.flush())
            out = torch.cat(outs, dim=1)
        rec = {"record": "si_sdr", "form": label, "stacked": (channels or 1) * (taps or 0),
               "device": [round(float(v), 3) for v in evaluate(out, dd, sr=args.sample_rate)["si_sdr"]],
               "restatement": [round(v, 3) for v in msc.restatement_si_sdr(label)]}
        records.append(rec)
        print(json.dumps(rec), flush=True)

    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_dereverb_mc_stream.jsonl"), "w") as fh:
            for r in records:
                fh.write(json.dumps(dict(r, commit=args.commit, library_digest=digest[:16])) + "\n")
        text = (f"Written by `tools/bench_dereverb_mc_stream.py` on one MI355X (device events, windows after a warm-up, median of "
                f"{args.groups}, the joint and the single-channel call alternating); D 3, n_fft 512, hop 128, block {block}: one step "
                f"is {block} frames of every stream.  The yardstick is `adn_wpe_stream` at K = 20 on the same C x recordings streams.\n\n"
                "| (C, K) | recordings (streams) | `adn_wpe_mc_stream` | per frame | `adn_wpe_stream`, K 20, same streams | joint / single | "
                "chain FMAs per lane and frame (joint; single) | state read + written; share of its 8 TB/s bound | torch ops |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        for r in (r for r in records if r["record"] == "step"):
            text += (f"| ({r['channels']}, {r['taps']}) | {r['recordings']} ({r['streams']}) | {r['c_call_ms']:.4f} ms | {r['us_per_frame']:.1f} us | "
                     f"{r['single_ms']:.4f} ms | {r['joint_over_single']:.2f} | {r['chain_fmas']}; {r['single_chain_fmas']} | "
                     f"{r['state_bytes'] / 1e6:.2f} MB; {r['share_of_bound']:.3f} | {r['composed_ms']:.2f} ms ({r['composed_over_c_call']} x; "
                     f"differs by {r['composed_max_rel_diff']:.2g}) |\n")
        text += ("\nThe whole tick of `StreamDereverberator(channels=2)` (analyse, WPE, emit; host included):\n\n"
                 "| recordings | analyse / emit | tick | real time |\n|---|---|---|---|\n")
        for r in (r for r in records if r["record"] == "tick"):
            text += (f"| {r['recordings']} | {r['analyze_ms']:.4f} / {r['emit_ms']:.4f} ms | {r['tick_ms']:.4f} ms | "
                     f"{r['real_time_factor']} x |\n")
        text += ("\nSI-SDR against the dry signal per channel on the device (`metrics.evaluate`), `StreamDereverberator` fed 1024 "
                 "samples at a time, the recording of the host block:\n\n| form | device | float64 restatement |\n|---|---|---|\n")
        fmt = lambda v: " / ".join(f"{s:.2f}" for s in v)  # noqa: E731
        for r in (r for r in records if r["record"] == "si_sdr"):
            text += f"| {r['form']} | {fmt(r['device'])} | {fmt(r['restatement'])} |\n"
        write_marked_block(os.path.join(args.write, "bench_dereverb_mc_stream.md"), text)


if __name__ == "__main__":
    main()
