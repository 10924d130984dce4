#!/usr/bin/env python3
"""Time of one tick of the pools of RECORDINGS (BeamformStreamPool; DereverbStreamPool(channels=C) at taps = 32 // C): 1, 16 and 64
recordings of 2, 4 and 8 channels (n_fft 512, hop 128, block 4), host included, beside the two lockstep forms of the same work:

    solo      the same recordings as that many lockstep objects of ONE recording each (StreamBeamformer / StreamDereverberator with
              n_streams = channels): the only way to serve recordings with independent timing before the pools took them, and the
              number to beat;
    lockstep  ONE lockstep object of that many groups: every recording starts, advances and ends together, which a server of
              many rooms cannot assume; the floor the pool can approach, not beat.

For the beamformer it also times adn_stream_pool_emit on all rows of the tick against the first row of each recording, which is
what the pool emits: `skipped_share` = (emit_all - emit_kept) / (tick + emit_all - emit_kept), the share of a tick that emitted
every row that the C - 1 unused rows would cost (the lockstep profile, profiles/bench_beamform_stream.md, records at most 11.7 %:
128 recordings of 8 channels).

Device events around a window of calls (tools/bench_common.py's time_ms: at least `--window-ms` long, after a warm-up, median of
`--groups` windows).  The tick that is timed is a steady-state one (step 8) of seeded uniform audio; calling it again reads the same
samples, ring cells and windows.  The operator states do move from call to call; the time does not depend on the values.  One JSON
line per (operator, channels, recordings):

    python tools/bench_stream_pool_mc.py [--write profiles] [--commit ID]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_common import time_ms, write_marked_block  # noqa: E402

STEP = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", default="1,16,64")
    ap.add_argument("--channels", default="2,4,8")
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--write", default=None, help="directory for bench_stream_pool_mc.jsonl and the device block of bench_stream_pool_mc.md")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import torch
    from audiodenoiser_amd import build
    from audiodenoiser_amd.beamform import BeamformStreamPool, StreamBeamformer
    from audiodenoiser_amd.dereverb import DereverbStreamPool, StreamDereverberator
    from audiodenoiser_amd.stream import POOL_MAX_ROWS, end_of
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_pool_mc: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    block, records = args.block, []

    def audio_of(n, channels, seed, plan):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.rand((n, channels, end_of(plan, STEP)), generator=g, device=dev) - 0.5

    def lockstep_at_step(make, audio):
        """A lockstep object over `audio` (recordings, C, L) whose steps 0 ... STEP - 1 have run -> the tick of step STEP."""
        n, c, total = audio.shape
        sd = make(n * c, c)
        base = end_of(sd._plan, STEP - 1)
        flat = audio.reshape(n * c, total)
        sd.push(flat[:, :base].contiguous())
        assert sd._done == STEP and sd._fill == 0, (sd._done, sd._fill)
        rest = flat[:, base:].contiguous()
        return lambda: sd.emit(sd._net(sd.analyze(rest, total - base, STEP, 1), STEP, 1), STEP, 1)

    def pool_at_step(pool, audio):
        """`pool` with every recording of `audio` open and steps 0 ... STEP - 1 run, the samples of step STEP in the rings -> the
        device work of the tick of step STEP as StreamPool.step does it (the book is left where it is), and its parts."""
        n, c, total = audio.shape
        rids, pos = [pool.open() for _ in range(n)], 0
        for step in range(STEP + 1):                         # the samples of a step, then the step; the last one is left ready
            end = end_of(pool.book.plan, step)
            for i, r in enumerate(rids):
                pool.push(r, audio[i, :, pos:end].contiguous())
            pos = end
            if step < STEP:
                assert len(pool.step()) == n
        rows = pool.book.rows()
        assert rows == [(r, STEP, -1) for r in rids]
        srows = pool.book.stream_rows(rows)
        per = POOL_MAX_ROWS // c * c

        def analyze():
            return torch.cat([pool.analyze(srows[i:i + per]) for i in range(0, len(srows), per)])

        def emit(y, erows):
            return [pool.emit(y[i:i + POOL_MAX_ROWS], erows[i:i + POOL_MAX_ROWS]) for i in range(0, len(erows), POOL_MAX_ROWS)]

        def tick():
            return emit(pool._net(analyze(), srows), pool._emit_rows(srows))
        return tick, analyze, emit, srows

    for name in ("beamform", "dereverb"):
        for channels in (int(v) for v in args.channels.split(",")):
            for n in (int(v) for v in args.recordings.split(",")):
                kw = dict(block_frames=block)
                if name == "beamform":
                    pool = BeamformStreamPool(dev, n, channels, **kw)
                    make = lambda streams, c: StreamBeamformer(dev, n_streams=streams, channels=c, **kw)  # noqa: E731
                else:
                    pool = DereverbStreamPool(dev, max_streams=n, channels=channels, **kw)
                    make = lambda streams, c: StreamDereverberator(dev, n_streams=streams, channels=c, **kw)  # noqa: E731
                audio = audio_of(n, channels, 1000 * channels + n, pool.book.plan)
                tick, analyze, emit, srows = pool_at_step(pool, audio)
                solos = [lockstep_at_step(make, audio[i:i + 1]) for i in range(n)]
                one = lockstep_at_step(make, audio)

                def solo_tick():
                    for fn in solos:
                        fn()
                t_pool, t_solo, t_one = (time_ms(fn, args.warmup, args.groups, args.window_ms) for fn in (tick, solo_tick, one))
                block_s = block * pool.book.hop_length / pool.book.sample_rate
                rec = {"operator": name, "channels": channels, "recordings": n, "streams": n * channels, "block": block,
                       "taps": pool.params.taps if name == "dereverb" else None,
                       "calls": -(-n // (POOL_MAX_ROWS // channels)),
                       "pool_ms": t_pool["ms"], "pool_min_max": [t_pool["ms_min"], t_pool["ms_max"]],
                       "solo_ms": t_solo["ms"], "solo_min_max": [t_solo["ms_min"], t_solo["ms_max"]],
                       "lockstep_ms": t_one["ms"], "lockstep_min_max": [t_one["ms_min"], t_one["ms_max"]],
                       "solo_over_pool": round(t_solo["ms"] / t_pool["ms"], 2), "pool_over_lockstep": round(t_pool["ms"] / t_one["ms"], 2),
                       "real_time_factor": round(n * block_s / (t_pool["ms"] * 1e-3), 1), "groups": args.groups}
                if name == "beamform":
                    y = analyze()
                    kept_y, kept_rows = y[::channels].contiguous(), srows[::channels]
                    e_all = time_ms(lambda: emit(y, srows), args.warmup, args.groups, args.window_ms)
                    e_kept = time_ms(lambda: emit(kept_y, kept_rows), args.warmup, args.groups, args.window_ms)
                    saved = e_all["ms"] - e_kept["ms"]
                    rec.update(emit_all_ms=e_all["ms"], emit_kept_ms=e_kept["ms"], skipped_share=round(saved / (t_pool["ms"] + saved), 3))
                records.append(rec)
                print(json.dumps(rec), flush=True)
                del pool, solos, one, tick, analyze, emit
                torch.cuda.empty_cache()

    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_stream_pool_mc.jsonl"), "w") as fh:
            for r in records:
                fh.write(json.dumps(dict(r, commit=args.commit, library_digest=digest[:16])) + "\n")
        text = (f"Written by `tools/bench_stream_pool_mc.py` on one MI355X (device events around windows of whole ticks, host included, "
                f"after a warm-up, median of {args.groups}); n_fft 512, hop 128, block {block}: one tick is {block} frames of every "
                "recording; defaults, `taps = 32 // C` for WPE.  solo: one lockstep object per recording.  lockstep: one lockstep "
                "object of all recordings.\n")
        for name, title in (("beamform", "`BeamformStreamPool`"), ("dereverb", "`DereverbStreamPool(channels=C)`")):
            text += (f"\n{title}:\n\n| C | recordings (streams) | pool tick | solo objects | solo / pool | one lockstep object | pool / lockstep | "
                     "real time |" + (" emit, all rows | emit, kept rows | skipped share |" if name == "beamform" else "") + "\n"
                     "|---|---|---|---|---|---|---|---|" + ("---|---|---|" if name == "beamform" else "") + "\n")
            for r in (r for r in records if r["operator"] == name):
                text += (f"| {r['channels']} | {r['recordings']} ({r['streams']}) | {r['pool_ms']:.4f} ms | {r['solo_ms']:.4f} ms | "
                         f"{r['solo_over_pool']:.2f} | {r['lockstep_ms']:.4f} ms | {r['pool_over_lockstep']:.2f} | {r['real_time_factor']} x |")
                if name == "beamform":
                    text += f" {r['emit_all_ms']:.4f} ms | {r['emit_kept_ms']:.4f} ms | {r['skipped_share']:.3f} |"
                text += "\n"
        write_marked_block(os.path.join(args.write, "bench_stream_pool_mc.md"), text)


if __name__ == "__main__":
    main()
