#!/usr/bin/env python3
"""Time of one tick of EchoStreamPool (n_fft 512, hop 128, block 4, defaults), host included, beside the lockstep forms of the same work:

    solo      the same calls as that many StreamEchoCanceller(pairs=1) objects: the only way to serve calls with independent timing
              before the pool took them, and the number to beat;
    lockstep  ONE StreamEchoCanceller of all pairs: every call starts, advances and ends together, which no call server can
              assume.  At mics > 1 it has mics pairs per call and is fed the call's far end mics times: what the pool's shared far
              end saves shows against it.

Cases: 64 calls at mics = 1 (pool, solo, lockstep); 64 calls at mics = 4 (pool, lockstep of 256 pairs); one call at mics = 1 (pool,
solo).  Then the C call alone, adn_aec_stream_pool at 1 / 64 / 128 calls of one microphone and 8 / 16 / 32 taps beside adn_aec_stream
on the same pairs: seeded ring cells and windows at a carried step, no analyze and no emit.

Device events around a window of calls (tools/bench_common.py's time_ms: at least `--window-ms` long, after a warm-up, median of
`--groups` windows).  The tick that is timed is a steady-state one (step 8) of seeded uniform audio; calling it again reads the same
samples and windows.  The echo states do move from call to call; the time does not depend on the values.  One JSON line per case:

    python tools/bench_echo_pool.py [--write profiles] [--commit ID]
"""
import argparse
import ctypes
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
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--write", default=None, help="directory for bench_echo_pool.jsonl and the device block of bench_echo_pool.md")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import torch
    from audiodenoiser_amd import _lib, build
    from audiodenoiser_amd._host import current_stream
    from audiodenoiser_amd.echo import AecParams, EchoStreamPool, StreamEchoCanceller
    from audiodenoiser_amd.stream import POOL_MAX_ROWS, end_of
    if not torch.cuda.is_available():
        raise SystemExit("bench_echo_pool: no ROCm device is visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    block, records = args.block, []
    kw = dict(block_frames=block)

    def timed(fn):
        return time_ms(fn, args.warmup, args.groups, args.window_ms)

    def audio_of(n, channels, seed, plan):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.rand((n, channels, end_of(plan, STEP)), generator=g, device=dev) - 0.5

    def lockstep_at_step(flat):
        """A StreamEchoCanceller over `flat` (2 pairs, L) whose steps 0 ... STEP - 1 have run -> the tick of step STEP."""
        sd = StreamEchoCanceller(dev, pairs=flat.shape[0] // 2, **kw)
        total = flat.shape[1]
        base = end_of(sd._plan, STEP - 1)
        sd.push(flat[:, :base].contiguous())
        assert sd._done == STEP and sd._fill == 0, (sd._done, sd._fill)
        rest = flat[:, base:].contiguous()
        return lambda: sd.emit(sd._net(sd.analyze(rest, total - base, STEP, 1), STEP, 1), STEP, 1)

    def pairs_of(audio):
        """(calls, mics + 1, L) -> (2 calls mics, L): microphone, far end, microphone, far end ...: the far end mics times."""
        n, c, total = audio.shape
        m = c - 1
        return torch.stack([audio[:, :m], audio[:, m:].expand(n, m, total)], dim=2).reshape(2 * n * m, total)

    def pool_at_step(pool, audio):
        """`pool` with every call of `audio` open and steps 0 ... STEP - 1 run, the samples of step STEP in the rings -> the device
        work of the tick of step STEP as StreamPool.step does it (the book is left where it is)."""
        n, c, total = audio.shape
        cids, pos = [pool.open() for _ in range(n)], 0
        for step in range(STEP + 1):
            end = end_of(pool.book.plan, step)
            for i, r in enumerate(cids):
                pool.push(r, audio[i, :, pos:end].contiguous())
            pos = end
            if step < STEP:
                assert len(pool.step()) == n
        rows = pool.book.rows()
        assert rows == [(r, STEP, -1) for r in cids]
        srows = pool.book.stream_rows(rows)
        per = POOL_MAX_ROWS // c * c

        def tick():
            x = torch.cat([pool.analyze(srows[i:i + per]) for i in range(0, len(srows), per)])
            y, erows = pool._net(x, srows), pool._emit_rows(srows)
            return [pool.emit(y[i:i + POOL_MAX_ROWS], erows[i:i + POOL_MAX_ROWS]) for i in range(0, len(erows), POOL_MAX_ROWS)]
        return tick

    for n, mics, with_solo in ((64, 1, True), (64, 4, False), (1, 1, True)):
        pool = EchoStreamPool(dev, n, mics, **kw)
        audio = audio_of(n, mics + 1, 1000 * mics + n, pool.book.plan)
        t_pool = timed(pool_at_step(pool, audio))
        block_s = block * pool.book.hop_length / pool.book.sample_rate
        rec = {"case": "tick", "calls": n, "mics": mics, "streams": n * (mics + 1), "lockstep_pairs": n * mics, "block": block,
               "pool_ms": t_pool["ms"], "pool_min_max": [t_pool["ms_min"], t_pool["ms_max"]],
               "real_time_factor": round(n * block_s / (t_pool["ms"] * 1e-3), 1), "groups": args.groups}
        if with_solo:
            solos = [lockstep_at_step(pairs_of(audio[i:i + 1])) for i in range(n)]

            def solo_tick():
                for fn in solos:
                    fn()
            t_solo = timed(solo_tick)
            rec.update(solo_ms=t_solo["ms"], solo_min_max=[t_solo["ms_min"], t_solo["ms_max"]], solo_over_pool=round(t_solo["ms"] / t_pool["ms"], 2))
            del solos
        if n > 1:
            t_one = timed(lockstep_at_step(pairs_of(audio)))
            rec.update(lockstep_ms=t_one["ms"], lockstep_min_max=[t_one["ms_min"], t_one["ms_max"]],
                       pool_over_lockstep=round(t_pool["ms"] / t_one["ms"], 2))
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del pool
        torch.cuda.empty_cache()

    # the C call alone, beside adn_aec_stream on the same pairs: a carried step on seeded cells
    L, E, C = _lib.load(), _lib.load_echo(), _lib.load_call()
    plan, st = (512, 128, 16, block, 0), current_stream(dev)
    f, step = 257, 3
    need = ctypes.c_size_t(0)
    for taps, forget in ((8, 0.995), (16, 0.97), (32, 0.984375)):
        p = AecParams(taps=taps, forget=forget).to_struct()
        for n in (1, 64, 128):
            g = torch.Generator(device=dev).manual_seed(taps + n)
            ring = 4096
            _lib.check(L.adn_stream_pool_state_bytes(2 * n, *plan, ring, ctypes.byref(need)), "adn_stream_pool_state_bytes")
            pstate = (torch.rand(need.value // 4, generator=g, device=dev) - 0.5).view(torch.uint8)
            _lib.check(L.adn_stream_state_bytes(2 * n, *plan, 1, ctypes.byref(need)), "adn_stream_state_bytes")
            sstate = (torch.rand(need.value // 4, generator=g, device=dev) - 0.5).view(torch.uint8)
            _lib.check_echo(E.adn_aec_stream_state_bytes(n, f, ctypes.byref(p), ctypes.byref(need)), "adn_aec_stream_state_bytes")
            astates = [torch.zeros(need.value, dtype=torch.uint8, device=dev) for _ in range(2)]
            y = torch.rand((2 * n, 1, f, 16), generator=g, device=dev)
            rows = (_lib.StreamPoolRow * (2 * n))(*[_lib.StreamPoolRow(s, step, -1) for s in range(2 * n)])

            def pool_call():
                _lib.check_call(C.adn_aec_stream_pool(pstate.data_ptr(), pstate.numel(), 2 * n, 1, *plan, ring, rows, 2 * n, y.data_ptr(),
                                                      ctypes.byref(p), astates[0].data_ptr(), astates[0].numel(), st), "adn_aec_stream_pool")

            def lock_call():
                _lib.check_echo(E.adn_aec_stream(sstate.data_ptr(), sstate.numel(), y.data_ptr(), 2 * n, step, 1, -1, *plan, 1,
                                                 ctypes.byref(p), astates[1].data_ptr(), astates[1].numel(), st), "adn_aec_stream")
            t_p, t_l = timed(pool_call), timed(lock_call)
            rec = {"case": "call", "calls": n, "mics": 1, "taps": taps, "block": block, "pool_call_ms": t_p["ms"],
                   "pool_call_min_max": [t_p["ms_min"], t_p["ms_max"]], "lockstep_call_ms": t_l["ms"],
                   "lockstep_call_min_max": [t_l["ms_min"], t_l["ms_max"]], "pool_over_lockstep": round(t_p["ms"] / t_l["ms"], 2),
                   "groups": args.groups}
            records.append(rec)
            print(json.dumps(rec), flush=True)

    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_echo_pool.jsonl"), "w") as fh:
            for r in records:
                fh.write(json.dumps(dict(r, commit=args.commit, library_digest=digest[:16])) + "\n")
        text = (f"Written by `tools/bench_echo_pool.py` on one MI355X (device events around windows of whole ticks, host included, after "
                f"a warm-up, median of {args.groups}); n_fft 512, hop 128, block {block}: one tick is {block} frames of every call; defaults.  "
                "solo: one `StreamEchoCanceller(pairs=1)` per call.  lockstep: one `StreamEchoCanceller` of calls x mics pairs, the far "
                "end fed once per microphone.\n\n"
                "| calls | mics | pool tick | solo objects | solo / pool | one lockstep object | pool / lockstep | real time |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for r in (r for r in records if r["case"] == "tick"):
            solo = f"{r['solo_ms']:.4f} ms | {r['solo_over_pool']:.2f}" if "solo_ms" in r else "not measured | not measured"
            lock = f"{r['lockstep_ms']:.4f} ms | {r['pool_over_lockstep']:.2f}" if "lockstep_ms" in r else "the solo object | --"
            text += f"| {r['calls']} | {r['mics']} | {r['pool_ms']:.4f} ms | {solo} | {lock} | {r['real_time_factor']} x |\n"
        text += ("\nThe C call alone at a carried step (no analyze, no emit), one microphone per call, beside `adn_aec_stream` on the same "
                 "pairs:\n\n| taps | calls | `adn_aec_stream_pool` | `adn_aec_stream` | pool / lockstep |\n|---|---|---|---|---|\n")
        for r in (r for r in records if r["case"] == "call"):
            text += f"| {r['taps']} | {r['calls']} | {r['pool_call_ms']:.4f} ms | {r['lockstep_call_ms']:.4f} ms | {r['pool_over_lockstep']:.2f} |\n"
        write_marked_block(os.path.join(args.write, "bench_echo_pool.md"), text)


if __name__ == "__main__":
    main()
