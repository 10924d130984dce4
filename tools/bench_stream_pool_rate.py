#!/usr/bin/env python3
"""A round of live feeds at their own rates through one StreamPool (audiodenoiser_amd/stream.py): every stream pushes 10 ms of
audio at its rate, then the pool ticks once.  Two forms, same process, same model, same card, the same samples:

    rate      the pool takes the rates itself: StreamPool(input_rates=...), one push_many (one staging copy, one
              adn_stream_pool_push_rate per 64 streams), step() with one adn_stream_pool_emit_rate per 64 rows that ran
    composed  what the pool's docstring recommended before: a StreamResampler(n_streams=1) on each side of every stream around
              pool.push / pool.step of a pool at the working rate

for 64 and 256 streams, all at 48 kHz and a 48 / 44.1 / 16 / 8 kHz mix, at the defaults (n_fft 512, hop 128, window 192, block 16: a
step per 0.256 s of audio, so about one round in 26 has steps to run; rounds with and without are reported apart).  Blocks arrive
as numpy arrays and results leave as numpy arrays in both forms.  Per round: device time (events around the round), host time
(the round's calls until they return; the device is synchronised after the clock is read) and the library calls that resample or
write a ring (adn_resample_stream, adn_stream_pool_write, adn_stream_pool_push_rate, adn_stream_pool_emit_rate), each a kernel
launch or up to two device copies.  Medians over the measured rounds.  One JSON line per record:

    python tools/bench_stream_pool_rate.py [--rounds 80] [--write profiles] [--commit ID]

Synthetic weights (seed 1234): times do not depend on the weights' values.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIX = (48000, 44100, 16000, 8000)
COUNTED = ("adn_resample_stream", "adn_stream_pool_write", "adn_stream_pool_push_rate", "adn_stream_pool_emit_rate")


class Counter:
    """Counts the calls of some entry points of the loaded library (the ctypes functions are wrapped in place)."""

    def __init__(self, lib, names):
        self.n = 0
        for name in names:
            fn = getattr(lib, name)
            setattr(lib, name, self._wrap(fn))

    def _wrap(self, fn):
        def call(*a):
            self.n += 1
            return fn(*a)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="64,256")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--warmup", type=int, default=30, help="rounds before the measured ones (at least one with steps)")
    ap.add_argument("--rounds", type=int, default=80)
    ap.add_argument("--write", default=None, help="directory for bench_stream_pool_rate.jsonl")
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from audiodenoiser_amd import StreamPool, StreamResampler, _lib, build
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.weights import make_state_dict
    assert torch.cuda.is_available(), "bench_stream_pool_rate.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    net = UNet(1, 1)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(1234).items()}, strict=True)
    net = net.to(dev).eval().set_compute_dtype(args.dtype)
    counter = Counter(_lib.load(), COUNTED)
    records = []

    for n in (int(s) for s in args.streams.split(",")):
        for name, rates in (("48k", [48000] * n), ("mix", [MIX[i % 4] for i in range(n)])):
            rng = np.random.default_rng(n)
            total = args.warmup + args.rounds
            feed = [rng.uniform(-0.5, 0.5, (r // 100) * total).astype(np.float32) for r in rates]

            pool = StreamPool(net, max_streams=n, input_rates=MIX)
            sids = [pool.open(input_rate=r) for r in rates]

            def rate_round(k):
                pool.push_many({sid: feed[i][k * (rates[i] // 100):(k + 1) * (rates[i] // 100)] for i, sid in enumerate(sids)})
                return len(pool.step())

            plain = StreamPool(net, max_streams=n)
            psids = [plain.open() for _ in rates]
            rs_in = [StreamResampler(r, 8000, 1, dev) for r in rates]
            rs_out = [StreamResampler(8000, r, 1, dev) for r in rates]

            def composed_round(k):
                for i, sid in enumerate(psids):
                    x = torch.from_numpy(feed[i][k * (rates[i] // 100):(k + 1) * (rates[i] // 100)]).to(dev)
                    plain.push(sid, rs_in[i].push(x)[0])
                outs = [rs_out[sid].push(samples) for sid, samples, _ in plain.step()]
                if outs:
                    torch.cat([o[0] for o in outs]).cpu()
                return len(outs)

            rec = {"record": "round", "dtype": args.dtype, "n_streams": n, "rates": name, "push_ms": 10}
            for form, fn in (("rate", rate_round), ("composed", composed_round)):
                rows = {False: [], True: []}
                for k in range(total):
                    torch.cuda.synchronize(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    calls = counter.n
                    e0.record()
                    t0 = time.perf_counter()
                    ran = fn(k)
                    host = (time.perf_counter() - t0) * 1e3
                    e1.record()
                    torch.cuda.synchronize(dev)
                    if k >= args.warmup:
                        rows[ran > 0].append((e0.elapsed_time(e1), host, counter.n - calls))
                for ticked, key in ((False, "push_round"), (True, "tick_round")):
                    r = rows[ticked]
                    rec[f"{form}_{key}"] = ({"rounds": len(r), "device_ms": round(statistics.median(x[0] for x in r), 4),
                                             "host_ms": round(statistics.median(x[1] for x in r), 4),
                                             "resample_calls": int(statistics.median(x[2] for x in r))} if r else {"rounds": 0})
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del pool, plain, rs_in, rs_out
            net._workspace = None
            torch.cuda.empty_cache()
    if args.write:
        digest = build.code_digest_of_built_library()
        with open(os.path.join(args.write, "bench_stream_pool_rate.jsonl"), "w") as fh:
            for rec in records:
                fh.write(json.dumps(dict(rec, commit=args.commit, library_digest=digest[:16])) + "\n")


if __name__ == "__main__":
    main()
