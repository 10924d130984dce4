#!/usr/bin/env python3
"""Forward and backward time of the per-clip CombinedPerceptualLoss (adn_perceptual_loss / adn_perceptual_loss_backward, both
gradients) through the C ABI, buffers allocated once.  Device events around `--steps` calls after `--warmup`, median of
`--groups` groups.  Prints one JSON line per shape; `bwd_bytes` is the backward's algorithmic HBM traffic (pred and target read
twice -- series sums, then the broadcast -- and both gradients written once).

    python tools/bench_loss_grad.py [--shapes 64x513x256,2x24x65535]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def time_ms(fn, steps, warmup, groups):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(groups):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x513x256,2x24x65535")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=5)
    args = ap.parse_args()
    from audiodenoiser_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for spec in args.shapes.split(","):
        b, f, t = (int(v) for v in spec.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        pred = torch.rand((b, 1, f, t), generator=g, device=dev) * 3
        tgt = torch.rand((b, 1, f, t), generator=g, device=dev) * 3
        gout = torch.full((b, 4), 0.0, device=dev)
        gout[:, 0] = 1.0 / b
        out = torch.empty((b, 4), device=dev)
        gp, gq = torch.empty_like(pred), torch.empty_like(tgt)
        n1, n2 = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(L.adn_perceptual_loss_workspace_bytes(b, f, t, ctypes.byref(n1)), "workspace")
        _lib.check(L.adn_perceptual_loss_backward_workspace_bytes(b, f, t, ctypes.byref(n2)), "workspace")
        ws1 = torch.empty(n1.value, dtype=torch.uint8, device=dev)
        ws2 = torch.empty(n2.value, dtype=torch.uint8, device=dev)

        def fwd():
            _lib.check(L.adn_perceptual_loss(pred.data_ptr(), tgt.data_ptr(), b, f, t, ws1.data_ptr(), n1.value,
                                             out.data_ptr(), st), "adn_perceptual_loss")

        def bwd():
            _lib.check(L.adn_perceptual_loss_backward(pred.data_ptr(), tgt.data_ptr(), b, f, t, gout.data_ptr(),
                                                      ws2.data_ptr(), n2.value, gp.data_ptr(), gq.data_ptr(), st),
                       "adn_perceptual_loss_backward")
        ms_f = time_ms(fwd, args.steps, args.warmup, args.groups)
        ms_b = time_ms(bwd, args.steps, args.warmup, args.groups)
        nbytes = b * f * t * 4
        print(json.dumps({"shape": [b, 1, f, t], "fwd_ms": round(ms_f, 4), "bwd_ms": round(ms_b, 4),
                          "bwd_over_fwd": round(ms_b / ms_f, 3), "bwd_bytes": 6 * nbytes,
                          "bwd_algorithmic_GBps": round(6 * nbytes / (ms_b * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
