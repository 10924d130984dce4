"""The case table of the perceptual-loss tests (tests/test_loss_cases_host.py, tests/test_gpu_loss_cases.py): inputs chosen so that
every mel-filterbank row, every STFT bin, every frame at a block join and every launch regime of csrc/loss_kernels.hip moves an
asserted number, and so that no |Xp| ~ |Xq| tie leaves the float32 and float64 gradients on different sides of a sign.

Construction.  Every input is ``series[t] + eps * noise[f, t]`` with noise that has zero mean over the F rows, so the frequency-mean
series is the chosen one.  With a gradient check the target is ``alpha * series + eps * noise'``, alpha alternating between 0.5 and
2 from clip to clip: |Xq| = alpha |Xp| up to rounding, so every |Xp| - |Xq| is half or all of |Xp| and no sign hangs on rounding
(checked entry by entry in test_loss_cases_host.py, factor 16).  Series take both signs.

The upstream gradient of every gradient case is ``weights(B)``: a fixed (B, 4) matrix of distinct entries with both signs and a
few zeros, backpropagated as sum(per_clip * W), so each clip and each of the four columns has its own weight.

``expected_tb(B, T)`` restates the block-width rule of launch_perceptual_loss_backward (csrc/loss_kernels.hip, the two lines
``int tb = LG_TB; while (tb > 64 && (long)n_clips * ((T + tb - 1) / tb) < 512) tb /= 2;``).  The rule cannot be observed from
Python: whoever changes it in C++ must mirror the change here, or the series-block cases no longer reach the regimes they name.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass, field

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as R  # noqa: E402

EPS = 0.02
LDS_T = 6784                               # ADN_LOSS_LDS_T: longer clips walk the mel frames in blocks of MEL_FB
MEL_FB = 256                               # LOSS_MEL_FB
BURST_W = 8
REACH = 62                                 # n_fft - 1: a frame that holds a burst sample reaches this far


def expected_tb(B: int, T: int) -> int:
    tb = 256
    while tb > 64 and B * ((T + tb - 1) // tb) < 512:
        tb //= 2
    return tb


def weights(B: int) -> torch.Tensor:
    """(B, 4) float32: a golden-ratio sequence on [-2, 2) (distinct entries, both signs) with three entries set to 0."""
    v = (np.arange(1, 4 * B + 1, dtype=np.float64) * 0.6180339887498949) % 1.0 * 4.0 - 2.0
    w = v.reshape(B, 4)
    w[0, 1] = 0.0
    w[B - 1, 3] = 0.0
    w[B // 2, 0] = 0.0
    return torch.from_numpy(w).float()


@dataclass
class Case:
    name: str
    pred: torch.Tensor                     # (B, 1, F, T) float32
    target: torch.Tensor
    grad: bool = True
    bursts: list | None = None             # per clip: centre of its burst (everything else is exactly zero)
    identical: tuple = ()                  # clips with pred == target
    info: dict = field(default_factory=dict)

    @property
    def shape(self):
        return tuple(self.pred.shape)

    @property
    def W(self):
        return weights(self.pred.shape[0])


def _noise(g, B, F, T):
    n = torch.randn(B, 1, F, T, generator=g, dtype=torch.float64)
    return n - n.mean(dim=2, keepdim=True)


def _alpha(B):
    return torch.tensor([0.5 if b % 2 == 0 else 2.0 for b in range(B)], dtype=torch.float64).reshape(B, 1, 1, 1)


def _pair(series: torch.Tensor, F: int, g, mask: torch.Tensor | None = None):
    """series (B, T) float64 -> pred, target (B,1,F,T) float32; mask (B, T) confines the noise (burst cases)."""
    B, T = series.shape
    s = series.reshape(B, 1, 1, T)
    n1, n2 = _noise(g, B, F, T), _noise(g, B, F, T)
    if mask is not None:
        m = mask.reshape(B, 1, 1, T).double()
        n1, n2 = n1 * m, n2 * m
    return (s + EPS * n1).float().contiguous(), (_alpha(B) * s + EPS * n2).float().contiguous()


def _broadband(name, B, F, T, seed, **info):
    g = torch.Generator().manual_seed(seed)
    series = torch.randn(B, T, generator=g, dtype=torch.float64)
    return Case(name, *_pair(series, F, g), info=info)


def burst_span(c: int, T: int) -> tuple[int, int]:
    return max(0, c - BURST_W // 2), min(T, c + BURST_W // 2)


def _bursts(name, T, centres, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(centres)
    series = torch.zeros(B, T, dtype=torch.float64)
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b, c in enumerate(centres):
        lo, hi = burst_span(c, T)
        v = torch.randn(hi - lo, generator=g, dtype=torch.float64)
        series[b, lo:hi] = v + 0.5 * torch.sign(v)         # both signs, nothing near zero
        mask[b, lo:hi] = True
    return Case(name, *_pair(series, 4, g, mask), bursts=list(centres))


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    kind, _, arg = name.partition(":")
    if kind == "bins":                                       # clip k: a tone at k / 63 cycles per sample + 0.3 white noise
        g = torch.Generator().manual_seed(101)
        t = torch.arange(96, dtype=torch.float64)
        k = torch.arange(32, dtype=torch.float64).reshape(32, 1)
        series = torch.cos(2 * np.pi * k * t / 63.0 + 0.7 * k) + 0.3 * torch.randn(32, 96, generator=g, dtype=torch.float64)
        return Case(name, *_pair(series, 24, g))
    if kind == "short":
        return _broadband(name, 4, 33, int(arg), 200 + int(arg))
    if kind == "rows":
        return _broadband(name, 2, int(arg), 40, 300 + int(arg) % 97)
    if kind == "bursts":
        T = int(arg)
        if T == LDS_T:
            centres = [0, 1, 31, 32, T // 2, T - 33, T - 32, T - 2, T - 1]
        else:
            centres = [16 * 255, 16 * 256, 16 * 256 - 31, 16 * 256 + 31]
            if T > 16 * 512:
                centres += [16 * 511, 16 * 512, T - 2, T - 1]
        return _bursts(name, T, centres, 400 + T % 89)
    if kind == "tb":
        B, T = (int(v) for v in arg.split("x"))
        return _broadband(name, B, 4, T, 500 + B, tb=expected_tb(B, T))
    if kind == "clips":                                      # 65537 distinct clips: 0.6 + 0.9 (-1)^t + 0.2 white noise, so the
        B, T = 65537, 32                                     # real-valued DC and Nyquist bins of every frame are far from 0
        g = torch.Generator().manual_seed(601)
        t = torch.arange(T, dtype=torch.float64)
        series = 0.6 + 0.9 * (1 - 2 * (t % 2)) + 0.2 * torch.randn(B, T, generator=g, dtype=torch.float64)
        return Case(name, *_pair(series, 1, g))
    if kind == "align":
        return _broadband(name, 3, 8, int(arg), 700 + int(arg))
    if kind == "exact":                                      # clip 1: pred == target
        c = _broadband(name, 3, 8, 48, 801)
        target = c.target.clone()
        target[1] = c.pred[1]
        return Case(name, c.pred, target, identical=(1,))
    raise KeyError(name)


SHORT = [f"short:{t}" for t in (32, 33, 47, 63, 64)]
ROWS = [f"rows:{f}" for f in (1, 31, 32, 33, 8225)]
BURSTS = [f"bursts:{t}" for t in (LDS_T, 6785, 8209)]
TB = ["tb:2x200", "tb:8x8200", "tb:16x8200", "tb:512x40"]
ALIGN = ["align:64", "align:63"]
GRAD_CASES = ["bins"] + SHORT + ROWS + BURSTS + TB + ["clips"] + ALIGN + ["exact"]

L1_ELEMS = (1, 255, 257, 2 ** 22 + 3)


@functools.lru_cache(maxsize=None)
def l1_inputs(elems: int):
    g = torch.Generator().manual_seed(900 + elems % 1000)
    return torch.randn(3, elems, generator=g), torch.randn(3, elems, generator=g)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(out, grad_pred, grad_target) of the float64 restatement for the case, computed once and shared; do not modify."""
    c = case(name)
    return R.run(R.per_clip, c.pred, c.target, c.W if c.grad else None, torch.float64)


@functools.lru_cache(maxsize=None)
def floors(name: str):
    c = case(name)
    # 65537 clips: the kernel-order loops over every 16th clip (4097 of them) keep the case at a few seconds
    return R.floors(c.pred, c.target, c.W if c.grad else None, reference(name), kernel_every=16 if name == "clips" else 1)


def bounds(name: str) -> dict[str, float]:
    """statistic -> MARGIN x floor: the bound of the device tests and the yardstick of the host sensitivity test."""
    return {k: R.MARGIN * v for k, v in floors(name)["floor"].items()}


def far_field(c: Case) -> torch.Tensor:
    """(B, T) bool: series positions farther than REACH from the clip's burst and from its reflections about 0 and T - 1."""
    B, T = c.pred.shape[0], c.pred.shape[3]
    t = np.arange(T)
    far = np.ones((B, T), dtype=bool)
    for b, centre in enumerate(c.bursts):
        lo, hi = burst_span(centre, T)
        for a, z in ((lo, hi - 1), (-(hi - 1), -lo), (2 * (T - 1) - (hi - 1), 2 * (T - 1) - lo)):
            far[b] &= (t < a - REACH) | (t > z + REACH)
    return torch.from_numpy(far)


if __name__ == "__main__":                                   # python tests/loss_cases.py: the floors of every case
    for nm in GRAD_CASES:
        fl = floors(nm)
        print(nm, case(nm).shape)
        for key in ("library", "kernel"):
            print("   ", key, " ".join(f"{k} {v:.2e}" for k, v in fl[key].items()))
