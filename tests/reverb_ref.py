"""The reverb of include/adn.h ("add_noise for reverb") restated as a plain per-sample loop, written from the definition and
not from the kernel: no chunks, no scan, one sample after the other.

``dtype`` is the working precision of everything after the scalars (``numpy.float64`` for the parity reference,
``numpy.float32`` for the rounding floor of the sequential form).  The scalars themselves are fp32 by definition, in the
header's order, whatever the working precision.
"""
from __future__ import annotations

import numpy as np

COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_TUNING = (556, 441, 341, 225)
DEFAULTS = dict(room_size=0.9, damping=0.9, wet_level=0.33, dry_level=0.4, width=1.0)


def delay_lengths(sample_rate: int):
    """(comb delays, all-pass delays) in samples: ``(sample_rate * tuning) // 44100``."""
    sr = int(sample_rate)
    return [sr * t // 44100 for t in COMB_TUNING], [sr * t // 44100 for t in ALLPASS_TUNING]


def scalars(room_size, damping, wet_level, dry_level, width):
    """feedback, damp, gain, wet1, dry: every operation rounded to fp32."""
    f = np.float32
    room_size, damping, wet_level, dry_level, width = f(room_size), f(damping), f(wet_level), f(dry_level), f(width)
    feedback = f(f(room_size * f(0.28)) + f(0.7))
    damp = f(damping * f(0.4))
    gain = f(0.015)
    wet1 = f(f(f(0.5) * f(wet_level * f(3.0))) * f(f(1.0) + width))
    dry = f(dry_level * f(2.0))
    return feedback, damp, gain, wet1, dry


def reverb_ref(x, sample_rate, room_size=0.9, damping=0.9, wet_level=0.33, dry_level=0.4, width=1.0, clip=True,
               dtype=np.float64):
    """``x`` (L,) or (B, L) -> the same shape in ``dtype``; every clip starts from zero state."""
    x = np.asarray(x)
    if x.ndim == 2:
        return np.stack([reverb_ref(row, sample_rate, room_size, damping, wet_level, dry_level, width, clip, dtype) for row in x])
    t = np.dtype(dtype).type
    feedback, damp, gain, wet1, dry = (t(v) for v in scalars(room_size, damping, wet_level, dry_level, width))
    one_minus_damp = t(1.0) - damp
    half = t(0.5)
    comb_d, ap_d = delay_lengths(sample_rate)
    comb = [[t(0.0)] * d for d in comb_d]
    last = [t(0.0)] * len(comb_d)
    ap = [[t(0.0)] * d for d in ap_d]
    xs = [t(v) for v in x.astype(dtype)]
    y = np.empty(len(xs), dtype=dtype)
    for n, xn in enumerate(xs):
        inp = xn * gain
        acc = t(0.0)
        for j, d in enumerate(comb_d):
            buf = comb[j]
            pos = n % d
            o = buf[pos]
            last[j] = o * one_minus_damp + last[j] * damp
            buf[pos] = inp + last[j] * feedback
            acc = acc + o
        for j, d in enumerate(ap_d):
            buf = ap[j]
            pos = n % d
            b = buf[pos]
            buf[pos] = acc + b * half
            acc = b - acc
        y[n] = acc * wet1 + xn * dry
    if clip:
        y = np.clip(y, t(-1.0), t(1.0))
    return y
