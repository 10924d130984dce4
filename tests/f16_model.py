"""A model of what the fp16 U-Net path computes, one block at a time -- TEST INFRASTRUCTURE (plain torch on the CPU).

The fp16 path (csrc/unet.hip, conv16_kernels.hip, convt16_kernels.hip, conv_dma<_Float16>) stores every activation as fp16, holds
its 3x3 and transposed-convolution weights as fp16 and accumulates in fp32.  This file restates that arithmetic with float64
accumulation, so that what is left between a kernel and the model is the order of the kernel's fp32 sums and the occasional
rounding tie that order flips -- one or two fp16 ulps per element -- instead of nine blocks of accumulated storage rounding.

What is restated (pack_weights / bn_fold in csrc/unet.hip):
  * BatchNorm fold in fp32: scale = gamma / sqrt(var + eps), bias = (b - mean) * scale + beta.
  * 3x3 weights fp16(w * scale[co]) (product in fp32), folded fp32 bias; ReLU, then rounding to fp16, after each of the two convs.
  * down1's first conv: fp32 weights w * scale on the fp32 network input (conv_first_kernel<_Float16>), or, where the layer is
    computed inside conv16_f16 (FIRST, one input plane, default switches), on the fp16 matrix cores: weights fp16(w * scale),
    the input as hi + lo = fp16(x) + fp16(x - fp16(x)), the bias as fp16(b) + fp16(b - fp16(b)) (`fused_first`).
  * transposed convolution: weights fp16(w), raw fp32 bias, output rounded to fp16 (no ReLU).
  * asymmetric pad + cat([skip, up]) and MaxPool2d(2) as oracle/unet_torch.py.
  * 1x1 output convolution: fp32 weights and bias, on the fp16 up4 tensor (conv_out_kernel; conv_dma's fused tail reads its staged
    fp16 values too) or, in conv16_f16's fused tail, on the UNROUNDED ReLU(accumulator) values.

Teacher forcing: ``run(x, mode, taps=device_taps)`` feeds every block the device's own block outputs (exact fp16 values), so a
block's error is its own.  ``taps=None`` runs the chain freely.

Modes: "f64" accumulates in float64 (the reference); "f32" accumulates in fp32 with the input channels permuted (the floor: a
stand-in for any legitimate fp32 summation order).  Every block returns ``(out, z)``: the fp16-rounded output and the value before
that rounding (after ReLU), both as float64 tensors.

Error unit of a block: u = ulp16(max(|z|, rms(z))), E = max over ALL elements of |tap - z| / u.  Outputs y: 2^-11 * max(|y|, rms(y)).
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from audiodenoiser_amd.weights import BN_EPS

DOWN = ("down1", "down2", "down3", "down4")
UP = ("up1", "up2", "up3", "up4")
BLOCKS = DOWN + ("bottleneck",) + UP
PREFIX = {"down1": "downconv1.conv", "down2": "downconv2.conv", "down3": "downconv3.conv", "down4": "downconv4.conv",
          "bottleneck": "bottleneck", "up1": "upconv1.conv", "up2": "upconv2.conv", "up3": "upconv3.conv", "up4": "upconv4.conv"}


def r16(t):
    """Round to fp16 (through fp32, as the device's accumulators are) and return in t's dtype."""
    return t.to(torch.float32).to(torch.float16).to(t.dtype)


def ulp16(v):
    """Spacing of fp16 at magnitude v (float64 tensor, v >= 0); below the smallest normal the subnormal spacing 2^-24."""
    _, e = torch.frexp(v)                                      # v = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e.clamp_min(-13) - 11)


def block_error(tap, z):
    """E of a block: max |tap - z| / ulp16(max(|z|, rms(z))) over every element."""
    tap, z = tap.double(), z.double()
    rms = z.pow(2).mean().sqrt()
    u = ulp16(torch.maximum(z.abs(), rms))
    return float(((tap - z).abs() / u).max())


def y_error(y, ref):
    y, ref = y.double(), ref.double()
    rms = ref.pow(2).mean().sqrt()
    u = torch.maximum(ref.abs(), rms) * 2.0 ** -11
    return float(((y - ref).abs() / u).max())


def pool_max(t):
    return F.max_pool2d(t, 2)


def pool_first_of_pair(t):
    """MUTATION: the maximum over the two rows, but the first column of the pair instead of the larger one."""
    h, w = t.shape[2] // 2 * 2, t.shape[3] // 2 * 2
    return torch.maximum(t[:, :, 0:h:2, 0:w:2], t[:, :, 1:h:2, 0:w:2])


class F16Model:
    def __init__(self, sd, fused_first=False, rounding=True, perm_seed=5):
        self.rounding = rounding
        self.fused_first = fused_first and rounding
        self.pad_shift = {}                                    # MUTATION: block -> extra left pad of the up tensor (right pad less)
        self.pool = pool_max
        self.perm_seed = perm_seed
        self.w, self.b = {}, {}
        q = (lambda a: a.astype(np.float16)) if rounding else (lambda a: a)
        for block, prefix in PREFIX.items():
            for idx in (0, 3):
                p = f"{prefix}.double_conv."
                w = np.asarray(sd[f"{p}{idx}.weight"], dtype=np.float32)
                gamma, beta = (np.asarray(sd[f"{p}{idx + 1}.{k}"], dtype=np.float32) for k in ("weight", "bias"))
                mean, var = (np.asarray(sd[f"{p}{idx + 1}.{k}"], dtype=np.float32) for k in ("running_mean", "running_var"))
                scale = gamma / np.sqrt(var + np.float32(BN_EPS))
                bias = (np.asarray(sd[f"{p}{idx}.bias"], dtype=np.float32) - mean) * scale + beta
                assert scale.dtype == np.float32 and bias.dtype == np.float32
                wf = w * scale[:, None, None, None]
                first = block == "down1" and idx == 0
                self.w[block, idx] = torch.from_numpy((wf if first and not self.fused_first else q(wf)).astype(np.float64))
                self.b[block, idx] = torch.from_numpy(bias.astype(np.float64))
        for block in UP:
            top = PREFIX[block].split(".")[0]
            self.w[block, "up"] = torch.from_numpy(q(np.asarray(sd[f"{top}.up.weight"], dtype=np.float32)).astype(np.float64))
            self.b[block, "up"] = torch.from_numpy(np.asarray(sd[f"{top}.up.bias"], dtype=np.float64))
        self.w["out"] = torch.from_numpy(np.asarray(sd["out.weight"], dtype=np.float64))
        self.b["out"] = torch.from_numpy(np.asarray(sd["out.bias"], dtype=np.float64))

    def mutated(self):
        """A copy whose weights, pad shifts and pooling may be changed without touching this model."""
        m = copy.copy(self)
        m.w = {k: v.clone() for k, v in self.w.items()}
        m.pad_shift = dict(self.pad_shift)
        return m

    # ---- one layer: float64 in, float64 out (the values an fp32 accumulation gives in mode "f32") -----------------------------
    def _perm(self, c):
        return torch.from_numpy(np.random.default_rng(self.perm_seed + c).permutation(c))

    def _apply(self, fn, x, w, b, mode, cin_dim, **kw):
        if mode == "f64":
            return fn(x.double(), w, b, **kw)
        assert mode == "f32", mode
        perm = self._perm(x.shape[1])
        return fn(x[:, perm].float().contiguous(), w.index_select(cin_dim, perm).float().contiguous(), b.float(), **kw).double()

    def _rnd(self, t):
        return r16(t) if self.rounding else t

    def _first_fused(self, x, mode):
        """Conv2d(1 -> 64) inside conv16_f16 (FIRST): K = 9 taps of fp16(x) + 9 taps of the fp16 remainder, bias as two fp16 terms."""
        hi = r16(x.double())
        lo = r16(x.double() - hi)
        w, b = self.w["down1", 0], self.b["down1", 0]
        bh = r16(b)
        b2 = bh + r16(b - bh)
        return self._apply(F.conv2d, torch.cat([hi, lo], 1), torch.cat([w, w], 1), b2, mode, 1, padding=1)

    def double_conv(self, block, x, mode):
        if block == "down1" and self.fused_first:
            assert x.shape[1] == 1
            a = self._first_fused(x, mode)
        else:
            a = self._apply(F.conv2d, x, self.w[block, 0], self.b[block, 0], mode, 1, padding=1)
        a = self._rnd(F.relu(a))
        z = F.relu(self._apply(F.conv2d, a, self.w[block, 3], self.b[block, 3], mode, 1, padding=1))
        return self._rnd(z), z

    def up(self, block, prev, skip, mode):
        x1 = self._rnd(self._apply(F.conv_transpose2d, prev, self.w[block, "up"], self.b[block, "up"], mode, 0, stride=2))
        dy, dx = skip.shape[2] - x1.shape[2], skip.shape[3] - x1.shape[3]
        s = self.pad_shift.get(block, 0)
        x1 = F.pad(x1, [dx // 2 + s, dx - dx // 2 - s, dy // 2, dy - dy // 2])           # (a negative pad crops)
        return self.double_conv(block, torch.cat([skip.double(), x1], 1), mode)

    def out(self, t, mode):
        """The 1x1 output convolution on `t`: the fp16 up4 tap, or the unrounded z of up4 (conv16_f16's fused tail)."""
        return self._apply(F.conv2d, t, self.w["out"], self.b["out"], mode, 1)

    # ---- the nine blocks ------------------------------------------------------------------------------------------------------
    def run(self, x, mode, taps=None):
        """block -> (out, z).  taps: the block outputs every block's input is taken from (teacher forcing); None: its own chain."""
        res = {}
        src = (lambda name: taps[name].double()) if taps is not None else (lambda name: res[name][0])
        cur = x.double()
        for name in DOWN:
            res[name] = self.double_conv(name, cur, mode)
            cur = self.pool(src(name))
        res["bottleneck"] = self.double_conv("bottleneck", cur, mode)
        prev = "bottleneck"
        for i, name in enumerate(UP):
            res[name] = self.up(name, src(prev), src(DOWN[3 - i]), mode)
            prev = name
        return res

    def one(self, block, x, mode, taps):
        """Block `block` alone from the teacher inputs in `taps` (x for down1)."""
        if block in DOWN or block == "bottleneck":
            i = BLOCKS.index(block)
            cur = x.double() if i == 0 else self.pool(taps[BLOCKS[i - 1]].double())
            return self.double_conv(block, cur, mode)
        i = UP.index(block)
        return self.up(block, taps[BLOCKS[4 + i]].double(), taps[DOWN[3 - i]].double(), mode)


# ---- the cases of tests/test_gpu_f16_blocks.py (tests/test_f16_model_host.py checks that they are benign) -----------------------
# Tiles: conv16_f16 and conv_dma<_Float16> 32 rows x 16 columns of output pixels (C16_TH x C16_TW, conv_geom), convt16_f16 16 x 16
# INPUT pixels (T16_ROWS x T16_PX), conv_dma's transposed convolution 8 x 16; conv16_ksplit cuts a layer of at most 64 workgroups.
SHAPES = (
    (1, 16, 16),     # one pixel at the bottom; every layer a single partial tile
    (2, 33, 47),     # odd at every level: every transposed convolution's output is smaller than its skip in both directions
    (3, 40, 33),     # 2 x 3 tiles at full resolution, one column / eight rows in the last ones; three clips
    (2, 31, 16),     # height-only pad at the top level (31 -> 15 -> 30), width exact
    (1, 16, 130),    # width-only pads (130 -> 65 -> 32 -> 16 -> 8); nine column tiles, the last of two columns
    (1, 64, 80),     # whole tiles in both directions at full resolution, 32 x 40 / 16 x 20 below
    (17, 33, 47),    # every 3x3 layer above 64 workgroups: conv16_ksplit returns 1 on the default handle (no K-split slices)
    (1, 72, 32),     # rows only: conv16_f16 tiles of 32 + 32 + 8 rows at full and 32 + 4 at half resolution, columns exact (2 / 1
                     # tiles); convt16_f16 reads 36 x 16 (16 + 16 + 4 rows, up4) and 18 x 8 (16 + 2 rows, up3)
    (1, 64, 40),     # columns only: conv16_f16 tiles of 16 + 16 + 8 columns at full and 16 + 4 at half resolution, rows exact (2 / 1
                     # tiles); convt16_f16 reads 32 x 20 (16 + 4 columns, rows exact, up4) and 16 x 10 (up3)
)
WEIGHT_SETS = ("benign", "heavy")                  # ("trained" overflows fp16 at down4 with make_input's scale 3)
HEAVY_SHAPES = ((2, 33, 47), (1, 64, 80))          # the shapes the "heavy" set runs at
INPUT_SEED = 7
# (in_channels, num_classes, shape): the first layer on its own launch with several planes, the output convolution class by class;
# 33 and 64 planes at T = 200: conv_first_kernel's window rows hold 4096 / Cin - 2 = 122 / 62 columns, so the rows are cut into
# column tiles (100 and 50 columns wide); at T = 248 the tiles of 64 planes are 62 columns wide, the widest, and the launch asks for
# exactly 160 KiB of LDS (64 planes x 10 rows x 64 columns x 4 bytes)
PLANES = ((2, 3, (2, 33, 47)), (20, 2, (1, 40, 56)), (33, 1, (1, 24, 200)), (64, 2, (1, 24, 200)), (64, 2, (1, 24, 248)))


def weight_set(kind, in_channels=1, num_classes=1):
    from audiodenoiser_amd.weights import make_state_dict_variant
    return make_state_dict_variant(kind, 1234, in_channels, num_classes)


def case_input(n, f, t, in_channels=1):
    from audiodenoiser_amd.weights import make_input
    return make_input(INPUT_SEED, n * in_channels, f, t).reshape(n, in_channels, f, t)


def floor_and_reference(model, x, taps, blocks=BLOCKS):
    """block -> (z of the float64 model, E_ref = error of the fp32-permuted model's rounded output against it), same teacher inputs."""
    out = {}
    for name in blocks:
        z = model.one(name, x, "f64", taps)[1]
        out[name] = (z, block_error(model.one(name, x, "f32", taps)[0], z))
    return out


def bound(e_ref):
    """The device's bound from the floor of the same block: twice the floor, which is at least one unit."""
    return 2.0 * max(e_ref, 1.0)
