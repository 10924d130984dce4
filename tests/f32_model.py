"""A float64 model of the fp32 U-Net path, one block at a time, and fp32 restatements of every arithmetic the device may run for a
block -- TEST INFRASTRUCTURE (plain torch on the CPU).  The fp32 counterpart of tests/f16_model.py, whose plumbing it shares.

Reference (`form` "f64"): BatchNorm folded in fp32 exactly as pack_weights / bn_fold do (scale = gamma / sqrt(var + eps), w * scale,
(b - mean) * scale + beta), everything after that in float64, no storage rounding anywhere.  ``one(block, x, taps)`` teacher-forces a
block on the device's own fp32 block outputs, so a block's error is its own; the pool of a down block is checked through the next
block, whose input is the pool of the exported skip.

Floors: the arithmetic of every kernel form restated in float32, in another summation order: the input channels permuted, and every
contraction as the kernels' matrix-core K loops form it -- ONE fp32 accumulator per output walked along K (`chain_matmul`; six
roundings per 16-channel chunk in the split form, `split_matmul`).  That chain is a property of every form, not a defect: its rounding
error grows as sqrt(K / 24) ulps (6 - 16 ulps rms at K = 2304 - 9216), where a CPU GEMM's blocked sums stay at 2 - 3; a floor taken
from the latter calls every kernel wrong by 3 - 6 x (measured on the direct fp32 kernel, which has nothing else in it).
  direct   fp32 products and sums (conv_mfma<float>; conv_first_kernel; the exact-fp32 transposed convolution, ADN_CONVT_SPLIT=0)
  f2, f4   Winograd F(2x2,3x3) / F(4x4,3x3) (wino_kernels.hip, wino4_kernels.hip): U = G g G^T * scale in double rounded once to
           fp32 (pack_wino3x3 / wino4_u), V = B^T d B and A^T M A in fp32 in two passes, the products summed in fp32; points
           0, +-1, inf and 0, +-1, +-2, inf (bt6 / at6 in csrc/adn_internal.h)
  split    both operands as hi + mid + lo, round-to-nearest bf16 terms with hi clamped to the largest finite bf16 (split3_bf16 /
           split3_host), the six products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi with fp32 sums (conv_dma<..., SPLIT>): the
           transposed convolutions directly, and "f4s" = the three-stage form (wino3s_kernels.hip), f4's transforms around a split GEMM
The fused tail (CONV3X3_RELU_DOT + finish) contracts the unrounded fp32 values the taps run stores: the same arithmetic in another
order, so its floor is the 1x1 convolution in fp32 on the restated up4 values.

A block's form is a tuple (transposed convolution, first 3x3, second 3x3); `form_set` restates choose_conv3 / choose_convt: the forms
a handle created under a configuration may run for a block at a shape (the table is in its docstring and in profiles/f32_blocks.md).

Error of a block, in fp32 ulps: e = |tap - z| / ulp32(max(|z|, rms z)) per element; E = (max e, rms e).  Outputs y: the same with
2^-24 * max(|y|, rms y).  Bound, per statistic: 2 * max(floor, 1), floor = the largest value of that statistic over the form set and
over the channel orders ORDERS (the factor 2 is f16_model.bound's margin over the stand-in's order).

The `dev` arguments put exactly one thing wrong into the split restatement: tests/test_f32_model_host.py holds the bound to
noticing each.
"""
import numpy as np
import torch
import torch.nn.functional as F

from audiodenoiser_amd.weights import BN_EPS
from f16_model import BLOCKS, DOWN, PLANES, PREFIX, SHAPES, UP, case_input, pool_max, weight_set  # noqa: F401  (shared with the tests)

LEVEL = {"down1": 0, "down2": 1, "down3": 2, "down4": 3, "bottleneck": 4, "up1": 3, "up2": 2, "up3": 1, "up4": 0}
BF16_MAX = float.fromhex("0x1.fep127")

# Winograd matrices: F(2x2,3x3) on the points 0, 1, -1, inf; F(4x4,3x3) on 0, 1, -1, 2, -2, inf (csrc/adn_internal.h, csrc/unet.hip)
WINO = {
    2: dict(BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
            G=[[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]],
            AT=[[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: dict(BT=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]],
            G=[[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
            AT=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
}


def ulp32(v):
    """Spacing of fp32 at magnitude v (float64 tensor, v >= 0); below the smallest normal the subnormal spacing 2^-149."""
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e.clamp_min(-125) - 24)


def _stats(r):
    return float(r.max()), float(r.pow(2).mean().sqrt())


def block_error(tap, z):
    """(E_max, E_rms) of a block: |tap - z| / ulp32(max(|z|, rms z)) over every element."""
    tap, z = tap.double(), z.double()
    return _stats((tap - z).abs() / ulp32(torch.maximum(z.abs(), z.pow(2).mean().sqrt())))


def y_error(y, ref):
    y, ref = y.double(), ref.double()
    return _stats((y - ref).abs() / (torch.maximum(ref.abs(), ref.pow(2).mean().sqrt()) * 2.0 ** -24))


def bound(floor):
    """Per statistic: twice the floor, which is at least one unit."""
    return tuple(2.0 * max(f, 1.0) for f in floor)


def within(e, b):
    return e[0] <= b[0] and e[1] <= b[1]


def floor_of(floors):
    """The floor of a form set: per statistic the largest value over its forms."""
    return tuple(max(f[i] for f in floors) for i in (0, 1))


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def split3(t):
    """split3_bf16 / split3_host on an fp32 tensor: (hi, mid, lo) as fp32 tensors holding bf16 values."""
    hi = bf16(t).clamp(-BF16_MAX, BF16_MAX)
    r1 = t - hi
    mid = bf16(r1)
    return hi, mid, bf16(r1 - mid)


def chain_matmul(a, b):
    """a @ b (fp32, batched) the way a matrix-core K loop sums it: ONE fp32 accumulator per output, walked along K a term at a time,
    acc = fl(acc + fl(a_k b_k)).  (A CPU GEMM sums in blocks, pairwise: 3 - 6 x less rounding error at K = 10^3 - 10^4 than any
    kernel that keeps one accumulator; rounding the product too, where the device fuses it, adds 0.3 ulp rms of the sum.)"""
    at = a.transpose(-1, -2).contiguous()
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
    for k in range(a.shape[-1]):
        acc.addcmul_(at[..., k, :, None], b[..., k, None, :])
    return acc


def split_matmul(a, b, dev=None, mask16=None):
    """a @ b (fp32, batched) as conv_dma<..., SPLIT> sums it: both operands in the three-term bf16 split, K in chunks of 16, six
    matrix-core products a chunk -- lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (activation . weight), small terms first.  One
    v_mfma_f32_32x32x16_bf16 adds its 16 products to the fp32 accumulator in two steps of 8 (k 0..7, then k 8..15), each step the sum
    of its products rounded once into the accumulator (tools/ubench/mfma_bf16_rounding.hip, profiles/f32_blocks.md): twelve roundings
    per 16 channels.
    mask16: the rows of b (input channels) of the last 16-channel chunk, for the deviation that zeroes their lo plane."""
    dev = dev or {}
    ah, am, al = split3(a)
    bh, bm, bl = split3(b)
    if dev.get("wlo16"):
        bl = bl.clone()
        bl[..., mask16, :] = 0.0
    pairs = [(p, q) for name, p, q in (("lo.hi", al, bh), ("hi.lo", ah, bl), ("mid.mid", am, bm), (None, am, bh), (None, ah, bm),
                                       (None, ah, bh)) if name is None or name != dev.get("drop")]
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
    for c in range(0, a.shape[-1], 16):
        for p, q in pairs:
            for h in (c, c + 8):
                acc = (acc.double() + torch.matmul(p[..., h:h + 8].double(), q[..., h:h + 8, :].double())).float()
    return acc


def _ksplit8(a, b, mm, dev):
    """a @ b over eight K slices whose copies are added in fp32 (the K-split reduce); `dev`: copy 5 rounded to bf16 first."""
    k = a.shape[-1] // 8
    out = None
    for s in range(8):
        t = mm(a[..., s * k:(s + 1) * k], b[..., s * k:(s + 1) * k, :], s)
        if dev.get("ksplit_bf16") and s == 5:
            t = bf16(t)
        out = t if out is None else out + t
    return out


class F32Model:
    def __init__(self, sd, perm_seed=5):
        self.perm_seed = perm_seed
        self.raw, self.scale, self.w, self.b32 = {}, {}, {}, {}
        for block, prefix in PREFIX.items():
            for idx in (0, 3):
                p = f"{prefix}.double_conv."
                w = np.asarray(sd[f"{p}{idx}.weight"], dtype=np.float32)
                gamma, beta = (np.asarray(sd[f"{p}{idx + 1}.{k}"], dtype=np.float32) for k in ("weight", "bias"))
                mean, var = (np.asarray(sd[f"{p}{idx + 1}.{k}"], dtype=np.float32) for k in ("running_mean", "running_var"))
                scale = gamma / np.sqrt(var + np.float32(BN_EPS))
                bias = (np.asarray(sd[f"{p}{idx}.bias"], dtype=np.float32) - mean) * scale + beta
                wf = w * scale[:, None, None, None]
                assert scale.dtype == np.float32 and bias.dtype == np.float32 and wf.dtype == np.float32
                self.raw[block, idx], self.scale[block, idx] = torch.from_numpy(w), torch.from_numpy(scale)
                self.w[block, idx] = torch.from_numpy(wf)                       # fp32 values; .double() where the reference reads them
                self.b32[block, idx] = torch.from_numpy(bias)
        for block in UP:
            top = PREFIX[block].split(".")[0]
            self.w[block, "up"] = torch.from_numpy(np.asarray(sd[f"{top}.up.weight"], dtype=np.float32))
            self.b32[block, "up"] = torch.from_numpy(np.asarray(sd[f"{top}.up.bias"], dtype=np.float32))
        self.w["out"] = torch.from_numpy(np.asarray(sd["out.weight"], dtype=np.float32))
        self.b32["out"] = torch.from_numpy(np.asarray(sd["out.bias"], dtype=np.float32))
        self._u = {}                                                            # (block, idx, m) -> U [pos][cin][cout], fp32

    def _perm(self, c):
        return torch.from_numpy(np.random.default_rng(self.perm_seed + c).permutation(c))

    # ---- one layer: fp32 values in (any dtype), float64 out, before the ReLU ----------------------------------------------------
    def _direct(self, x, w, b):
        """Conv2d (3x3 with padding 1, or 1x1) as one fp32 chain over the permuted channels, the taps of a channel in turn."""
        n, c, h, wd = x.shape
        perm = self._perm(c)
        ks = w.shape[2]
        a = F.unfold(x[:, perm].float(), ks, padding=ks // 2).permute(0, 2, 1).reshape(n * h * wd, c * ks * ks)
        y = chain_matmul(a, w[:, perm].reshape(w.shape[0], -1).T.contiguous()) + b
        return y.reshape(n, h, wd, -1).permute(0, 3, 1, 2).double()

    def _wino_u(self, key, m, dev):
        """U = G g G^T * scale in double, rounded once to fp32, as [pos][cin][cout]."""
        tap = dev.get("tap")
        if (key, m) in self._u and not tap:
            return self._u[key, m]
        g = self.raw[key].double()
        if tap:
            g = g.clone()
            g[:, :, 1, 2] *= 1.0 + 2.0 ** -12                   # the right neighbour: read wherever an image has two columns
        G = torch.tensor(WINO[m]["G"], dtype=torch.float64)
        u = (torch.matmul(torch.matmul(G, g), G.T) * self.scale[key].double()[:, None, None, None]).float()
        a = m + 2
        u = u.permute(2, 3, 1, 0).reshape(a * a, g.shape[1], g.shape[0]).contiguous()
        if not tap:
            self._u[key, m] = u
        return u

    def _wino(self, key, x, m, split=False, dev=None):
        dev = dev or {}
        n, c, h, w = x.shape
        a = m + 2
        ty, tx = -(-h // m), -(-w // m)
        bt = torch.tensor(WINO[m]["BT"], dtype=torch.float32)
        at = torch.tensor(WINO[m]["AT"], dtype=torch.float32)
        if dev.get("bt"):
            bt[0, 2] *= 1.0 + 2.0 ** -10
        if dev.get("at"):
            at[1, 3:5] *= 1.0 + 2.0 ** -10                        # at6's constant 2 (row 1 is used wherever an image has two rows)
        perm = self._perm(c)
        d = F.pad(x.float(), [1, tx * m - w + 1, 1, ty * m - h + 1]).unfold(2, a, m).unfold(3, a, m)        # n, c, ty, tx, a, a
        v = torch.matmul(torch.matmul(bt, d), bt.T)                                                         # two passes, fp32
        v = v.permute(4, 5, 0, 2, 3, 1).reshape(a * a, n * ty * tx, c)[:, :, perm].contiguous()
        u = self._wino_u(key, m, dev)[:, perm]
        if split:
            mm = split_matmul(v, u, dev, perm >= c - 16)
        else:
            mm = chain_matmul(v, u)
        cout = u.shape[2]
        mm = mm.reshape(a, a, n, ty, tx, cout).permute(2, 5, 3, 4, 0, 1)                                    # n, cout, ty, tx, a, a
        y = torch.matmul(torch.matmul(at, mm), at.T)                                                        # n, cout, ty, tx, m, m
        y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, cout, ty * m, tx * m)[:, :, :h, :w]
        b = self.b32[key]
        if dev.get("bias_bf16"):
            b = bf16(b)
        return (y + b[None, :, None, None]).double()

    def conv3(self, key, x, form, dev=None):
        if form == "f64":
            return F.conv2d(x.double(), self.w[key].double(), self.b32[key].double(), padding=1)
        if form == "direct" or key == ("down1", 0):             # the first layer is a direct fp32 kernel on every handle
            return self._direct(x, self.w[key], self.b32[key])
        if form in ("f2", "f4"):
            return self._wino(key, x, int(form[1]))
        assert form == "f4s", form
        return self._wino(key, x, 4, split=True, dev=dev)

    def convt(self, block, x, form, dev=None):
        w, b = self.w[block, "up"], self.b32[block, "up"]
        if form == "f64":
            return F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2)
        assert form in ("direct", "split"), form
        dev = dev or {}
        n, c, h, wd = x.shape
        perm = self._perm(c)
        cout = w.shape[1]
        xm = x.float().permute(0, 2, 3, 1).reshape(n * h * wd, c)[:, perm].contiguous()
        wm = w.reshape(c, cout * 4)[perm].contiguous()
        mask = perm >= c - 16
        if form == "direct":
            y = chain_matmul(xm, wm)
        elif dev.get("ksplit_bf16"):
            k = c // 8
            y = _ksplit8(xm, wm, lambda p, q, s: split_matmul(p, q, dev, mask[s * k:(s + 1) * k]), dev)
        else:
            y = split_matmul(xm, wm, dev, mask)
        if dev.get("bias_bf16"):
            b = bf16(b)
        y = y.reshape(n, h, wd, cout, 2, 2) + b[None, None, None, :, None, None]
        return y.permute(0, 3, 1, 4, 2, 5).reshape(n, cout, 2 * h, 2 * wd).double()

    # ---- blocks: form = (transposed convolution, first 3x3, second 3x3), or "f64" -------------------------------------------------
    @staticmethod
    def _forms(form):
        return ("f64",) * 3 if form == "f64" else form

    def double_conv(self, block, x, form, dev=None):
        _, f0, f3 = self._forms(form)
        dev = dev or {}
        a = F.relu(self.conv3((block, 0), x, f0, dev if dev.get("conv") == 0 else None))
        return F.relu(self.conv3((block, 3), a, f3, dev if dev.get("conv") == 3 else None))

    def up(self, block, prev, skip, form, dev=None, x1=None):
        """x1: the transposed convolution's output where the caller has it already (several deviated ones stacked as clips)."""
        dev = dev or {}
        if x1 is None:
            x1 = self.convt(block, prev, self._forms(form)[0], dev if dev.get("conv") == "up" else None)
        dy, dx = skip.shape[2] - x1.shape[2], skip.shape[3] - x1.shape[3]
        x1 = F.pad(x1, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
        return self.double_conv(block, torch.cat([skip.double(), x1], 1), form, dev)

    def out(self, t, form):
        w, b = self.w["out"], self.b32["out"]
        if form == "f64":
            return F.conv2d(t.double(), w.double(), b.double())
        return self._direct(t, w, b)

    def one(self, block, x, form, taps, dev=None):
        """z of block `block` alone (float64, after the ReLU) from the teacher inputs in `taps` (x for down1)."""
        if block in DOWN or block == "bottleneck":
            i = BLOCKS.index(block)
            cur = x.double() if i == 0 else pool_max(taps[BLOCKS[i - 1]].double())
            return self.double_conv(block, cur, form, dev)
        i = UP.index(block)
        return self.up(block, taps[BLOCKS[4 + i]].double(), taps[DOWN[3 - i]].double(), form, dev)

    def run(self, x, form="f64", rnd=False):
        """The free-running chain: block -> z.  rnd: every block output rounded to fp32 (what a device's chain stores)."""
        res = {}
        q = (lambda t: t.float().double()) if rnd else (lambda t: t)
        fm = form if isinstance(form, dict) else {b: form for b in BLOCKS}
        cur = x.double()
        for name in DOWN:
            res[name] = q(self.double_conv(name, cur, fm[name]))
            cur = pool_max(res[name])
        res["bottleneck"] = q(self.double_conv("bottleneck", cur, fm["bottleneck"]))
        prev = "bottleneck"
        for i, name in enumerate(UP):
            res[name] = q(self.up(name, res[prev], res[DOWN[3 - i]], fm[name]))
            prev = name
        return res


# ---- which forms a handle may run (choose_conv3 / choose_convt restated) -----------------------------------------------------------
CONFIGS = {"default": {}, "direct": {"ADN_CONV_ALGO": "direct"}, "tile2": {"ADN_WINO_TILE": "2"}, "tile4": {"ADN_WINO_TILE": "4"},
           "gemm0": {"ADN_WINO_GEMM": "0"}, "gemm2": {"ADN_WINO_GEMM": "2"}, "convt0": {"ADN_CONVT_SPLIT": "0"}}
AUTOMATIC = ("default", "gemm2")                    # the configurations that also run with the automatic kernel choice
CHANNELS = {"down1": (None, 64), "down2": (64, 128), "down3": (128, 256), "down4": (256, 512), "bottleneck": (512, 1024),
            "up1": (1024, 512), "up2": (512, 256), "up3": (256, 128), "up4": (128, 64)}      # the double conv's input / output channels
GEMM_GRID = 1536                                    # adn_unet::gemm_grid


def wino_ksplit(nwg, nchunk):
    """csrc/adn_internal.h: the K splits of a layer launched as `nwg` F(2x2) workgroups (16x16 pixels x 32 couts) of `nchunk` 8-channel
    chunks, while the grid stays within the chip's 512 slots and a slice keeps four chunks."""
    ks = 1
    while ks < 8 and nwg * ks * 2 <= 512 and nchunk % (ks * 2) == 0 and nchunk // (ks * 2) >= 4:
        ks *= 2
    return ks


def level_hw(f, t, level):
    return f >> level, t >> level


def f4_ok(h, w):
    """wino4_applicable without `force`: the 32x32 tiles (32x16 per clip in pair mode) waste at most a quarter of the tiled area."""
    th, tw = -(-h // 32), -(-w // 32)
    tiled = th * 32 * 16 if w <= 16 else th * tw * 1024
    return tiled * 3 <= h * w * 4


def three_stage(block, idx, n, f, t):
    """(fits, gemm grid) of the three-stage form for a layer, or None where the layer has no such form (pack_weights: levels 3 and 4
    from 512 input channels on; wino_scratch / wino3s_geom: V and M behind the layer's largest tensor in a ping-pong buffer)."""
    cin, cout = CHANNELS[block]
    if idx == 3:
        cin = cout
    if LEVEL[block] < 3 or cin is None or cin < 512 or cout % 128:
        return None
    h, w = level_hw(f, t, LEVEL[block])
    full = n * f * t * 64 * 4
    widest = max(cin // 2 if (block in UP and idx == 0) else cin, cout)
    front = n * h * w * widest * 4
    rows = n * -(-h // 4) * -(-w // 4)
    fits = front < full and 36 * rows * max(cin, cout) * 4 <= full - front
    return fits, 36 * -(-rows // 128) * (cout // 128)


def form_set(cfg, pinned, block, n, f, t):
    """The forms (transposed convolution, first 3x3, second 3x3) a handle created under CONFIGS[cfg] may run for `block` at n x f x t.

      configuration            transposed conv   3x3 layers
      direct                   split             direct
      tile2                    split             f2
      tile4                    split             f4 (forced: whatever the image size)
      gemm0 pinned             split             g = f4 where its tiles fit the image (f4_ok), else f2
      default / gemm2 pinned   split             f4s on the layers that have the form and whose V and M fit, g on the others
      convt0 pinned            direct            as default pinned
      default automatic        split             f2, and f4 where f4_ok (either may be K-split: the same arithmetic in slices);
                                                 f4s only from a GEMM grid of 1536 workgroups on, which no shape here reaches
      gemm2 automatic          split             f4s where it fits, f2 / f4 on the others
    The first layer (in_channels planes) is a direct fp32 kernel, or computed in fp32 inside the F(2x2) kernel, on every handle."""
    ct = None if block not in UP else ("direct" if cfg == "convt0" else "split")
    if cfg in ("direct", "tile2", "tile4"):
        f3 = {"direct": "direct", "tile2": "f2", "tile4": "f4"}[cfg]
        return {(ct, f3, f3)}
    h, w = level_hw(f, t, LEVEL[block])
    plain = ["f4" if f4_ok(h, w) else "f2"] if pinned else (["f2", "f4"] if f4_ok(h, w) else ["f2"])
    out = set()
    for g in plain:
        forms = []
        for idx in (0, 3):
            ts = three_stage(block, idx, n, f, t) if cfg != "gemm0" else None
            runs = ts is not None and ts[0] and (pinned or cfg == "gemm2" or ts[1] >= GEMM_GRID)
            forms.append("f4s" if runs else g)
        out.add((ct, forms[0], forms[1]))
    return out


ORDERS = (5, 6)        # seeds of the channel orders a floor is taken over


def restated(model, fn, orders=ORDERS):
    """fn() under each channel order: the restatement's values, one per order."""
    saved, res = model.perm_seed, []
    try:
        for seed in orders:
            model.perm_seed = seed
            res.append(fn())
    finally:
        model.perm_seed = saved
    return res


def floor_and_reference(model, x, taps, forms, blocks=BLOCKS, orders=ORDERS):
    """block -> (z of the float64 model, {form: (E_max, E_rms) of that form's fp32 restatement against z}), same teacher inputs.
    forms: block -> the forms to restate.  Each statistic is the larger of the restatement's in the channel orders `orders`: the
    largest element's error is set by how far the partial sums of a few outputs wander along the chain, which changes by +-20 % (up to
    1.5 x under F(4x4)) from one order to the next; one order alone understates what an order may legitimately cost."""
    out = {}
    for name in blocks:
        z = model.one(name, x, "f64", taps)
        out[name] = (z, {fm: floor_of(restated(model, lambda: block_error(model.one(name, x, fm, taps).float(), z), orders))
                         for fm in sorted(forms[name], key=str)})
    return out
