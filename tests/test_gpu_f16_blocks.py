"""Every block of the fp16 U-Net path against a float64 model of its own arithmetic (tests/f16_model.py), teacher-forced on the
device's block outputs: E = max over ALL elements of |tap - z| / ulp16(max(|z|, rms(z))) must stay within 2 * max(E_ref, 1), where
E_ref is the same measure for an fp32 accumulation in another channel order, computed here from the same inputs.  The factor 2 is
the margin over that floor: MFMA block order and K-split slices associate differently from the stand-in.  The bound comes out at
2 - 4 units; the fp32-referenced tests of this path allow about 100 (5e-2 of a block's rms).

Handles are created under their switches (read once, when the handle is created): default, ADN_F16_FIRST=0 (conv_first_kernel
instead of conv16_f16's FIRST form), ADN_F16_CONV=32 (conv_dma<_Float16> on every 3x3 layer), ADN_F16_CONVT=dma (conv_dma<_Float16>
instead of convt16_f16), each with set_batch_invariant(True) and without -- without it small batches run the deep 3x3 layers as
conv_dma<_Float16> K-split slices plus a reduce launch.  Shapes and what each crosses: f16_model.SHAPES.

The pooled tensors are not exported: the pooling epilogue of a down block is checked through the next block, whose model input is
the pool of the exported skip.

What the model knows about a handle: whether Conv2d(1 -> 64) runs inside conv16_f16 (fp16 weights, input and bias as two fp16
terms each) and whether the fused 1x1 tail contracts unrounded accumulators (conv16_f16) or staged fp16 values (conv_dma).
"""
import os

import numpy as np
import pytest
import torch

import f16_model as fm

pytestmark = pytest.mark.gpu

ENV_KEYS = ("ADN_BATCH_INVARIANT", "ADN_F16_FIRST", "ADN_F16_CONV", "ADN_F16_CONVT")
CONFIGS = {"default": {}, "first0": {"ADN_F16_FIRST": "0"}, "conv32": {"ADN_F16_CONV": "32"}, "convt_dma": {"ADN_F16_CONVT": "dma"}}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _net(sd, dev, env, pinned, dtype="f16", in_ch=1, classes=1):
    """A network whose handle is created under `env`: the environment is set around the first forward and restored after it."""
    from audiodenoiser_amd.model import UNet
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    try:
        m = UNet(in_ch, classes)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).eval().set_compute_dtype(dtype)
        if pinned:
            m.set_batch_invariant(True)
        with torch.no_grad():
            m(torch.zeros((1, in_ch, 16, 16), device=dev))
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return m


@pytest.fixture(scope="module")
def nets(dev):
    """(weight set, config, pinned) -> network, packed once per module."""
    cache, sds = {}, {}

    def sd(kind):
        if kind not in sds:
            sds[kind] = fm.weight_set(kind)
        return sds[kind]

    def get(kind, cfg, pinned):
        if (kind, cfg, pinned) not in cache:
            cache[kind, cfg, pinned] = _net(sd(kind), dev, CONFIGS[cfg], pinned)
        return cache[kind, cfg, pinned]
    get.sd = sd
    return get


@pytest.fixture(scope="module")
def models():
    """(weight set, fused first) -> F16Model (a few seconds of fp16 rounding of 31 M weights, once)."""
    cache = {}

    def get(kind, fused, sd):
        if (kind, fused) not in cache:
            cache[kind, fused] = fm.F16Model(sd, fused_first=fused)
        return cache[kind, fused]
    return get


def _check(net, model, x_np, dev, label, tail_unrounded):
    """One forward with block outputs and one without; every block and both outputs against the model.  Returns (y_taps, y, taps)."""
    x = torch.from_numpy(x_np)
    with torch.no_grad():
        y_t, taps_d = net(x.to(dev), return_taps=True)
        y_p = net(x.to(dev))
        torch.cuda.synchronize()
    taps = {k: v.cpu() for k, v in taps_d.items()}
    y_t, y_p = y_t.cpu(), y_p.cpu()
    assert torch.equal(taps["out"], y_t)
    for name in fm.BLOCKS:                                     # the exported block outputs are fp16 values
        assert torch.equal(taps[name], fm.r16(taps[name])), (label, name)
    fr = fm.floor_and_reference(model, x, taps)
    failed = []
    for name in fm.BLOCKS:
        z, e_ref = fr[name]
        e = fm.block_error(taps[name], z)
        print(f"f16 blocks {label:<36} {name:<10} E = {e:6.2f}  E_ref = {e_ref:5.2f}  bound {fm.bound(e_ref):5.2f}")
        if not e <= fm.bound(e_ref):
            failed.append((name, e, e_ref))
    # outputs: the taps path runs conv_out_kernel on the fp16 up4 tensor; the production path's fused tail contracts the unrounded
    # ReLU(accumulator) values where conv16_f16 runs it, the staged fp16 values where conv_dma does
    ref_t = model.out(taps["up4"], "f64")
    eref_t = fm.y_error(model.out(taps["up4"], "f32"), ref_t)
    if tail_unrounded:
        ref_p = model.out(fr["up4"][0], "f64")
        eref_p = fm.y_error(model.out(model.one("up4", x, "f32", taps)[1], "f32"), ref_p)
    else:
        ref_p, eref_p = ref_t, eref_t
    for name, y, ref, e_ref in (("y (taps run)", y_t, ref_t, eref_t), ("y", y_p, ref_p, eref_p)):
        e = fm.y_error(y, ref)
        print(f"f16 blocks {label:<36} {name:<10} E = {e:6.2f}  E_ref = {e_ref:5.2f}  bound {fm.bound(e_ref):5.2f}")
        if not e <= fm.bound(e_ref):
            failed.append((name, e, e_ref))
    assert not failed, (label, failed)
    return y_t, y_p, taps


def _fused_first(cfg, in_ch=1):
    return in_ch == 1 and cfg in ("default", "convt_dma")      # choose_conv3: first && f16_fuse_first && the conv16 weights are there


@pytest.mark.parametrize("n,f,t", fm.SHAPES, ids=["x".join(map(str, s)) for s in fm.SHAPES])
@pytest.mark.parametrize("pinned", [False, True], ids=["auto", "pinned"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_block_within_twice_the_floor(nets, models, dev, cfg, pinned, n, f, t):
    sd = nets.sd("benign")
    net = nets("benign", cfg, pinned)
    model = models("benign", _fused_first(cfg), sd)
    label = f"{cfg} {'pinned' if pinned else 'auto'} {n}x{f}x{t}"
    y_t, y_p, _ = _check(net, model, fm.case_input(n, f, t), dev, label, tail_unrounded=cfg != "conv32")
    if cfg != "conv32":
        assert not torch.equal(y_t, y_p), label               # conv16_f16's fused tail did run: it contracts unrounded values


@pytest.mark.parametrize("n,f,t", fm.HEAVY_SHAPES, ids=["x".join(map(str, s)) for s in fm.HEAVY_SHAPES])
@pytest.mark.parametrize("pinned", [False, True], ids=["auto", "pinned"])
def test_every_block_within_twice_the_floor_heavy_tailed_weights(nets, models, dev, pinned, n, f, t):
    sd = nets.sd("heavy")
    _check(nets("heavy", "default", pinned), models("heavy", True, sd), fm.case_input(n, f, t), dev,
           f"heavy default {'pinned' if pinned else 'auto'} {n}x{f}x{t}", tail_unrounded=True)


def test_the_switches_select_other_kernels(nets, dev):
    """The default handle and the ADN_F16_CONV=32 handle differ in the last bits (other kernels ran); at 17 x 33x47 no layer of the
    default handle is cut along K, so it runs the pinned handle's kernels bit for bit, and at 2 x 33x47 it does not."""
    with torch.no_grad():
        x = torch.from_numpy(fm.case_input(2, 33, 47)).to(dev)
        ya, yp, y32 = nets("benign", "default", False)(x), nets("benign", "default", True)(x), nets("benign", "conv32", True)(x)
        assert not torch.equal(yp, y32)
        assert not torch.equal(ya, yp)                          # K-split slices + reduce launch at the deep levels
        assert not torch.equal(nets("benign", "first0", True)(x), yp)
        assert not torch.equal(nets("benign", "convt_dma", True)(x), yp)
        x = torch.from_numpy(fm.case_input(17, 33, 47)).to(dev)
        assert torch.equal(nets("benign", "default", False)(x), nets("benign", "default", True)(x))


@pytest.mark.parametrize("cin,k,shape", fm.PLANES, ids=[f"c{c}k{k}-" + "x".join(map(str, s)) for c, k, s in fm.PLANES])
def test_many_input_planes_and_classes(dev, cin, k, shape):
    """The first layer on its own launch (conv_first_kernel: several planes, rows cut into column tiles, up to exactly 160 KiB of LDS
    at 64 planes) and the output convolution class by class.  fp16: every block within twice the floor; fp32: 1e-4 of max against
    the torch oracle."""
    from oracle import unet_torch
    sd = fm.weight_set("benign", cin, k)
    x = fm.case_input(*shape, in_channels=cin)
    net = _net(sd, dev, {}, False, "f16", cin, k)
    _check(net, fm.F16Model(sd), x, dev, f"UNet({cin},{k}) " + "x".join(map(str, shape)), tail_unrounded=k == 1)
    ref_y, ref = unet_torch.unet_forward(unet_torch.to_torch_state(sd), torch.from_numpy(x), want_taps=True)
    net32 = _net(sd, dev, {}, False, "f32", cin, k)
    with torch.no_grad():
        y, taps = net32(torch.from_numpy(x).to(dev), return_taps=True)
        y_plain = net32(torch.from_numpy(x).to(dev))
    for name in fm.BLOCKS:
        e = float((taps[name].cpu() - ref[name]).abs().max() / ref[name].abs().max())
        assert e <= 1e-4, (name, e)
    for got in (y, y_plain):
        e = float((got.cpu() - ref_y).abs().max() / ref_y.abs().max())
        print(f"UNet({cin},{k}) f32 {shape}: {e:.2e} of max|y| (bound 1e-4)")
        assert got.shape == ref_y.shape and e <= 1e-4, e
