"""Every block of the fp32 U-Net path against a float64 model (tests/f32_model.py), teacher-forced on the device's own block outputs,
at the fp32 floor: E = |tap - z| / ulp32(max(|z|, rms z)), as its maximum and as its root mean square over all elements, must each
stay within 2 * max(floor, 1).  The floor is the same statistic for an fp32 restatement, in another summation order, of every
arithmetic the handle may run for that block (f32_model.form_set: direct fp32, Winograd F(2x2) / F(4x4), the three-term bf16 split of
the transposed convolutions and of the three-stage form's GEMMs), computed here from the same inputs.  The chain-sized bounds of the
other fp32 tests (1e-4 of max against the oracle, 2e-5 between two kernel choices) are hundreds of fp32 ulps per element.

Handles are created under their switches (read once, when the handle is created), each pinned (set_batch_invariant); the default and
the ADN_WINO_GEMM=2 handle also with the automatic kernel choice, where one to three clips run K-split slices + a reduce launch
(wino_ksplit, wino4_ksplit, convt_ksplit).  Which form ran is shown by bit-inequality between handles only.

The pooled tensors are not exported: the pooling epilogue of a down block is checked through the next block.  The production output
(fused first layer, fused 1x1 tail) contracts the unrounded fp32 values of up4: its reference is the 1x1 convolution of the model's up4.

One line per block is printed: label, block, E, floor, bound (max / rms); profiles/f32_blocks.md holds a run's table.
"""
import os

import numpy as np
import pytest
import torch

import f32_model as fm

pytestmark = pytest.mark.gpu

ENV_KEYS = ("ADN_BATCH_INVARIANT", "ADN_CONV_ALGO", "ADN_WINO_TILE", "ADN_WINO_GEMM", "ADN_CONVT_SPLIT", "ADN_WINO_SPLITK",
            "ADN_AUTO_GRID", "ADN_AUTO_GRID64")
HANDLES = [(cfg, True) for cfg in fm.CONFIGS] + [(cfg, False) for cfg in fm.AUTOMATIC]
SHAPES = fm.SHAPES[:7]            # (1,16,16) (2,33,47) (3,40,33) (2,31,16) (1,16,130) (1,64,80) (17,33,47): what each crosses is in f16_model
# level 3 is 8 x 15: 2 x 4 tiles of 4x4 outputs a clip (the last column of tiles partial), 136 GEMM rows = one whole 128-row tile + 8
# rows; V and M of every three-stage layer fit (20 MB of the 29 MB behind the level's tensors)
GEMM_ROWS_SHAPE = (17, 64, 120)
HEAVY_SHAPES = ((2, 33, 47), (1, 64, 80))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _net(sd, dev, env, pinned, in_ch=1, classes=1):
    """An fp32 network whose handle is created under `env`: the environment is set around the first forward and restored after it."""
    from audiodenoiser_amd.model import UNet
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    try:
        m = UNet(in_ch, classes)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).eval().set_compute_dtype("f32")
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
    """(weight set, config, pinned) -> network, and weight set -> F32Model; packed once per module."""
    cache, sds, models = {}, {}, {}

    def sd(kind):
        if kind not in sds:
            sds[kind] = fm.weight_set(kind)
        return sds[kind]

    def get(kind, cfg, pinned):
        if (kind, cfg, pinned) not in cache:
            cache[kind, cfg, pinned] = _net(sd(kind), dev, fm.CONFIGS[cfg], pinned)
        return cache[kind, cfg, pinned]

    def model(kind):
        if kind not in models:
            models[kind] = fm.F32Model(sd(kind))
        return models[kind]
    get.model = model
    return get


def _line(label, name, e, floor, b):
    print(f"f32 blocks {label:<34} {name:<12} E = {e[0]:7.2f} / {e[1]:5.2f}  floor {floor[0]:7.2f} / {floor[1]:5.2f}  "
          f"bound {b[0]:7.2f} / {b[1]:5.2f}")


def _check(net, model, x_np, dev, label, cfg, pinned, blocks=fm.BLOCKS, fused_tail=True):
    """One forward with block outputs and one without; `blocks` and (with all nine) both outputs against the model."""
    x = torch.from_numpy(x_np)
    n, _, f, t = x.shape
    with torch.no_grad():
        y_t, taps_d = net(x.to(dev), return_taps=True)
        y_p = net(x.to(dev))
        torch.cuda.synchronize()
    taps = {k: v.cpu() for k, v in taps_d.items()}
    y_t, y_p = y_t.cpu(), y_p.cpu()
    assert torch.equal(taps["out"], y_t)
    for name in fm.BLOCKS:
        assert taps[name].dtype == torch.float32 and bool(torch.isfinite(taps[name]).all()), (label, name)
    forms = {name: fm.form_set(cfg, pinned, name, n, f, t) for name in blocks}
    fr = fm.floor_and_reference(model, x, taps, forms, blocks)
    failed = []

    def judge(name, e, floor):
        b = fm.bound(floor)
        _line(label, name, e, floor, b)
        if not fm.within(e, b):
            failed.append((name, e, floor))

    for name in blocks:
        z, floors = fr[name]
        judge(name, fm.block_error(taps[name], z), fm.floor_of(floors.values()))
    if len(blocks) == len(fm.BLOCKS):
        ref_t = model.out(taps["up4"], "f64")
        floor_t = fm.floor_of(fm.restated(model, lambda: fm.y_error(model.out(taps["up4"], "f32").float(), ref_t)))
        judge("y (taps run)", fm.y_error(y_t, ref_t), floor_t)
        if fused_tail:                                         # one class: the tail contracts the kernel's own unrounded up4 values
            ref_p = model.out(fr["up4"][0], "f64")
            floor_p = fm.floor_of([e for form in forms["up4"] for e in fm.restated(
                model, lambda: fm.y_error(model.out(model.one("up4", x, form, taps).float(), "f32").float(), ref_p))])
        else:                                                  # several classes: conv_out_kernel on the up4 tensor in both runs
            ref_p, floor_p = ref_t, floor_t
        judge("y", fm.y_error(y_p, ref_p), floor_p)
    assert not failed, (label, failed)
    return y_t, y_p


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.mark.parametrize("n,f,t", SHAPES, ids=_ids(SHAPES))
@pytest.mark.parametrize("cfg,pinned", HANDLES, ids=[f"{c}-{'pinned' if p else 'auto'}" for c, p in HANDLES])
def test_every_block_within_twice_the_floor(nets, dev, cfg, pinned, n, f, t):
    _check(nets("benign", cfg, pinned), nets.model("benign"), fm.case_input(n, f, t), dev,
           f"{cfg} {'pinned' if pinned else 'auto'} {n}x{f}x{t}", cfg, pinned)


@pytest.mark.parametrize("cfg,pinned", [("default", True), ("gemm2", True), ("gemm2", False)], ids=["default-pinned", "gemm2-pinned", "gemm2-auto"])
def test_three_stage_gemm_with_a_partial_last_row_tile(nets, dev, cfg, pinned):
    """136 GEMM rows at level 3 (one whole 128-row tile and 8 rows), 34 at level 4: the blocks that run the three-stage form."""
    n, f, t = GEMM_ROWS_SHAPE
    for block, idx in (("down4", 3), ("bottleneck", 0), ("bottleneck", 3), ("up1", 0), ("up1", 3)):
        assert fm.three_stage(block, idx, n, f, t)[0], (block, idx)
    _check(nets("benign", cfg, pinned), nets.model("benign"), fm.case_input(n, f, t), dev,
           f"{cfg} {'pinned' if pinned else 'auto'} {n}x{f}x{t}", cfg, pinned, blocks=("down4", "bottleneck", "up1"))


@pytest.mark.parametrize("n,f,t", HEAVY_SHAPES, ids=_ids(HEAVY_SHAPES))
@pytest.mark.parametrize("cfg,pinned", [(c, p) for c in fm.AUTOMATIC for p in (True, False)],
                         ids=[f"{c}-{'pinned' if p else 'auto'}" for c in fm.AUTOMATIC for p in (True, False)])
def test_every_block_within_twice_the_floor_heavy_tailed_weights(nets, dev, cfg, pinned, n, f, t):
    _check(nets("heavy", cfg, pinned), nets.model("heavy"), fm.case_input(n, f, t), dev,
           f"heavy {cfg} {'pinned' if pinned else 'auto'} {n}x{f}x{t}", cfg, pinned)


@pytest.mark.parametrize("cfg,pinned", [(c, p) for c in fm.AUTOMATIC for p in (True, False)],
                         ids=[f"{c}-{'pinned' if p else 'auto'}" for c in fm.AUTOMATIC for p in (True, False)])
def test_every_block_within_twice_the_floor_trained_like_weights(nets, dev, cfg, pinned):
    """Folded BatchNorm scales from 0 to 47 (tests/test_f32_model_host.py: the floors of this set stay finite)."""
    _check(nets("trained", cfg, pinned), nets.model("trained"), fm.case_input(2, 33, 47), dev,
           f"trained {cfg} {'pinned' if pinned else 'auto'} 2x33x47", cfg, pinned)


@pytest.mark.parametrize("cin,k,shape", fm.PLANES, ids=[f"c{c}k{k}-" + "x".join(map(str, s)) for c, k, s in fm.PLANES])
def test_many_input_planes_and_classes(dev, cin, k, shape):
    """The first layer on its own launch (conv_first_kernel<float>: several planes, rows cut into column tiles, up to exactly 160 KiB
    of LDS at 64 planes) and the output convolution class by class, on the default handle with the automatic kernel choice."""
    sd = fm.weight_set("benign", cin, k)
    _check(_net(sd, dev, {}, False, cin, k), fm.F32Model(sd), fm.case_input(*shape, in_channels=cin), dev,
           f"UNet({cin},{k}) " + "x".join(map(str, shape)), "default", False, fused_tail=k == 1)


def test_the_switches_select_other_kernels(nets, dev):
    """Bit-inequality between handles: the three-stage form ran (ADN_WINO_GEMM=2 against 0, at a shape where V and M fit), the
    split-bf16 transposed convolution ran (default against ADN_CONVT_SPLIT=0), F(2x2) and F(4x4) ran (ADN_WINO_TILE=2 against 4), and
    two clips run K-split slices on the automatic handle (down1 already: 36 workgroups of 8 chunks).

    17 clips of 33x47: the fp16 path's rule cuts nothing there, and the automatic fp16 handle equals the pinned one bit for bit
    (test_gpu_f16_blocks.py).  The fp32 rules differ: wino_ksplit still cuts the level-1 and level-2 layers in two (136 workgroups of
    8 / 16 chunks against 512 slots), and a pinned handle takes the three-stage form wherever it fits while the automatic one waits
    for 1536 GEMM workgroups (choose_conv3) -- so the outputs differ by design, and what is bit-equal is what the rules leave alone:
    level 0 (306 workgroups, no cut), i.e. the down1 tap."""
    def run(cfg, pinned, x):
        with torch.no_grad():
            y, taps = nets("benign", cfg, pinned)(x, return_taps=True)
        return y, taps
    x = torch.from_numpy(fm.case_input(2, 33, 47)).to(dev)
    y = {h: run(*h, x) for h in (("gemm2", True), ("gemm0", True), ("convt0", True), ("default", True), ("tile2", True), ("tile4", True),
                                 ("default", False))}
    assert fm.three_stage("bottleneck", 3, 2, 33, 47)[0]
    assert not torch.equal(y["gemm2", True][0], y["gemm0", True][0])
    assert not torch.equal(y["convt0", True][0], y["default", True][0])
    assert not torch.equal(y["tile2", True][0], y["tile4", True][0])
    assert not torch.equal(y["default", False][0], y["default", True][0])
    assert fm.wino_ksplit(2 * 9 * 2, 8) == 2 and not torch.equal(y["default", False][1]["down1"], y["default", True][1]["down1"])
    assert torch.equal(y["default", True][0], y["gemm2", True][0])        # pinned: the three-stage form wherever it fits, as ADN_WINO_GEMM=2
    x = torch.from_numpy(fm.case_input(17, 33, 47)).to(dev)
    (ya, ta), (yp, tp) = run("default", False, x), run("default", True, x)
    assert fm.wino_ksplit(17 * 9 * 2, 8) == 1 and torch.equal(ta["down1"], tp["down1"])
    assert fm.wino_ksplit(17 * 2 * 4, 8) == 2 and not torch.equal(ta["down2"], tp["down2"])
    assert not torch.equal(ya, yp)
