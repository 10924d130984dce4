"""The float64 model of the fp32 U-Net path and its fp32 restatements (tests/f32_model.py) checked on the CPU: the model is the
reference's network, every restatement computes the block it restates, and the bound the GPU test derives from the restatements'
floors notices one wrong thing in the split arithmetic -- or this file says where it cannot.

No device is involved: the teacher inputs are the chain of the F(2x2) / split restatement, rounded to fp32 after every block.
"""
import numpy as np
import pytest
import torch

import f32_model as fm

# A restatement with a wrong matrix entry, index or term is off by 2^-10 of a block's rms or more (16 000 fp32 ulps; the smallest
# deviation below, one constant of a transform off by 2^-10, lands at 10^3 - 10^5 ulps): 256 ulps (1.5e-5 of the rms, the size of the
# suite's chain bounds) of rms error separate a correct fp32 restatement, whatever its order, from a wrong one; the largest element
# (of 10^3 - 10^5, and F(4x4)'s A^T weighs a tile's last row and column 8 x) may be 16 x that: 4096 ulps, still a quarter of 2^-10.
FLOOR_SANE = 256.0
CASES = [("benign", s) for s in fm.SHAPES[:6]] + [("heavy", (2, 33, 47))]       # 17 x 33x47: the layers of 2 x 33x47, more clips
# the cases the deviations are tried at (each costs thirty restatements of every block the split arithmetic runs in): one pixel at the
# bottom, odd at every level, whole F(4x4) tiles at full resolution, heavy-tailed weights
DEV_CASES = [("benign", (1, 16, 16)), ("benign", (2, 33, 47)), ("benign", (1, 64, 80)), ("heavy", (2, 33, 47))]
HANDLES = [(cfg, True) for cfg in fm.CONFIGS] + [(cfg, False) for cfg in fm.AUTOMATIC]


@pytest.fixture(scope="module")
def sets():
    cache = {}

    def get(kind):
        if kind not in cache:
            sd = fm.weight_set(kind)
            cache[kind] = (sd, fm.F32Model(sd))
        return cache[kind]
    return get


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("kind", ("benign", "heavy", "trained"))
@pytest.mark.parametrize("n,f,t", [(2, 33, 47), (1, 16, 16)])
def test_free_running_model_is_the_reference_network(sets, kind, n, f, t):
    """Block by block within 1e-6 of max of the C oracle with float64 accumulation (same fold, pad / concat order and pooling; the
    oracle stores fp32 between layers), and within 2e-5 of the fp32 torch oracle (the bound the suite holds two fp32 forms of the
    whole chain to)."""
    import oracle
    from oracle import unet_torch
    sd, m = sets(kind)
    x = fm.case_input(n, f, t)
    res = m.run(torch.from_numpy(x))
    y = m.out(res["up4"], "f64").numpy()
    ref_y, ref = oracle.unet_forward(sd, x, acc64=True, want_taps=True)
    for name in fm.BLOCKS:
        assert _rel(res[name].numpy(), ref[name]) <= 1e-6, name
    assert _rel(y, ref_y) <= 1e-6
    ref_y, ref = unet_torch.unet_forward(unet_torch.to_torch_state(sd), torch.from_numpy(x), want_taps=True)
    for name in fm.BLOCKS:
        assert _rel(res[name].numpy(), ref[name].numpy()) <= 2e-5, name
    assert _rel(y, ref_y.numpy()) <= 2e-5


def _teacher(m, x):
    chain = {b: (("split" if b in fm.UP else None), "f2", "f2") for b in fm.BLOCKS}
    return {k: v.float() for k, v in m.run(x, chain, rnd=True).items()}


ALL_FORMS = ("direct", "f2", "f4", "f4s")


@pytest.mark.parametrize("kind,shape", CASES + [("trained", (2, 33, 47))], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_restatement_computes_its_block(sets, kind, shape):
    """Every form of every block, teacher-forced: finite, and within FLOOR_SANE fp32 ulps (rms; 16 x that in the largest element) of the float64 block.
    The floors are printed: form by form, max / rms."""
    _, m = sets(kind)
    x = torch.from_numpy(fm.case_input(*shape))
    taps = _teacher(m, x)
    forms = {b: {(("split" if b in fm.UP else None), g, g) for g in ALL_FORMS} | ({("direct", "direct", "direct")} if b in fm.UP else set())
             for b in fm.BLOCKS}
    fr = fm.floor_and_reference(m, x, taps, forms, orders=fm.ORDERS[:1])
    for name in fm.BLOCKS:
        z, floors = fr[name]
        assert bool(torch.isfinite(z).all()), name
        print(f"floor {kind:<7} {'x'.join(map(str, shape)):<9} {name:<10} " +
              "  ".join(f"{'+'.join(dict.fromkeys(p for p in form if p))} {e[0]:6.1f} / {e[1]:5.2f}" for form, e in floors.items()))
        for form, e in floors.items():
            assert e[0] <= 16 * FLOOR_SANE and e[1] <= FLOOR_SANE, (name, form, e)
    y_ref = m.out(taps["up4"], "f64")
    e = fm.y_error(m.out(taps["up4"], "f32").float(), y_ref)
    print(f"floor {kind:<7} {'x'.join(map(str, shape)):<9} y          1x1 {e[0]:6.1f} / {e[1]:5.2f}")
    assert e[0] <= 16 * FLOOR_SANE and e[1] <= FLOOR_SANE


def test_form_sets_follow_the_kernel_choice():
    """form_set at the geometries whose choice csrc/unet.hip's comments and the other GPU tests state."""
    # 16x16: V and M of no layer fit behind the tensors -> one-launch kernels; F(4x4) tiles waste too much of every level
    for b in fm.BLOCKS:
        assert fm.form_set("default", True, b, 1, 16, 16) == {(("split" if b in fm.UP else None), "f2", "f2")}
    # 2 x 33x47: five layers run the three-stage form on a pinned handle, none on the automatic one (4 GEMM workgroups a position)
    assert fm.form_set("default", True, "down4", 2, 33, 47) == {(None, "f2", "f4s")}
    assert fm.form_set("default", True, "bottleneck", 2, 33, 47) == {(None, "f4s", "f4s")}
    assert fm.form_set("gemm2", False, "up1", 2, 33, 47) == {("split", "f4s", "f4s")}
    assert fm.form_set("default", False, "up1", 2, 33, 47) == {("split", "f2", "f2")}
    assert fm.form_set("gemm0", True, "up1", 2, 33, 47) == {("split", "f2", "f2")}
    assert fm.form_set("convt0", True, "up1", 2, 33, 47) == {("direct", "f4s", "f4s")}
    # 64x80: 2 x 3 tiles of 32x32 cover 6144 pixels for 5120 -> F(4x4) at full resolution; 32x40 below is 1 x 2 tiles for 1280: not
    assert fm.form_set("gemm0", True, "up4", 1, 64, 80) == {("split", "f4", "f4")}
    assert fm.form_set("gemm0", True, "up3", 1, 64, 80) == {("split", "f2", "f2")}
    assert fm.form_set("default", False, "down1", 1, 64, 80) == {(None, "f2", "f2"), (None, "f4", "f4")}
    assert fm.form_set("tile4", True, "bottleneck", 1, 16, 16) == {(None, "f4", "f4")}
    # the flagship shape: 513x256 reaches 1536 GEMM workgroups at level 3 from batch 11 on (csrc/unet.hip, gemm_grid) -> the automatic
    # handle runs the form too
    assert fm.three_stage("down4", 3, 11, 513, 256) == (True, 36 * 11 * 4) and fm.three_stage("down4", 3, 10, 513, 256)[1] < fm.GEMM_GRID
    assert fm.form_set("default", False, "down4", 11, 513, 256) == {(None, "f2", "f4s"), (None, "f4", "f4s")}
    assert fm.three_stage("down4", 0, 64, 513, 256) is None


# ---- the condition that keeps the bound honest -------------------------------------------------------------------------------------
# name -> (dev keys, where it applies: "up" = the transposed convolution, "3x3" = a three-stage layer)
DEV = {
    "drop hi.lo": ({"drop": "hi.lo"}, ("up", "3x3")),
    "drop lo.hi": ({"drop": "lo.hi"}, ("up", "3x3")),
    "drop mid.mid": ({"drop": "mid.mid"}, ("up", "3x3")),
    "weights' lo plane zero, last 16 channels": ({"wlo16": True}, ("up", "3x3")),
    "3x3 tap (1,2) * (1 + 2^-12)": ({"tap": True}, ("3x3",)),
    "bias rounded to bf16": ({"bias_bf16": True}, ("up", "3x3")),
    "one of 8 K-split copies rounded to bf16": ({"ksplit_bf16": True}, ("up",)),        # only the transposed convolutions are cut along K
    "at6: 2 -> 2 (1 + 2^-10)": ({"at": True}, ("3x3",)),
    "bt6: -5 -> -5 (1 + 2^-10)": ({"bt": True}, ("3x3",)),
}
# What a block output cannot show at the fp32 floor, whatever the form set (profiles/f32_blocks.md):
#  * the lo plane of 16 of K >= 128 channels: 2^-17 of sqrt(16 / K) of the sum, 1 - 4 fp32 ulps before two 3x3 layers spread it;
#  * a product dropped from a transposed convolution, seen through the block's two 3x3 layers: 27 - 31 ulps rms at the layer's own
#    output, half of the next layer's input channels, against a block floor of sqrt(K / 24) = 10 - 20 ulps at the deep levels
#    (K = 4608 - 9216).  Held to: the handles whose 3x3 layers add the least (direct fp32, F(2x2)) notice at least one dropped product
#    on at least one block in every case -- "covered" as profiles/f32_blocks.md defines it; block by block the ratios are printed.
NOT_SEPARABLE = ("weights' lo plane zero, last 16 channels",)
DROPPED = ("drop hi.lo", "drop lo.hi", "drop mid.mid")
CONVT_COVERED = ("direct", "tile2")


def _asserted(where, name, cfg, pinned):
    """Whether the bound of this handle must notice the deviation on every block it applies to.  Three-stage layers: every handle
    that runs exactly that form (pinned, or ADN_WINO_GEMM=2).  Transposed convolution: every handle for the bias and the K-split
    copy; the dropped products through CONVT_COVERED above."""
    if name in NOT_SEPARABLE:
        return False
    return (pinned or cfg == "gemm2") if where == "3x3" else name not in DROPPED


@pytest.mark.parametrize("kind,shape", DEV_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_one_deviation_in_the_split_arithmetic_lands_outside_the_bound(sets, kind, shape):
    _, m = sets(kind)
    n, f, t = shape
    x = torch.from_numpy(fm.case_input(n, f, t))
    taps = _teacher(m, x)
    label = f"{kind} {'x'.join(map(str, shape))}"
    missed, seen = [], {cfg: 0.0 for cfg in CONVT_COVERED}
    for block in fm.BLOCKS:
        sets_of = {h: fm.form_set(*h, block, n, f, t) for h in HANDLES}
        forms = set().union(*sets_of.values())
        targets = []                                           # (where, conv, the forms whose arithmetic it is)
        if block in fm.UP:
            targets.append(("up", "up", {fo for fo in forms if fo[0] == "split"}))
        for idx in (0, 3):
            hit = {fo for fo in forms if fo[1 + idx // 3] == "f4s"}
            if hit:
                targets.append(("3x3", idx, hit))
        if not targets:
            continue
        z, floors = fm.floor_and_reference(m, x, taps, {block: forms}, [block])[block]
        for where, conv, hit in targets:
            names = [name for name, (_, applies) in DEV.items() if where in applies]
            errors = {}                                        # (name, form) -> E of the deviated block
            if where == "up":                                  # the deviated layer outputs stacked as clips: one pass through the 3x3 layers
                i = fm.UP.index(block)
                prev, skip = taps[fm.BLOCKS[4 + i]].double(), taps[fm.DOWN[3 - i]].double()
                x1 = torch.cat([m.convt(block, prev, "split", DEV[name][0]) for name in names], 0)
                for form in hit:
                    outs = m.up(block, None, skip.repeat(len(names), 1, 1, 1), form, x1=x1).float().chunk(len(names), 0)
                    errors.update({(name, form): fm.block_error(o, z) for name, o in zip(names, outs)})
            else:
                errors = {(name, form): fm.block_error(m.one(block, x, form, taps, dict(DEV[name][0], conv=conv)).float(), z)
                          for name in names for form in hit}
            for name in names:
                worst = {}
                for form in sorted(hit, key=str):
                    e = errors[name, form]
                    for h, s in sets_of.items():
                        if form in s:
                            b = fm.bound(fm.floor_of([floors[fo] for fo in s]))
                            r = (max(e[0] / b[0], e[1] / b[1]), e[0] / b[0], e[1] / b[1])
                            worst[h] = min(worst.get(h, r), r)
                for (cfg, pinned), (r, r_max, r_rms) in worst.items():
                    must = _asserted(where, name, cfg, pinned)
                    if where == "up" and name in DROPPED and cfg in seen:
                        seen[cfg] = max(seen[cfg], r)
                    print(f"deviation {label:<16} {block:<10} conv {str(conv):<3} {name:<40} {cfg:<8}{'pinned' if pinned else 'auto':<7}"
                          f" E / bound = {r:8.2f} (max {r_max:6.2f}, rms {r_rms:6.2f}) {'' if r > 1 else ('HIDDEN' if not must else 'MISSED')}")
                    if must and not r > 1:
                        missed.append((block, conv, name, cfg, pinned, r))
    print(f"deviation {label:<16} a product dropped from a transposed convolution, largest E / bound over blocks and products: " +
          ", ".join(f"{cfg} {r:.2f}" for cfg, r in seen.items()))
    assert not missed, (label, missed)
    assert all(r > 1 for r in seen.values()), (label, seen)
