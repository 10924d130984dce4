"""The float64 model of the fp16 U-Net path (tests/f16_model.py) checked on the CPU: it is the reference's network, its fp16 roundings
cost what the fp16 path is allowed today, the inputs the GPU test uses are benign (an fp32 accumulation in another order stays within
2.5 units of the model in every block), and one wrong term in one block lands beyond the GPU test's bound.

The stand-in for the device is the model itself in mode "f32": fp32 accumulation with the input channels permuted.
"""
import numpy as np
import pytest
import torch

import f16_model as fm

FLOOR_MAX = 2.5      # per block, teacher-forced: measured 0.50 - 1.96


@pytest.fixture(scope="module")
def sets():
    cache = {}

    def get(kind, cin=1, k=1):
        if (kind, cin, k) not in cache:
            cache[kind, cin, k] = fm.weight_set(kind, cin, k)
        return cache[kind, cin, k]
    return get


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("kind", fm.WEIGHT_SETS)
@pytest.mark.parametrize("n,f,t", [(2, 33, 47), (1, 16, 16)])
def test_without_rounding_the_model_is_the_reference_network(sets, kind, n, f, t):
    """Every fp16 rounding switched off: the block outputs of the free-running float64 model equal the C oracle's (float64
    accumulation) to 1e-6 of max -- same fold, same pad / concat order, same pooling."""
    import oracle
    sd = sets(kind)
    x = fm.case_input(n, f, t)
    ref_y, ref = oracle.unet_forward(sd, x, acc64=True, want_taps=True)
    m = fm.F16Model(sd, rounding=False)
    res = m.run(torch.from_numpy(x), "f64")
    for name in fm.BLOCKS:
        assert _rel(res[name][0].numpy(), ref[name]) <= 1e-6, name
    assert _rel(m.out(res["up4"][0], "f64").numpy(), ref_y) <= 1e-6


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", fm.WEIGHT_SETS)
def test_free_running_model_is_within_the_fp16_paths_bound_of_fp32(sets, kind, fused):
    """Nine blocks of fp16 storage: within 1e-2 of max of the fp32 oracle, the bound the fp16 path is held to."""
    from oracle import unet_torch
    sd = sets(kind)
    x = torch.from_numpy(fm.case_input(2, 33, 47))
    ref_y, ref = unet_torch.unet_forward(unet_torch.to_torch_state(sd), x, want_taps=True)
    m = fm.F16Model(sd, fused_first=fused)
    res = m.run(x, "f64")
    for name in fm.BLOCKS:
        assert _rel(res[name][0].numpy(), ref[name].numpy()) <= 1e-2, name
    assert _rel(m.out(res["up4"][0], "f64").numpy(), ref_y.numpy()) <= 1e-2


def _floor_case(sd, x, fused, label):
    """Floor of every block and of both outputs on the fp32 mode's own chain; asserts finiteness and the floor's bound."""
    m = fm.F16Model(sd, fused_first=fused)
    taps = {k: v[0] for k, v in m.run(x, "f32").items()}
    fr = fm.floor_and_reference(m, x, taps)
    for name, (z, e_ref) in fr.items():
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(taps[name]).all()), (label, name)
    y_tap = fm.y_error(m.out(taps["up4"], "f32"), m.out(taps["up4"], "f64"))
    y_prod = fm.y_error(m.out(m.one("up4", x, "f32", taps)[1], "f32"), m.out(fr["up4"][0], "f64"))
    row = [fr[name][1] for name in fm.BLOCKS] + [y_tap, y_prod]
    print(f"floor {label:<34} " + " ".join(f"{e:5.2f}" for e in row))
    for name, e in zip(fm.BLOCKS + ("y_taps", "y_fused"), row):
        assert e <= FLOOR_MAX, (label, name, e)
    return row


def test_floor_of_every_case_of_the_gpu_test(sets):
    """The inputs are benign: an fp32 accumulation in another channel order is within 2.5 units of the float64 model in every block
    of every (weights, shape, first-layer form) the GPU test runs, and every value is finite."""
    print("floor: E_ref per block, teacher-forced on the fp32 mode's own chain\n" + " " * 41 +
          " ".join(f"{b[:5]:>5}" for b in fm.BLOCKS + ("y_tap", "y_fus")))
    for kind in fm.WEIGHT_SETS:
        for n, f, t in (fm.SHAPES if kind == "benign" else fm.HEAVY_SHAPES):
            x = torch.from_numpy(fm.case_input(n, f, t))
            for fused in (False, True):
                _floor_case(sets(kind), x, fused, f"{kind} {n}x{f}x{t} {'fused' if fused else 'plain'} first")
    for cin, k, (n, f, t) in fm.PLANES:
        x = torch.from_numpy(fm.case_input(n, f, t, cin))
        _floor_case(sets("benign", cin, k), x, False, f"UNet({cin},{k}) {n}x{f}x{t}")


# ---- sensitivity: one wrong term in the stand-in device must land beyond the GPU test's bound -----------------------------------

@pytest.fixture(scope="module")
def clean(sets):
    """The clean model at 2 x 33x47, its fp32 chain as teacher inputs, and per block the float64 z and the floor."""
    m = fm.F16Model(sets("benign"))
    x = torch.from_numpy(fm.case_input(2, 33, 47))
    taps = {k: v[0] for k, v in m.run(x, "f32").items()}
    return m, x, taps, fm.floor_and_reference(m, x, taps)


def _block_input(m, block, x, taps):
    """The tensor the block's first 3x3 conv reads (for an up block: the skip channels; its up channels come behind them)."""
    i = fm.BLOCKS.index(block)
    if block in fm.UP:
        return taps[fm.DOWN[3 - fm.UP.index(block)]]
    return x if i == 0 else m.pool(taps[fm.BLOCKS[i - 1]])


def _alive(t):
    """The channel with the largest mean magnitude (a dead channel shows nothing)."""
    return int(t.abs().mean(dim=(0, 2, 3)).argmax())


def _assert_beyond(clean, mut, block, what):
    m, x, taps, fr = clean
    z, e_ref = fr[block]
    out = mut.one(block, x, "f32", taps)[0]
    e = fm.block_error(out, z)
    u = fm.ulp16(torch.maximum(z.abs(), z.pow(2).mean().sqrt()))
    frac = float((((out - z).abs() / u) > fm.bound(e_ref)).double().mean())
    print(f"mutation {what:<44} {block:<10} E = {e:8.1f}  bound {fm.bound(e_ref):.2f}  beyond it {100 * frac:.2f} % of the elements")
    assert e > fm.bound(e_ref), (what, block, e, e_ref)


@pytest.mark.parametrize("block", ["down2", "down4", "bottleneck", "up1", "up2", "up4"])
def test_one_input_channel_tap_zeroed_in_a_3x3_conv(clean, block):
    m, x, taps, _ = clean
    mut = m.mutated()
    ci = _alive(_block_input(m, block, x, taps))
    mut.w[block, 0][:, ci, 0, 2] = 0.0                          # tap (dy, dx) = (0, 2): the upper right neighbour
    _assert_beyond(clean, mut, block, f"3x3 term (channel {ci}, tap 0,2) zeroed")


@pytest.mark.parametrize("block", fm.UP)
def test_one_input_channel_tap_zeroed_in_a_transposed_conv(clean, block):
    m, x, taps, _ = clean
    mut = m.mutated()
    ci = _alive(taps[fm.BLOCKS[4 + fm.UP.index(block)]])
    mut.w[block, "up"][ci, :, 1, 0] = 0.0
    _assert_beyond(clean, mut, block, f"transposed-conv term (channel {ci}, tap 1,0) zeroed")


@pytest.mark.parametrize("block", fm.UP)
def test_pad_offset_of_the_concat_off_by_one(clean, block):
    mut = clean[0].mutated()
    mut.pad_shift[block] = 1
    _assert_beyond(clean, mut, block, "pad offset of the virtual concat + 1")


@pytest.mark.parametrize("block", ["down2", "down3", "down4", "bottleneck"])
def test_pooling_takes_the_first_of_a_pair(clean, block):
    mut = clean[0].mutated()
    mut.pool = fm.pool_first_of_pair
    _assert_beyond(clean, mut, block, "pooling: first column of the pair, not the max")


@pytest.mark.parametrize("block,idx,lo", [("down3", 3, 32), ("bottleneck", 0, 480), ("up2", 0, 480), ("up4", 3, 32)])
def test_one_k_chunk_of_32_channels_left_out(clean, block, idx, lo):
    mut = clean[0].mutated()
    assert mut.w[block, idx].shape[1] >= lo + 32
    mut.w[block, idx][:, lo:lo + 32] = 0.0
    _assert_beyond(clean, mut, block, f"conv {idx}: channels {lo}..{lo + 31} left out")


def test_fused_first_layer_differs_from_the_plain_one_by_rounding_only(sets):
    """The two forms of Conv2d(1 -> 64) the model knows are both needed (they differ by more than the GPU test's bound allows
    for in places) and both honest (they differ by fp16 weight rounding only: 2^-11 relative per term)."""
    sd = sets("benign")
    x = torch.from_numpy(fm.case_input(2, 33, 47))
    plain, fused = fm.F16Model(sd), fm.F16Model(sd, fused_first=True)
    a = plain._apply(torch.nn.functional.conv2d, x, plain.w["down1", 0], plain.b["down1", 0], "f64", 1, padding=1)
    b = fused._first_fused(x, "f64")
    assert not torch.equal(a, b)
    assert float((a - b).abs().max()) <= 9 * 2.0 ** -11 * float(plain.w["down1", 0].abs().max()) * float(x.abs().max()) * 1.01
