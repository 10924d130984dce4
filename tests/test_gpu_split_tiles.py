"""Workgroup tiles of the split-bf16 GEMMs -- the GEMM stage of the three-stage F(4x4,3x3) form and the fp32 transposed convolutions
(conv_dma<float, 8, BN, ..., WINO_GEMM | CONVT2X2, ..., SPLIT>): 128 rows x 128 columns, x 256 columns on 4 waves, x 256 columns on
8 waves (ADN_SPLIT_BN = 128 | 256 | 256w8, read when the handle is created; adn::SplitTile).

The tile decides which wave holds an accumulator and nothing else: every output element sees the same 16-channel chunks in the
same order and the same six products per chunk in the same order.  So the bound between widths is EQUALITY of the bits, on the
output and on every block tap, and non-finite values included.  U is packed per column tile: a handle whose planes and kernel
disagreed about the width would not get one tensor right.  Handles as in tests/test_gpu_wino3s.py: ADN_WINO_GEMM=2 +
ADN_BATCH_INVARIANT=1 put all five layers on the form whatever the batch.

Shapes: 2 x 33x47 (level 3: 4x5 pixels, level 4: 2x2 -- 8 and 2 GEMM rows, one partial row tile); 3 x 40x33; 5 x 257x188 (level 3:
32x23 pixels = 240 rows, a full and a partial row tile; level 4: 16x11 = 60 rows; the transposed convolutions read 16x11 and 32x23
images, partial in both directions, and their outputs are padded by an odd amount).
"""
import os

import numpy as np
import pytest
import torch

import footprint as fp
from conftest import load_variant_golden, variant_input
from test_gpu_footprint import _forward_in, _need, _same_bits
from test_gpu_wino3s import ENV_KEYS as WINO_ENV_KEYS, FORCED, TOL, _check_golden

pytestmark = pytest.mark.gpu

ENV_KEYS = WINO_ENV_KEYS + ("ADN_SPLIT_BN",)
WIDE = ("256", "256w8")
SHAPES = ((2, 33, 47), (3, 40, 33), (5, 257, 188))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _net(sd, dev, env):
    """A network whose handle is created under `env` alone (the switches are read once, when the handle is created)."""
    from audiodenoiser_amd.model import UNet
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    try:
        m = UNet(1, 1)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).eval()
        with torch.no_grad():
            m(torch.zeros((1, 1, 16, 16), device=dev))
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return m


@pytest.fixture(scope="module")
def nets(weights_np, dev):
    """width ("128", "256", "256w8", or "default": the library's own table, switches unset) -> forced handle; one each for the file."""
    cache = {}

    def get(width):
        if width not in cache:
            cache[width] = _net(weights_np, dev, dict(FORCED) if width == "default" else dict(FORCED, ADN_SPLIT_BN=width))
        return cache[width]
    return get


@pytest.fixture(scope="module")
def narrow_results(nets, dev):
    """(shape, poison) -> (y, taps) of the 128-column handle: computed once, shared by both wide forms, never written."""
    cache = {}

    def get(shape, poison):
        if (shape, poison) not in cache:
            with torch.no_grad():
                y, taps = nets("128")(_input(shape, poison, dev), return_taps=True)
            cache[(shape, poison)] = (y.clone(), {k: v.clone() for k, v in taps.items()})
        return cache[(shape, poison)]
    return get


def _input(shape, poison, dev):
    from audiodenoiser_amd.weights import make_input
    n, f, t = shape
    x = torch.from_numpy(make_input(500 + f, n, f, t)).to(dev)
    if poison:                                               # one +inf pixel (first clip), one NaN pixel (last clip)
        x[0, 0, f // 3, t // 2] = float("inf")
        x[n - 1, 0, f - 2, 1] = float("nan")
    return x


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("width", WIDE)
def test_wide_tiles_give_the_bits_of_the_128_column_tile(nets, narrow_results, dev, width, shape):
    y0, taps0 = narrow_results(shape, False)
    with torch.no_grad():
        y, taps = nets(width)(_input(shape, False, dev), return_taps=True)
    assert bool(torch.isfinite(y0).all())
    assert set(taps) == set(taps0) and len(taps) == 10
    for name in taps0:
        assert torch.equal(taps[name], taps0[name]), (width, shape, name)
    assert torch.equal(y, y0), (width, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("width", WIDE)
def test_wide_tiles_carry_non_finite_pixels_bit_for_bit(nets, narrow_results, dev, width, shape):
    """One +inf and one NaN pixel: the NaN positions are the same and every word is the same (_same_bits: a NaN equals the same NaN)."""
    y0, taps0 = narrow_results(shape, True)
    with torch.no_grad():
        y, taps = nets(width)(_input(shape, True, dev), return_taps=True)
    assert not bool(torch.isfinite(y0[0]).all()) and not bool(torch.isfinite(y0[-1]).all())      # the pixels did travel
    for name in taps0:
        assert torch.equal(torch.isnan(taps[name]), torch.isnan(taps0[name])), (width, shape, name)
        assert _same_bits(taps[name], taps0[name]), (width, shape, name)
    assert torch.equal(torch.isnan(y), torch.isnan(y0)) and _same_bits(y, y0), (width, shape)


def test_default_handle_stays_within_the_bound_of_the_reference_goldens(nets, dev, golden_dir, variant_weights):
    """The library's own choice of tiles against the goldens tests/test_gpu_wino3s.py loads: benign weights and the "trained" set,
    33x47 and 257x188, the project's 1e-4 of max|y|, every block tap."""
    from audiodenoiser_amd.weights import make_input
    for n, f, t in ((2, 33, 47), (1, 257, 188)):
        g = np.load(os.path.join(golden_dir, f"unet_{f}x{t}.npz"))
        _check_golden(nets("default"), g, torch.from_numpy(make_input(7, n, f, t)).to(dev), TOL, f"default tiles, benign {f}x{t}")
    m = _net(variant_weights("trained"), dev, FORCED)
    for f, t in ((33, 47), (257, 188)):
        g = load_variant_golden(golden_dir, "trained", f, t)
        _check_golden(m, g, torch.from_numpy(variant_input(golden_dir, f, t)).to(dev), TOL, f"default tiles, trained {f}x{t}")


@pytest.mark.parametrize("width", WIDE)
def test_wide_tiles_write_inside_the_workspace_and_read_nothing_stale(nets, narrow_results, dev, width):
    """5 x 257x188 in exactly adn_unet_workspace_bytes bytes between two guards, the workspace handed over as zeros and as 0xFF
    bytes (NaN), outputs carved too (tests/footprint.py): a 256-column epilogue that stored past the last GEMM row or past M, or
    staged a row it never computed, changes a guard, a tap, or makes the result depend on the fill."""
    shape = SHAPES[2]
    m, x = nets(width), _input(shape, False, dev)
    need = _need(m, *shape)
    runs = []
    for fill in (0x00, 0xFF):
        ws, hws = fp.carve(need, fill, dev)
        got, handles = _forward_in(m, x, ws, True, dev)
        fp.assert_guards_intact(hws, f"{width}: workspace of {need} bytes (fill {fill:#04x})")
        for name, h in handles.items():
            fp.assert_guards_intact(h, f"{width}: {name} (fill {fill:#04x})")
        runs.append(got)
        del ws, hws
    y0, taps0 = narrow_results(shape, False)
    for name in runs[0]:
        assert _same_bits(runs[0][name], runs[1][name]), f"{width}: {name} depends on what the workspace held"
        assert _same_bits(runs[0][name], y0 if name == "y" else taps0[name]), f"{width}: {name} differs from the 128-column tile"


def test_default_tiles_pinned_and_unpinned_agree_at_batch_64(weights_np, nets, dev):
    """64 x 257x188: the automatic choice takes the form at both levels (GEMM grids of 3456 and 1728 128-column workgroups: the
    threshold does not move with the tile), so the default handle runs the kernels of the pinned one -- the same bits, as
    tests/test_gpu_wino3s.py expects -- and those are the bits of the 128-column tile."""
    from audiodenoiser_amd.weights import make_input
    x = torch.from_numpy(make_input(300 + 257, 64, 257, 188)).to(dev)
    auto = _net(weights_np, dev, {})
    with torch.no_grad():
        ya = auto(x).clone()
        assert torch.equal(ya, nets("default")(x))
        assert torch.equal(ya, nets("128")(x))


@pytest.mark.parametrize("width", WIDE)
def test_unpinned_handles_agree_where_the_transposed_convolutions_are_cut_along_k(weights_np, dev, width):
    """Automatic kernel choice: one clip of 257x188 has its transposed convolutions cut along K, and those slices stay on the
    128-column planes whatever tile the layer has (it keeps both packings); 5 clips run the wide tile unsplit.  Same bits."""
    from audiodenoiser_amd.weights import make_input
    wide, narrow = _net(weights_np, dev, {"ADN_SPLIT_BN": width}), _net(weights_np, dev, {"ADN_SPLIT_BN": "128"})
    for n in (1, 5):
        x = torch.from_numpy(make_input(40 + n, n, 257, 188)).to(dev)
        with torch.no_grad():
            yw, tw = wide(x, return_taps=True)
            yn, tn = narrow(x, return_taps=True)
        for name in tn:
            assert torch.equal(tw[name], tn[name]), (width, n, name)
        assert torch.equal(yw, yn) and bool(torch.isfinite(yn).all()), (width, n)


def test_an_unknown_width_is_refused_when_the_handle_is_created(weights_np, dev):
    from audiodenoiser_amd._lib import AdnError
    with pytest.raises(AdnError, match="ADN_SPLIT_BN"):
        _net(weights_np, dev, dict(FORCED, ADN_SPLIT_BN="192"))
