"""The three-stage F(4x4,3x3) form of the deep fp32 3x3 layers (csrc/wino3s_kernels.hip + conv_dma<..., WINO_GEMM>): input transform,
36 split-bf16 GEMMs, output transform, with V and M in the unused part of the workspace's ping-pong buffers.

ADN_WINO_GEMM=2 forces the form wherever its buffers fit (FORCED below also pins the other layers, so that a clip's result does not
depend on its batch); ADN_WINO_GEMM=0 is the library without it (OFF: pinned F(4x4,3x3) / F(2x2,3x3) in one launch per layer, the
kernels the goldens have been checked against since round 2).  Bounds are the project's own: 1e-4 of max|y| against the reference's
goldens and the oracle, 2e-5 between two kernel choices (tests/test_gpu_shapes.py::test_automatic_and_pinned_kernel_choice_agree).
At 16x16 the buffers do not fit beside the tensors (V of one tile x 1024 channels is 147 KB, a ping-pong buffer 65 KB per clip): the
layers stay on their one-launch kernels, which is what choose_conv3 promises there.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import VARIANT_KINDS, load_variant_golden, variant_input

pytestmark = pytest.mark.gpu

TOL = 1e-4
AGREE = 2e-5
ENV_KEYS = ("ADN_BATCH_INVARIANT", "ADN_WINO_TILE", "ADN_CONV_ALGO", "ADN_WINO_SPLITK", "ADN_CONVT_SPLIT", "ADN_WINO_GEMM",
            "ADN_AUTO_GRID", "ADN_AUTO_GRID64")
FORCED = {"ADN_WINO_GEMM": "2", "ADN_BATCH_INVARIANT": "1"}
OFF = {"ADN_WINO_GEMM": "0", "ADN_BATCH_INVARIANT": "1"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _net(sd, dev, env, in_ch=1, classes=1):
    """A network whose handle is created under `env` (the switches are read once, when the handle is created)."""
    from audiodenoiser_amd.model import UNet
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    try:
        m = UNet(in_ch, classes)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).eval()
        with torch.no_grad():
            m(torch.zeros((1, in_ch, 16, 16), device=dev))
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return m


@pytest.fixture(scope="module")
def forced(weights_np, dev):
    return _net(weights_np, dev, FORCED)


@pytest.fixture(scope="module")
def off(weights_np, dev):
    return _net(weights_np, dev, OFF)


def _rel(a, ref):
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def _check_golden(m, g, x, tol, label):
    with torch.no_grad():
        y, taps = m(x, return_taps=True)
        y_plain = m(x)
    worst = 0.0
    for clip in range(x.shape[0]):                             # per clip: a x100 clip must not mask the x1 clip
        for got in (y[clip], y_plain[clip]):
            e = _rel(got.cpu().numpy(), g["y"][clip])
            worst = max(worst, e)
            assert e <= tol, (label, clip, e)
    for name, tp in taps.items():
        a = tp.cpu().numpy().astype(np.float64).ravel()
        s_, sa, sq, cnt = g[f"{name}_stats"]
        assert a.size == int(cnt), name
        assert np.abs(a[g[f"{name}_idx"]] - g[f"{name}_val"]).max() <= 10 * tol * np.sqrt(sq / cnt), (label, name)
        assert abs(np.abs(a).sum() - sa) <= tol * sa, (label, name)
    print(f"three-stage forced, {label}: worst output error {worst:.2e} of max|y| (bound {tol:g})")


@pytest.mark.parametrize("n,f,t", [(2, 33, 47), (1, 257, 188)])
def test_forced_matches_reference_goldens_benign(forced, off, dev, golden_dir, n, f, t):
    """33x47: 4x5 and 2x2 pixel images at the two deepest levels -- partial tiles in both directions, two / one GEMM rows per clip,
    a transposed-convolution output smaller than its skip (pad offset of the virtual concat)."""
    from audiodenoiser_amd.weights import make_input
    g = np.load(os.path.join(golden_dir, f"unet_{f}x{t}.npz"))
    x = torch.from_numpy(make_input(7, n, f, t)).to(dev)
    _check_golden(forced, g, x, TOL, f"benign {f}x{t}")
    with torch.no_grad():
        assert not torch.equal(forced(x), off(x))             # the form did run (its sums differ in the last bits)


@pytest.mark.parametrize("kind", VARIANT_KINDS)
def test_forced_matches_reference_goldens_under_weight_variants(dev, golden_dir, variant_weights, kind):
    """"trained" and "heavy" weight sets, inputs at scale 1 (clip 0) and 100 (clip 1), 33x47 and 257x188, every block tap."""
    m = _net(variant_weights(kind), dev, FORCED)
    for f, t in ((33, 47), (257, 188)):
        g = load_variant_golden(golden_dir, kind, f, t)
        x = torch.from_numpy(variant_input(golden_dir, f, t)).to(dev)
        _check_golden(m, g, x, TOL, f"{kind} {f}x{t}")


def test_forced_two_input_planes_three_classes(dev, golden_dir):
    from audiodenoiser_amd.weights import make_input, make_state_dict
    g = np.load(os.path.join(golden_dir, "unet_c2k3_33x47.npz"))
    m = _net(make_state_dict(1234, 2, 3), dev, FORCED, 2, 3)
    x = torch.from_numpy(make_input(7, 4, 33, 47).reshape(2, 2, 33, 47)).to(dev)
    with torch.no_grad():
        y, taps = m(x, return_taps=True)
    assert _rel(y.cpu().numpy(), g["y"]) <= TOL
    for name, tp in taps.items():
        a = tp.cpu().numpy().astype(np.float64).ravel()
        s_, sa, sq, cnt = g[f"{name}_stats"]
        assert np.abs(a[g[f"{name}_idx"]] - g[f"{name}_val"]).max() <= 10 * TOL * np.sqrt(sq / cnt), name


@pytest.mark.parametrize("n,f,t", [(1, 16, 16), (3, 16, 16), (3, 40, 33)])
def test_forced_matches_oracle_all_blocks(forced, dev, weights_np, n, f, t):
    """16x16: the deepest level is one pixel (the buffers do not fit: one-launch kernels); 40x33 with three clips: 5x4 and 2x2
    pixel images, every block output against the oracle."""
    import oracle
    from audiodenoiser_amd.weights import make_input
    x = make_input(21, n, f, t)
    ref, rtaps = oracle.unet_forward(weights_np, x, acc64=True, want_taps=True)
    with torch.no_grad():
        y, taps = forced(torch.from_numpy(x).to(dev), return_taps=True)
    for name in oracle.TAP_NAMES:
        assert _rel(taps[name].cpu().numpy(), rtaps[name]) <= TOL, name
    assert _rel(y.cpu().numpy(), ref) <= TOL


AGREE_SHAPES = ((2, 33, 47), (1, 16, 16), (3, 16, 16), (3, 40, 33), (1, 257, 188), (64, 257, 188))


def test_forced_and_default_agree_with_the_one_launch_kernels(forced, off, dev, weights_np):
    """Forced against the pinned one-launch kernels (ADN_WINO_GEMM=0) to the last bits of fp32, and the default handle at
    64 x 257x188, where the automatic choice takes the form (GEMM grids of 3456 and 1728 workgroups at levels 3 and 4)."""
    from audiodenoiser_amd.weights import make_input
    auto = _net(weights_np, dev, {})
    worst = 0.0
    for n, f, t in AGREE_SHAPES:
        x = torch.from_numpy(make_input(300 + f, n, f, t)).to(dev)
        with torch.no_grad():
            yf, yo = forced(x), off(x)
            err = float((yf - yo).abs().max() / yo.abs().max())
            print(f"three-stage forced vs one-launch kernels, {n} x {f}x{t}: {err:.2e} of max|y| (bound {AGREE:g})")
            worst = max(worst, err)
            assert bool(torch.isfinite(yf).all()) and err <= AGREE, (n, f, t, err)
            if n == 64:
                ya = auto(x)
                erra = float((ya - yo).abs().max() / yo.abs().max())
                print(f"default handle vs one-launch kernels, {n} x {f}x{t}: {erra:.2e} of max|y|")
                assert erra <= AGREE and not torch.equal(ya, yo)
                assert torch.equal(ya, yf)                   # at this size the default runs the kernels of the pinned handle
    print(f"three-stage forced vs one-launch kernels: worst {worst:.2e} of max|y|")


def test_forced_is_bit_identical_across_batches_and_calls(forced, dev):
    """64x48: 8x6 and 4x3 pixel images, 4 GEMM rows per clip at level 3 -- in a batch of 64 the rows of clips 31 and 32 lie on either
    side of the boundary between two 128-row GEMM tiles.  GEMM rows do not mix: a clip alone, in batches of 2, 5 and 64."""
    from audiodenoiser_amd.weights import make_input
    x = torch.from_numpy(make_input(11, 64, 64, 48)).to(dev)
    with torch.no_grad():
        y = forced(x).clone()
        assert torch.equal(forced(x), y)
        for i in (0, 31, 32, 63):
            assert torch.equal(forced(x[i:i + 1].clone())[0], y[i]), i
        assert torch.equal(forced(x[31:33].clone()), y[31:33])
        assert torch.equal(forced(x[30:35].clone()), y[30:35])


def test_forced_nonfinite_pixels_travel_as_in_the_reference(forced, dev, golden_dir):
    """unet_nonfinite_257x188.npz = the reference's forward of one +inf / one NaN pixel: the non-finite set holds the reference's and
    exceeds it by at most the F(4x4,3x3) allowance (3 pixels per layer at the layer's resolution, 92 level-0 pixels each: DESIGN.md
    section 2; the three-stage form poisons exactly the tiles whose 6x6 patch holds a poisoned pixel, as wino4_conv_f32 does)."""
    from test_gpu_variants import _check_nonfinite
    g = np.load(os.path.join(golden_dir, "unet_nonfinite_257x188.npz"))
    for kind in ("inf", "nan"):
        compared, room = _check_nonfinite(forced, g, 257, 188, kind, 3, TOL, dev, "wino_gemm_forced")
        assert compared >= room and compared > 0


def test_forced_poisoned_clip_leaves_its_neighbours_alone(forced, dev):
    from audiodenoiser_amd.weights import make_input
    clean = torch.from_numpy(make_input(7, 4, 257, 188)).to(dev)
    with torch.no_grad():
        y0 = forced(clean).clone()
        bad = clean.clone()
        bad[1, 0, 20, 20] = float("inf")
        bad[2, 0, 200, 100] = float("nan")
        yb = forced(bad).clone()
        y1 = forced(clean)
    assert bool(torch.isfinite(y0).all()) and torch.equal(y0, y1)        # nothing sticks in V or M
    assert torch.equal(yb[0], y0[0]) and torch.equal(yb[3], y0[3])
    assert not bool(torch.isfinite(yb[1]).all()) and not bool(torch.isfinite(yb[2]).all())


def _bt():
    return np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                     [0, 4, 0, -5, 0, 1]], dtype=np.float64)


def _vmax(t):
    """max |B^T d B| over the 4x4-output tiles of a (C, H, W) tensor with a zero border (float64)."""
    c, h, w = t.shape
    ty, tx = (h + 3) // 4, (w + 3) // 4
    p = np.zeros((c, 4 * ty + 2, 4 * tx + 2))
    p[:, 1:h + 1, 1:w + 1] = t
    bt, best = _bt(), 0.0
    for i in range(ty):
        for j in range(tx):
            v = np.einsum("ai,cij,bj->cab", bt, p[:, 4 * i:4 * i + 6, 4 * j:4 * j + 6], bt)
            best = max(best, float(np.abs(v).max()))
    return best


def test_forced_finite_operand_near_flt_max_in_the_transform_domain(dev, weights_np):
    """A FINITE transform-domain value in the top 0.2 % of fp32's range (>= 3.3961e38, where bf16 round-to-nearest would make the
    leading term of the split infinite) must split exactly: finite in, finite out, and the same results as the exact-fp32 kernels.
    down4's output is made 1000x everything before it; it feeds up1's first conv (skip) and, pooled, the bottleneck's first conv, both
    on the three-stage form: the larger of their two largest |V| is steered into the window, and both layers scale their sums
    back into range (BatchNorm factor 1e-9), as does the transposed convolution between them."""
    from audiodenoiser_amd.weights import make_input
    sd = {k: np.array(v, copy=True) for k, v in weights_np.items()}
    sd["downconv4.conv.double_conv.4.weight"] *= np.float32(1e3)
    for key in ("bottleneck.double_conv.1", "upconv1.conv.double_conv.1"):
        sd[key + ".weight"] *= np.float32(1e-9)
    assert "downconv4.conv.double_conv.4.weight" in weights_np and "upconv1.conv.double_conv.1.weight" in weights_np
    three, exact = _net(sd, dev, FORCED), _net(sd, dev, OFF)
    x0 = torch.from_numpy(make_input(7, 1, 33, 47)).to(dev)

    def vmax_of(taps):
        d4 = taps["down4"][0].double().cpu().numpy()
        pooled = d4[:, :d4.shape[1] // 2 * 2, :d4.shape[2] // 2 * 2].reshape(d4.shape[0], d4.shape[1] // 2, 2, d4.shape[2] // 2, 2).max(axis=(2, 4))
        return max(_vmax(d4), _vmax(pooled))
    with torch.no_grad():
        # a ReLU network is positively homogeneous once the biases are negligible: probe at 1e28, then scale into the window
        v1 = vmax_of(exact(x0 * 1e28, return_taps=True)[1])
        assert np.isfinite(v1) and v1 > 1e28
        x = x0 * (1e28 * (3.3995e38 / v1))
        ye, te = exact(x, return_taps=True)
        yt, tt = three(x, return_taps=True)
    top = vmax_of(tt)                                          # what the three-stage layers transform (down4 is their own output)
    print(f"largest transform-domain value: {top:.5e}")
    assert 3.3961e38 <= top <= 3.4028e38, top
    assert bool(torch.isfinite(tt["down4"]).all()) and torch.equal(te["down3"], tt["down3"])     # same kernels up to level 3
    for name in ("down4", "bottleneck", "up1", "out"):
        a, b = te[name], tt[name]
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        assert float((a - b).abs().max()) <= AGREE * float(a.abs().max()), name
    assert bool(torch.isfinite(yt).all())


@pytest.mark.parametrize("n,f,t", [(1, 33, 47), (3, 33, 47), (64, 33, 47), (8, 257, 188)])
def test_forced_runs_in_exactly_the_workspace(forced, off, dev, n, f, t):
    """The forward runs in adn_unet_workspace_bytes bytes: a patterned guard behind them is untouched, and every block output --
    the skips, the tensors the deep layers read and write -- agrees with the one-launch kernels, i.e. V and M overlapped
    no live tensor on their way through the ping-pong buffers."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.weights import make_input
    x = torch.from_numpy(make_input(5, n, f, t)).to(dev)
    need = ctypes.c_size_t()
    _lib.check(_lib.load().adn_unet_workspace_bytes(forced._handle, n, f, t, ctypes.byref(need)), "adn_unet_workspace_bytes")
    guard = 1 << 20
    buf = torch.full((need.value + guard,), 0xA5, dtype=torch.uint8, device=dev)
    kept = forced._workspace
    forced._workspace = buf[:need.value]
    try:
        with torch.no_grad():
            y, taps = forced(x, return_taps=True)
            y_plain = forced(x)
        torch.cuda.synchronize()
        assert forced._workspace.data_ptr() == buf.data_ptr()
    finally:
        forced._workspace = kept
    assert bool((buf[need.value:] == 0xA5).all())
    with torch.no_grad():
        yo, to = off(x, return_taps=True)
    for name in taps:
        assert float((taps[name] - to[name]).abs().max()) <= TOL * float(to[name].abs().max()), name
    assert float((y_plain - yo).abs().max()) <= AGREE * float(yo.abs().max())


def test_forced_forward_is_graph_capturable(forced, dev):
    x = torch.rand((2, 1, 64, 48), device=dev) * 3
    with torch.no_grad():
        forced(x)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            forced(x)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = forced(x)
        x.copy_(torch.rand((2, 1, 64, 48), device=dev) * 3)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, forced(x))
