"""Where the entry points that take a caller's workspace write, and what they read back (tests/footprint.py).

Value parity is pinned elsewhere (goldens, float64 restatements, weight variants, non-finite cases).  Here every buffer a call
touches -- workspace, x, y, every block output, losses, gradients, audio -- sits between patterned guards, the workspace is handed
over holding zeros and then 0xFF bytes (NaN in fp32 and in fp16), and the results are compared bit for bit:

  * no byte outside `*_workspace_bytes` and the outputs is written (front and back guards of every buffer);
  * inputs are unchanged;
  * the result does not depend on what the workspace held (zeros against NaN), nor on the run (NaN against NaN: the forward has no
    atomics and its reduce launches add in a fixed order);
  * one byte less of workspace is refused and nothing is written.

No tolerance appears in the footprint checks: every comparison is bit equality.  The first-layer edge cases and the three iSTFT sizes
no other test runs are compared with their oracles at the tree's own bounds (1e-4 / 1e-2 of max|y|, tests/test_gpu_shapes.py; 1e-4,
tests/test_gpu_parity.py) in addition.

U-Net shapes (N, F, T): each is the smallest that crosses a decision of choose_conv3, choose_convt or make_plan (csrc/unet.hip) --
one-pixel bottleneck where the three-stage buffers do not fit (1,16,16); images 16 wide at level 0, pair mode, odd rows (1,33,47),
(2,31,16); pair mode with an odd clip count on a tall image (3,1025,16); the shapes of test_automatic_and_pinned_kernel_choice_agree
where the small-grid rules switch kernels and split counts; one production clip (1,513,256), where every split rule fires.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import footprint as fp
from test_gpu_wino3s import ENV_KEYS as WINO_ENV_KEYS

pytestmark = pytest.mark.gpu

ENV_KEYS = WINO_ENV_KEYS + ("ADN_F16_FIRST", "ADN_F16_CONV", "ADN_F16_CONVT")
ADN_ERR_WORKSPACE = 3
TAP_NAMES = ("down1", "down2", "down3", "down4", "bottleneck", "up1", "up2", "up3", "up4", "out")

MODES = {
    "f32": {"auto": {}, "batch_invariant": {"ADN_BATCH_INVARIANT": "1"}, "splitk": {"ADN_WINO_SPLITK": "1"},
            "tile2": {"ADN_WINO_TILE": "2"}, "tile4": {"ADN_WINO_TILE": "4"}, "direct": {"ADN_CONV_ALGO": "direct"},
            "convt_exact": {"ADN_CONVT_SPLIT": "0"}, "wino_gemm0": {"ADN_WINO_GEMM": "0"}, "wino_gemm2": {"ADN_WINO_GEMM": "2"}},
    "f16": {"auto": {}, "batch_invariant": {"ADN_BATCH_INVARIANT": "1"}, "first0": {"ADN_F16_FIRST": "0"},
            "conv32": {"ADN_F16_CONV": "32"}, "convt_dma": {"ADN_F16_CONVT": "dma"}},
}
SHAPES = [(1, 16, 16), (1, 33, 47), (2, 31, 16), (3, 1025, 16), (1, 16, 130), (3, 129, 65), (2, 64, 80), (1, 257, 188), (5, 257, 188),
          (16, 256, 64), (7, 48, 1040), (1, 40, 2000), (1, 513, 256)]
SUBSET = [(1, 16, 16), (2, 31, 16), (1, 33, 47), (3, 129, 65), (1, 257, 188)]
UNET_CASES = [(dtype, mode, shape) for dtype in ("f32", "f16") for mode in MODES[dtype] for shape in (SHAPES if mode == "auto" else SUBSET)]


def _shape_id(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nets(weights_np, dev):
    """(dtype, mode, in_channels, classes) -> a network whose handle was created under the mode's switches (they are read once, when
    the handle is created), as tests/test_gpu_wino3s.py::_net does; one handle per key for the whole file."""
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.weights import make_state_dict
    cache = {}

    def get(dtype, mode="auto", in_ch=1, classes=1):
        key = (dtype, mode, in_ch, classes)
        if key in cache:
            return cache[key]
        sd = weights_np if (in_ch, classes) == (1, 1) else make_state_dict(1234, in_ch, classes)
        saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
        os.environ.update(MODES[dtype][mode])
        try:
            m = UNet(in_ch, classes)
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
            m = m.to(dev).eval().set_compute_dtype(dtype)
            with torch.no_grad():
                m(torch.zeros((1, in_ch, 16, 16), device=dev))
        finally:
            for k in ENV_KEYS:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
        cache[key] = m
        return m
    return get


def _same_bits(a, b):
    """Bit for bit (torch.equal on the words: a NaN equals the same NaN, -0.0 is not +0.0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _need(m, n, f, t):
    from audiodenoiser_amd import _lib
    need = ctypes.c_size_t()
    _lib.check(_lib.load().adn_unet_workspace_bytes(m._handle, n, f, t, ctypes.byref(need)), "adn_unet_workspace_bytes")
    return need.value


def _forward_in(m, x, ws, taps, dev):
    """m(x) with `ws` as the module's workspace and y (and the ten block outputs) carved; returns (tensors by name, their handles)."""
    kept = m._workspace
    m._workspace = ws
    try:
        with torch.no_grad(), fp.carved_outputs(dev) as made:
            out = m(x, return_taps=taps)
        torch.cuda.synchronize()
        assert m._workspace.data_ptr() == ws.data_ptr() and m._workspace.numel() == ws.numel()     # the library got this view
    finally:
        m._workspace = kept
    got = {"y": out[0], **out[1]} if taps else {"y": out}
    assert len(made) == len(got) and all(h.view.data_ptr() == t.data_ptr() for h, t in zip(made, got.values()))
    return got, dict(zip(got, made))


def _check_forward_footprint(m, x_host, taps, dev, label):
    """Steps 1-6 of a U-Net case; returns y of the zero-filled run."""
    n, _, f, t = x_host.shape
    need = _need(m, n, f, t)
    x, hx = fp.carve_copy(x_host, dev)
    x_before = x.clone()
    runs = []
    for k, fill in enumerate((0x00, 0xFF, 0xFF)):
        ws, hws = fp.carve(need, fill, dev)
        got, handles = _forward_in(m, x, ws, taps, dev)
        fp.assert_guards_intact(hws, f"{label}: workspace of {need} bytes, run {k} (fill {fill:#04x})")
        for name, h in handles.items():
            fp.assert_guards_intact(h, f"{label}: {name}, run {k}")
        fp.assert_guards_intact(hx, f"{label}: x, run {k}")
        assert torch.equal(x, x_before), (label, "x was written", k)
        runs.append(got)
        del ws, hws
    for name in runs[0]:
        assert _same_bits(runs[1][name], runs[2][name]), f"{label}: {name} differs between two runs on a NaN-filled workspace (not deterministic)"
        assert _same_bits(runs[0][name], runs[1][name]), f"{label}: {name} depends on what the workspace held (zeros against 0xFF bytes)"
    assert bool(torch.isfinite(runs[0]["y"]).all()), label
    with torch.no_grad():
        plain = m(x, return_taps=taps)                   # the module's ordinary call, its own workspace
    plain = {"y": plain[0], **plain[1]} if taps else {"y": plain}
    for name in plain:
        assert _same_bits(plain[name], runs[0][name]), f"{label}: {name} differs from the module's ordinary call"
    return runs[0]["y"]


# ---- the helper itself ---------------------------------------------------------------------------------------------------------

def test_helper_reports_a_write_into_either_guard_with_sign_and_offset(dev):
    view, h = fp.carve(1000, 0x00, dev, guard=4096)
    fp.assert_guards_intact(h, "untouched")
    assert fp.first_guard_hit(h) is None and view.numel() == 1000 and fp.keeps_fill(h, 0x00)
    h.buf[4096 - 7] = 1                                  # 7 bytes in front of the owned region
    assert fp.first_guard_hit(h) == (-7, 1)
    with pytest.raises(AssertionError, match=r"offset -7 .*7 bytes in front"):
        fp.assert_guards_intact(h, "front")
    h.buf[4096 - 7] = fp.PATTERN
    h.buf[4096 + 1000] = 2                               # the first byte behind it
    h.buf[4096 + 1000 + 40] = 3
    assert fp.first_guard_hit(h) == (1, 2)
    with pytest.raises(AssertionError, match=r"offset \+1 .*1 bytes behind"):
        fp.assert_guards_intact(h, "back")
    h.buf[4096 + 1000] = fp.PATTERN
    assert fp.first_guard_hit(h) == (41, 3)
    view[999] = 9                                        # the last owned byte is the caller's
    h.buf[4096 + 1000 + 40] = fp.PATTERN
    fp.assert_guards_intact(h, "owned")
    assert not fp.keeps_fill(h, 0x00)
    t, ht = fp.carve_tensor((3, 5), 0xFF, dev)
    assert t.shape == (3, 5) and t.dtype == torch.float32 and bool(torch.isnan(t).all()) and ht.guard == 4 * fp.FLOAT_GUARD
    assert bool(torch.isnan(fp.carve(64, 0xFF, dev, dtype=torch.float16)[0]).all())


def test_helper_view_is_the_pointer_the_library_receives(nets, dev):
    m = nets("f32")
    need = _need(m, 1, 16, 16)
    ws, h = fp.carve(need, 0x00, dev)
    assert ws.data_ptr() == h.buf.data_ptr() + fp.WS_GUARD and ws.data_ptr() % 16 == 0 and ws.numel() == need
    got, handles = _forward_in(m, torch.ones((1, 1, 16, 16), device=dev), ws, False, dev)          # asserts m._workspace.data_ptr()
    assert got["y"].data_ptr() == handles["y"].buf.data_ptr() + 4 * fp.FLOAT_GUARD
    assert bool((h.owned_bytes() != 0).any())            # and the forward did write through it


# ---- U-Net forward -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("taps", [False, True], ids=["plain", "taps"])
@pytest.mark.parametrize("dtype,mode,shape", UNET_CASES, ids=[f"{d}-{m}-{_shape_id(s)}" for d, m, s in UNET_CASES])
def test_unet_forward_footprint(nets, dev, dtype, mode, shape, taps):
    from audiodenoiser_amd.weights import make_input
    n, f, t = shape
    x = torch.from_numpy(make_input(300 + f, n, f, t))
    _check_forward_footprint(nets(dtype, mode), x, taps, dev, f"{dtype} {mode} {n} x {f}x{t} {'taps' if taps else 'plain'}")


def test_unet_small_forward_in_the_leading_bytes_of_a_used_workspace(nets, dev):
    """(1,33,47) in exactly its `need` bytes, which are the leading bytes of the workspace a (5,257,188) forward of the same handle
    has just used, not refilled: bit-identical to the run in a zero-filled workspace."""
    from audiodenoiser_amd.weights import make_input
    m = nets("f32")
    big = torch.from_numpy(make_input(300 + 257, 5, 257, 188)).to(dev)
    small = torch.from_numpy(make_input(300 + 33, 1, 33, 47)).to(dev)
    need_big, need = _need(m, 5, 257, 188), _need(m, 1, 33, 47)
    assert need < need_big
    zero, hzero = fp.carve(need, 0x00, dev)
    ref = _forward_in(m, small, zero, False, dev)[0]["y"]
    ws, hws = fp.carve(need_big, 0xFF, dev)
    _forward_in(m, big, ws, False, dev)
    used = ws[:need].clone()
    got, handles = _forward_in(m, small, ws[:need], False, dev)
    assert not torch.equal(used, ws[:need])              # (the small forward did run in those bytes)
    assert torch.equal(got["y"], ref)
    fp.assert_guards_intact(hws, "workspace of the large forward")
    fp.assert_guards_intact(hzero, "zero-filled workspace")
    fp.assert_guards_intact(handles["y"], "y")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_unet_forward_refuses_one_byte_less(nets, dev, dtype):
    from audiodenoiser_amd import _lib
    L = _lib.load()
    m = nets(dtype)
    for n, f, t in ((1, 33, 47), (1, 257, 188)):
        need = _need(m, n, f, t)
        x = torch.rand((n, 1, f, t), device=dev)
        ws, hws = fp.carve(need, 0xFF, dev)
        y, hy = fp.carve_tensor((n, 1, f, t), 0xFF, dev)
        taps = [fp.carve_tensor((1,), 0xFF, dev) for _ in TAP_NAMES]
        arr = (ctypes.c_void_p * 10)(*[tp.data_ptr() for tp, _ in taps])
        assert L.adn_unet_forward(m._handle, x.data_ptr(), y.data_ptr(), n, f, t, ws.data_ptr(), need - 1, None) == ADN_ERR_WORKSPACE
        assert b"workspace" in L.adn_last_error()
        assert L.adn_unet_forward_taps(m._handle, x.data_ptr(), y.data_ptr(), n, f, t, ws.data_ptr(), need - 1, arr, None) == ADN_ERR_WORKSPACE
        torch.cuda.synchronize()
        for h in [hws, hy] + [h for _, h in taps]:
            assert fp.keeps_fill(h, 0xFF)
            fp.assert_guards_intact(h, "refused call")


# ---- the first layer as its own launch: column tiles, LDS boundary ---------------------------------------------------------------

_oracle_cache = {}


def _oracle(sd, x, key):
    """The torch oracle's forward, computed once per input and shared."""
    from oracle import unet_torch
    if key not in _oracle_cache:
        _oracle_cache[key] = unet_torch.unet_forward(unet_torch.to_torch_state(sd), x).numpy()
    return _oracle_cache[key]


def _rel(a, ref):
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("dtype,mode,tol", [("f32", "tile4", 1e-4), ("f16", "first0", 1e-2)])
def test_first_layer_long_clip_column_tiles(nets, dev, weights_np, dtype, mode, tol):
    """1 x 16 x 33000: the first layer as its own launch (F(4x4,3x3) forced / ADN_F16_FIRST=0), cut into column tiles of 115 -- 287
    tiles cover the width, a 288th would start at x = 33005."""
    from audiodenoiser_amd.weights import make_input
    x = torch.from_numpy(make_input(11, 1, 16, 33000))
    ref = _oracle(weights_np, x, ("1x1", 16, 33000))
    for taps in (False, True):
        y = _check_forward_footprint(nets(dtype, mode), x, taps, dev, f"{dtype} {mode} 1 x 16x33000 {'taps' if taps else 'plain'}")
        e = _rel(y.cpu().numpy(), ref)
        print(f"16x33000 {dtype} {mode}: {e:.2e} of max|y| (bound {tol:g})")
        assert e <= tol, (dtype, mode, taps, e)


# in_channels = 64: 4096 / 64 - 2 = 62 columns per tile, a window of exactly 160 KiB of LDS -- one tile, two tiles with a partial row
# tile, three tiles; in_channels = 33: 4096 / 33 is not exact, 122 columns per tile
PLANES = [(64, (24, 62)), (64, (21, 63)), (64, (24, 130)), (33, (24, 122)), (33, (21, 123)), (33, (24, 300))]


@pytest.mark.parametrize("dtype,tol", [("f32", 1e-4), ("f16", 1e-2)])
@pytest.mark.parametrize("cin,hw", PLANES, ids=[f"cin{c}-{h}x{w}" for c, (h, w) in PLANES])
def test_first_layer_many_input_planes(nets, dev, cin, hw, dtype, tol):
    from audiodenoiser_amd.weights import make_input, make_state_dict
    h, w = hw
    x = torch.from_numpy(make_input(13, cin, h, w).reshape(1, cin, h, w))
    ref = _oracle(make_state_dict(1234, cin, 2), x, (cin, h, w))
    y = _check_forward_footprint(nets(dtype, "auto", cin, 2), x, False, dev, f"UNet({cin},2) {dtype} {h}x{w}")
    e = _rel(y.cpu().numpy(), ref)
    print(f"UNet({cin},2) {h}x{w} {dtype}: {e:.2e} of max|y| (bound {tol:g})")
    assert y.shape == ref.shape and e <= tol, (cin, hw, dtype, e)


# ---- the other entry points that take a caller's workspace ----------------------------------------------------------------------

def _bytes_of(fn, *args):
    from audiodenoiser_amd import _lib
    need = ctypes.c_size_t()
    _lib.check(fn(*args, ctypes.byref(need)), fn.__name__)
    return need.value


def _two_fills(call, need, out_shapes, inputs, dev, label):
    """`call(ws_ptr, ws_bytes, out_ptrs) -> status` with the workspace zero-filled, then 0xFF-filled, outputs carved (0xFF = NaN: an
    element never written shows), inputs watched; then with one byte less.  Returns the outputs (bit-identical across the fills).
    out_shapes: a shape per output pointer, None = pass a null pointer (its absence is all there is to check)."""
    before = [(t, h, t.clone()) for t, h in inputs]
    results = []
    for fill in (0x00, 0xFF):
        ws, hws = fp.carve(need, fill, dev)
        outs = [fp.carve_tensor(s, 0xFF, dev) if s is not None else (None, None) for s in out_shapes]
        rc = call(ws.data_ptr(), need, [o.data_ptr() if o is not None else None for o, _ in outs])
        torch.cuda.synchronize()
        assert rc == 0, (label, rc)
        fp.assert_guards_intact(hws, f"{label}: workspace of {need} bytes (fill {fill:#04x})")
        for k, (o, h) in enumerate(outs):
            if h is not None:
                fp.assert_guards_intact(h, f"{label}: output {k} (fill {fill:#04x})")
        for k, (t, h, was) in enumerate(before):
            fp.assert_guards_intact(h, f"{label}: input {k}")
            assert torch.equal(t, was), (label, "input written", k)
        results.append([o for o, _ in outs])
    for a, b in zip(*results):
        if a is not None:
            assert bool(torch.isfinite(a).all()), f"{label}: an output element is not finite (never written, or computed from the workspace's NaN)"
            assert _same_bits(a, b), f"{label}: the result depends on what the workspace held (zeros against 0xFF bytes)"
    if need > 0:
        ws, hws = fp.carve(need, 0xFF, dev)
        outs = [fp.carve_tensor(s, 0xFF, dev) if s is not None else (None, None) for s in out_shapes]
        rc = call(ws.data_ptr(), need - 1, [o.data_ptr() if o is not None else None for o, _ in outs])
        torch.cuda.synchronize()
        assert rc == ADN_ERR_WORKSPACE, (label, rc)
        for h in [hws] + [h for _, h in outs if h is not None]:
            assert fp.keeps_fill(h, 0xFF), (label, "a refused call wrote")
            fp.assert_guards_intact(h, f"{label}: refused call")
    return results[0]


LOSS_SHAPES = [(2, 16, 63), (1, 33, 64), (3, 40, 96), (2, 24, 6785)]       # (2,24,6785): one frame beyond what the LDS of one CU holds


def _loss_inputs(b, f, t, dev):
    g = torch.Generator().manual_seed(5)
    pred = torch.rand((b, 1, f, t), generator=g) * 3
    tgt = torch.rand((b, 1, f, t), generator=g) * 3
    return fp.carve_copy(pred, dev), fp.carve_copy(tgt, dev)


@pytest.mark.parametrize("b,f,t", LOSS_SHAPES, ids=[_shape_id(s) for s in LOSS_SHAPES])
def test_perceptual_loss_footprint(dev, b, f, t):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.loss import perceptual_loss_per_clip
    L = _lib.load()
    (pred, hp), (tgt, ht) = _loss_inputs(b, f, t, dev)
    need = _bytes_of(L.adn_perceptual_loss_workspace_bytes, b, f, t)
    out, = _two_fills(lambda ws, nb, o: L.adn_perceptual_loss(pred.data_ptr(), tgt.data_ptr(), b, f, t, ws, nb, o[0], None),
                      need, [(b, 4)], [(pred, hp), (tgt, ht)], dev, f"adn_perceptual_loss {b} x {f}x{t}")
    assert torch.equal(out, perceptual_loss_per_clip(pred, tgt))


@pytest.mark.parametrize("which", ["both", "pred", "target"])
@pytest.mark.parametrize("b,f,t", LOSS_SHAPES, ids=[_shape_id(s) for s in LOSS_SHAPES])
def test_perceptual_loss_backward_footprint(dev, b, f, t, which):
    """Both gradients, then each alone: the other pointer is null, and what stands where it would have pointed is not written (the
    guards of every input -- pred and target lie next to nothing of theirs -- are checked all the same)."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.loss import _backward
    L = _lib.load()
    (pred, hp), (tgt, ht) = _loss_inputs(b, f, t, dev)
    go, hgo = fp.carve_copy(torch.rand((b, 4), generator=torch.Generator().manual_seed(9)) + 0.5, dev)
    need = _bytes_of(L.adn_perceptual_loss_backward_workspace_bytes, b, f, t)
    shapes = [(b, 1, f, t) if which in ("both", "pred") else None, (b, 1, f, t) if which in ("both", "target") else None]
    gp, gt = _two_fills(lambda ws, nb, o: L.adn_perceptual_loss_backward(pred.data_ptr(), tgt.data_ptr(), b, f, t, go.data_ptr(), ws, nb,
                                                                         o[0], o[1], None),
                        need, shapes, [(pred, hp), (tgt, ht), (go, hgo)], dev, f"adn_perceptual_loss_backward {b} x {f}x{t} ({which})")
    wp, wt = _backward(pred, tgt, go, shapes[0] is not None, shapes[1] is not None)
    assert (gp is None) == (wp is None) and (gt is None) == (wt is None)
    assert (gp is None or torch.equal(gp, wp)) and (gt is None or torch.equal(gt, wt))


@pytest.mark.parametrize("n,bins,frames,n_fft,hop,iters", [(2, 257, 188, 512, 128, 2), (1, 33, 9, 64, 16, 2)], ids=["2x257x188", "1x33x9"])
def test_griffin_lim_footprint(dev, n, bins, frames, n_fft, hop, iters):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.griffin_lim import griffin_lim_reconstruction
    L = _lib.load()
    g = torch.Generator().manual_seed(bins)
    mag, hm = fp.carve_copy(torch.rand((n, bins, frames), generator=g) * 2, dev)
    rnd, hr = fp.carve_copy(torch.rand((n, bins, frames), generator=g), dev)
    need = _bytes_of(L.adn_griffin_lim_workspace_bytes, n, bins, frames)
    out, = _two_fills(lambda ws, nb, o: L.adn_griffin_lim(mag.data_ptr(), rnd.data_ptr(), n, bins, frames, n_fft, hop, iters, ws, nb, o[0], None),
                      need, [(n, hop * (frames - 1))], [(mag, hm), (rnd, hr)], dev, f"adn_griffin_lim {n} x {bins}x{frames}")
    assert torch.equal(out, griffin_lim_reconstruction(mag, n_fft, hop, iterations=iters, rand=rnd))


GL_TOL = 1e-4                                            # tests/test_gpu_parity.py::TOL, of max|ref|
ISTFT_SIZES = [(512, 128, 188), (64, 16, 9), (128, 32, 7), (2048, 512, 5), (4096, 1024, 3)]


@pytest.mark.parametrize("n_fft,hop,nfr", ISTFT_SIZES, ids=[_shape_id(s) for s in ISTFT_SIZES])
def test_istft_footprint(dev, n_fft, hop, nfr):
    """128, 2048 and 4096 are instantiations of istft_frames_kernel (csrc/gl_kernels.hip) that no other test runs: those are compared
    with the numpy oracle as well, as tests/test_gpu_parity.py::test_istft_and_complex_stft_match_oracle compares the other sizes."""
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.griffin_lim import istft, stft_complex
    L = _lib.load()
    rng = np.random.default_rng(n_fft + nfr)
    bins = n_fft // 2 + 1
    spec = (rng.normal(size=(2, bins, nfr)) + 1j * rng.normal(size=(2, bins, nfr))).astype(np.complex64)
    fm_host = torch.from_numpy(np.ascontiguousarray(spec.transpose(0, 2, 1)))                   # frame-major
    fm, hfm = fp.carve_copy(torch.view_as_real(fm_host).contiguous(), dev)
    need = _bytes_of(L.adn_istft_workspace_bytes, 2, nfr, n_fft)
    out, = _two_fills(lambda ws, nb, o: L.adn_istft(fm.data_ptr(), 2, nfr, n_fft, hop, ws, nb, o[0], None),
                      need, [(2, hop * (nfr - 1))], [(fm, hfm)], dev, f"adn_istft {n_fft}/{hop} x {nfr}")
    assert torch.equal(out, istft(torch.view_as_complex(fm), hop))
    if n_fft in (128, 2048, 4096):
        from oracle import griffin_lim_numpy as gl
        got = out.cpu().numpy()
        for c in range(2):
            ref = gl.istft(spec[c], hop)
            assert got[c].shape == ref.shape and np.max(np.abs(got[c] - ref)) <= GL_TOL * np.max(np.abs(ref))
        audio = rng.uniform(-1, 1, (2, hop * (nfr - 1))).astype(np.float32)
        z = stft_complex(torch.from_numpy(audio).to(dev), n_fft, hop).cpu().numpy()
        for c in range(2):
            ref = gl.stft_complex(audio[c], n_fft, hop, True).T
            assert z[c].shape == ref.shape and np.max(np.abs(z[c] - ref)) <= GL_TOL * np.max(np.abs(ref))


@pytest.mark.parametrize("n,length", [(4, 16000), (1, 1)], ids=["4x16000", "1x1"])
def test_mix_snr_footprint(dev, n, length):
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.resample import mix_snr
    L = _lib.load()
    g = torch.Generator().manual_seed(length)
    clean, hc = fp.carve_copy(torch.rand((n, length), generator=g) - 0.5, dev)
    noise, hn = fp.carve_copy(torch.rand((n, length), generator=g) * 2 - 1, dev)
    need = _bytes_of(L.adn_mix_snr_workspace_bytes, n, length)
    out, = _two_fills(lambda ws, nb, o: L.adn_mix_snr(clean.data_ptr(), noise.data_ptr(), n, length, 8.0, ws, nb, o[0], None),
                      need, [(n, length)], [(clean, hc), (noise, hn)], dev, f"adn_mix_snr {n} x {length}")
    assert torch.equal(out, mix_snr(clean, noise, 8.0))
