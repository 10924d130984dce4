"""adn_perceptual_loss, adn_perceptual_loss_backward and adn_per_clip_l1 on the device over the case table of tests/loss_cases.py,
against the float64 restatement of tests/loss_ref.py computed on the CPU.

Bounds (derived, not tuned).  Per case and per statistic the FLOOR is the largest deviation from float64, over the clips of the
case, of the two float32 host restatements (library order and kernel order, loss_ref.floors), never below 2^-23; it is measured
when the test runs, from the restatements alone, never from a device figure.  Then
* per clip and output column: |got - ref| <= 4 floor |ref|;
* per clip and gradient: ||g - g_ref||_2 <= 4 floor_l2 ||g_ref||_2 and max|g - g_ref| <= 4 floor_max max|g_ref|,
the gradients those of sum(per_clip * W) with a distinct weight per clip and column (loss_cases.weights).  The factor 4 is the
project's standing margin over a float32 floor (tests/test_gpu_dereverb_stream.py): room for another summation order, more than two
orders of magnitude below the smallest mutation of tests/test_loss_cases_host.py, each of which lands at least 10 bounds out.
Exact: the far field of the bursts and the pred == target clip are 0 bit for bit, an input one float into a buffer gives the bits
of an aligned one, two backward calls give the same bits.  Every ratio is printed before it is asserted; profiles/loss_cases.md
holds the measured ones.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as C  # noqa: E402
import loss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda", 0)


def _one_float_in(x, dev):
    """x on the device as a contiguous tensor that starts 4 bytes into its buffer (not 16-byte aligned)."""
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def device_run(c, dev, misaligned=False):
    """(out, grad_pred, grad_target) of the device for sum(per_clip * W), on the device in float32."""
    from audiodenoiser_amd.loss import perceptual_loss_per_clip
    put = (lambda x: _one_float_in(x, dev)) if misaligned else (lambda x: x.to(dev))
    p = put(c.pred).detach().requires_grad_()
    q = put(c.target).detach().requires_grad_()
    if misaligned:
        assert p.data_ptr() % 16 == 4 and q.data_ptr() % 16 == 4
    out = perceptual_loss_per_clip(p, q)
    (out * c.W.to(dev)).sum().backward()
    return out.detach(), p.grad, q.grad


def check(name, got):
    """Every statistic of every clip against 4 x its floor; returns the worst ratio to the floor."""
    dev = R.deviations(tuple(g.cpu().double() for g in got), C.reference(name))
    both = C.floors(name)
    fl = both["floor"]
    worst = 0.0
    for k in R.STATS:
        ratio = float(dev[k].max()) / fl[k]
        print(f"{name} {k}: device {float(dev[k].max()):.3g}, library {both['library'][k]:.3g}, kernel {both['kernel'][k]:.3g}, "
              f"floor {fl[k]:.3g}, ratio {ratio:.2f} (bound 4)" + ("  ABOVE THE FLOOR" if ratio > 1 else ""))
        worst = max(worst, ratio)
    for k in R.STATS:
        assert bool((dev[k] <= R.MARGIN * fl[k]).all()), (name, k, float(dev[k].max()), fl[k])
    return worst


@pytest.mark.parametrize("name", C.GRAD_CASES)
def test_case_at_the_float32_floor(dev, name):
    c = C.case(name)
    got = device_run(c, dev)
    check(name, got)
    for clip in c.identical:                                  # pred == target: the output row and both gradients are exactly 0
        assert all(float(g[clip].abs().max()) == 0.0 for g in got), name
    if c.bursts is not None:                                  # farther than 62 positions from the burst and its reflections: 0
        far = C.far_field(c)[:, None, None, :].expand(c.shape).to(dev)
        assert int(far.sum()) > 0
        assert float(got[1][far].abs().max()) == 0.0 and float(got[2][far].abs().max()) == 0.0, name


def test_one_float_into_a_buffer_gives_the_same_bits(dev):
    """T % 4 == 0 and a misaligned tensor: loss_grad_input_kernel<1> where <4> would run on an aligned one."""
    for name in C.ALIGN:
        c = C.case(name)
        a = device_run(c, dev)
        b = device_run(c, dev, misaligned=True)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.contiguous().view(torch.int32)), name
        check(name, b)


def test_two_backward_calls_at_tb_128_are_bit_identical(dev):
    c = C.case("tb:8x8200")
    assert c.info["tb"] == 128
    a = device_run(c, dev)
    b = device_run(c, dev)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("elems", C.L1_ELEMS)
def test_per_clip_l1_at_the_float32_floor(dev, elems):
    from audiodenoiser_amd.loss import per_clip_l1
    a, b = C.l1_inputs(elems)
    ref = R.l1_float64(a, b)
    floor = max(float(((R.l1_kernel_order(a, b).double() - ref).abs() / ref).max()), R.EPS32)
    got = per_clip_l1(a.to(dev), b.to(dev)).cpu().double()
    err = float(((got - ref).abs() / ref).max())
    print(f"per_clip_l1 elems {elems}: device {err:.3g}, floor {floor:.3g}, ratio {err / floor:.2f} (bound 4)")
    assert bool(((got - ref).abs() <= R.MARGIN * floor * ref).all()), (elems, err, floor)
