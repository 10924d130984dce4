"""Gradient of CombinedPerceptualLoss, host side: the differentiable float64 restatement the GPU gradient tests compare against
(anchored to oracle/loss_torch.per_clip and checked by gradcheck), and the host argument checks of the two backward entry points
of the C ABI (no device needed)."""
import ctypes

import pytest
import torch

from oracle import loss_torch as L


def per_clip_autograd(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(B,1,F,T) x2 -> (B,4) = [total, stft, mel, l1] per clip: oracle/loss_torch.per_clip written without no_grad, in the
    inputs' dtype, so that torch autograd differentiates it (float64 on the CPU is the gradient reference)."""
    b = pred.shape[0]
    dt = pred.dtype
    p = pred.mean(dim=2).squeeze(1)
    q = target.mean(dim=2).squeeze(1)
    stft = torch.zeros(b, dtype=dt)
    for n_fft, hop in L.SCALES:
        win = torch.ones(n_fft, dtype=dt)
        pm = torch.stft(p, n_fft=n_fft, hop_length=hop, return_complex=True, pad_mode="constant", window=win).abs()
        qm = torch.stft(q, n_fft=n_fft, hop_length=hop, return_complex=True, pad_mode="constant", window=win).abs()
        stft = stft + (pm - qm).abs().reshape(b, -1).mean(dim=1)
    stft = stft / len(L.SCALES)
    fb = torch.from_numpy(L.mel_filterbank()).to(dt)
    win = torch.hann_window(L.MEL_NFFT, periodic=True, dtype=dt)

    def mel(x):
        s = torch.stft(x, n_fft=L.MEL_NFFT, hop_length=L.MEL_HOP, window=win, center=True, pad_mode="reflect",
                       return_complex=True).abs().pow(2.0)
        return torch.matmul(s.transpose(1, 2), fb).transpose(1, 2)
    melv = (mel(p) - mel(q)).abs().reshape(b, -1).mean(dim=1)
    l1 = (pred - target).abs().reshape(b, -1).mean(dim=1)
    total = L.W_STFT * stft + L.W_MEL * melv + L.W_L1 * l1
    return torch.stack([total, stft, melv, l1], dim=1)


@pytest.mark.parametrize("shape", [(3, 1, 40, 96), (2, 1, 16, 63), (1, 1, 24, 300)])
def test_restatement_forward_equals_oracle(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g) * 3
    b = torch.rand(shape, generator=g) * 3
    ref = L.per_clip(a, b)
    got = per_clip_autograd(a, b).detach()
    assert torch.allclose(got, ref, rtol=1e-6, atol=0), (got - ref).abs().max()


@pytest.mark.parametrize("shape", [(2, 1, 4, 32), (1, 1, 3, 40)])
def test_restatement_gradcheck_float64(shape):
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(shape, generator=g, dtype=torch.float64) * 3).requires_grad_()
    b = (torch.rand(shape, generator=g, dtype=torch.float64) * 3).requires_grad_()
    assert torch.autograd.gradcheck(per_clip_autograd, (a, b), eps=1e-7, atol=1e-6, rtol=1e-4)


def test_backward_workspace_bytes():
    from audiodenoiser_amd import _lib
    lib = _lib.load()
    need = ctypes.c_size_t()
    for b, f, t in ((1, 64, 32), (2, 513, 256), (64, 513, 256), (2, 24, 65535), (3, 40, 97)):
        assert lib.adn_perceptual_loss_backward_workspace_bytes(b, f, t, ctypes.byref(need)) == 0
        nslab = (f + 31) // 32
        partial = (b * nslab * (2 * t + 1) + 3) // 4 * 4           # row-slab partials, rounded to 16 bytes
        assert need.value == (partial + 2 * b * t) * 4, (b, f, t, need.value)
    assert lib.adn_perceptual_loss_backward_workspace_bytes(1, 64, 1 << 24, ctypes.byref(need)) == 0
    for args in ((1, 64, 31), (1, 64, (1 << 24) + 1), (0, 64, 64), (1, 0, 64)):
        assert lib.adn_perceptual_loss_backward_workspace_bytes(*args, ctypes.byref(need)) == 1, args
    assert lib.adn_perceptual_loss_backward_workspace_bytes(1, 64, 64, None) == 1


def test_backward_argument_checks_before_any_launch():
    from audiodenoiser_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    # T outside [32, 2^24], like the forward (ADN_LOSS_MIN_T / ADN_LOSS_MAX_T)
    assert lib.adn_perceptual_loss_backward(p, p, 1, 64, 31, p, p, big, p, p, None) == 1
    assert b"32 <= T" in lib.adn_last_error()
    assert lib.adn_perceptual_loss_backward(p, p, 1, 64, (1 << 24) + 1, p, p, big, p, p, None) == 1
    assert b"2^24" in lib.adn_last_error()
    # both gradient outputs null
    assert lib.adn_perceptual_loss_backward(p, p, 1, 64, 64, p, p, big, None, None, None) == 1
    assert b"both null" in lib.adn_last_error()
    # null grad_out / inputs
    assert lib.adn_perceptual_loss_backward(p, p, 1, 64, 64, None, p, big, p, p, None) == 1
    assert b"null pointer" in lib.adn_last_error()
    assert lib.adn_perceptual_loss_backward(None, p, 1, 64, 64, p, p, big, p, p, None) == 1
    # workspace too small / missing
    assert lib.adn_perceptual_loss_backward(p, p, 1, 64, 64, p, p, 16, p, p, None) == 3
    assert lib.adn_perceptual_loss_backward(p, p, 1, 64, 64, p, None, big, p, p, None) == 3
