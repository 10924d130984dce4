"""Spectral baseline denoiser: noise tracking + Wiener gain, no checkpoint.

    from audiodenoiser_amd.baseline import SpectralDenoiser, SpectralParams, spectral_gain
    dn = SpectralDenoiser()                            # no model: the current ROCm device, 8 kHz, n_fft 512, hop 128
    clean = dn.denoise(noisy, sr=44100)                # (L,) or (N, L); numpy -> numpy, device tensor -> device tensor
    dn.denoise_file("noisy.wav", "clean.wav")

    python -m audiodenoiser_amd.baseline IN OUT [--reference CLEAN] [--bias 1.0] [--gain-floor 0.1]

The operator is DEFINED in ``include/adn.h`` ("baseline"; float64 restatement: ``tests/baseline_ref.py``) and is unpinned against
any package: Doblinger's continuous minimum tracking for the noise power, the decision-directed a-priori SNR of Ephraim and Malah,
a Wiener gain with a floor.  It is causal, carries three floats per bin and needs no weights, which makes it the figure a trained
network has to beat in the ``--reference`` report.  ``SpectralDenoiser`` is ``Denoiser`` with the network replaced:

1. ``adn_stft_complex``: the centred complex STFT, ``T = 1 + L // hop`` frames;
2. ``adn_spectral_gain`` (``csrc/baseline_kernels.hip``) into a zeroed ``(n, 1, F, max(T, 16))`` buffer;
3. ``adn_denoise_resynth`` with ``window = max(T, 16)`` and ``overlap = 0``: one window per clip, the plan's exact pass-through
   case ("a frame covered by one window is y itself, bit for bit"), the noisy input's own phase, all ``L`` samples back.

``denoise``, ``denoise_file``, the rate handling and the every-channel-a-clip rule are ``Denoiser``'s, unchanged.

What is NOT here: streaming (the state layout and the per-row fresh-start sentinel are there for it; ``StreamDenoiser`` /
``StreamPool`` would need a bin-major magnitude input form of the kernel), Griffin-Lim phase, log-MMSE gains, any tuning of the
defaults by ear.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os

import torch

from . import _lib
from .denoise import Denoiser, _report, _stream
from .griffin_lim import stft_complex

__all__ = ["SpectralParams", "spectral_gain", "SpectralDenoiser"]


@dataclasses.dataclass(frozen=True)
class SpectralParams:
    """``adn_spectral_params`` of ``include/adn.h`` with its defaults and its legal ranges."""
    smooth: float = 0.7
    beta: float = 0.96
    gamma: float = 0.998
    alpha: float = 0.98
    gain_floor: float = 0.1
    bias: float = 1.0

    def __post_init__(self):
        for name in ("smooth", "beta", "alpha"):
            if not 0.0 <= float(getattr(self, name)) < 1.0:
                raise ValueError(f"SpectralParams: need 0 <= {name} < 1")
        if not 0.0 < float(self.gamma) < 1.0:
            raise ValueError("SpectralParams: need 0 < gamma < 1")
        if not 0.0 < float(self.gain_floor) <= 1.0:
            raise ValueError("SpectralParams: need 0 < gain_floor <= 1")
        if not 0.0 < float(self.bias) <= 100.0:
            raise ValueError("SpectralParams: need 0 < bias <= 100")

    def to_struct(self) -> "_lib.SpectralParamsStruct":
        return _lib.SpectralParamsStruct(*(float(v) for v in dataclasses.astuple(self)))

    @classmethod
    def from_struct(cls, s) -> "SpectralParams":
        return cls(*(float(getattr(s, name)) for name, _ in _lib.SpectralParamsStruct._fields_))


def spectral_gain(spec: torch.Tensor, params: SpectralParams = None, state: torch.Tensor = None, out: torch.Tensor = None,
                  col0: int = 0):
    """``adn_spectral_gain`` on the current stream.  ``spec``: complex64 ``(n_clips, T, F)`` on a ROCm device (``stft_complex``).
    ``state``: float32 ``(n_clips, 3, F)`` carried from the previous call (rows ``P``, ``Pmin``, ``S``; a row whose ``P`` is
    negative starts fresh), or None: every row starts fresh.  ``out``: float32 ``(n_clips, 1, F, width)`` whose columns
    ``[col0, col0 + T)`` are written and nothing else; None allocates ``(n_clips, 1, F, T)``.  Returns ``(out, new_state)``; the
    new state is a new tensor, ``state`` itself is left as it was."""
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 3:
        raise ValueError("spectral_gain: expected a (n_clips, n_frames, n_bins) complex64 tensor on a ROCm device")
    n, t, f = spec.shape
    if n < 1 or t < 1 or f < 1:
        raise ValueError("spectral_gain: need at least one clip, one frame and one bin")
    dev = spec.device
    s = torch.view_as_real(spec.contiguous())
    if state is not None:
        if not state.is_cuda or state.device != dev or state.dtype != torch.float32 or tuple(state.shape) != (n, 3, f):
            raise ValueError("spectral_gain: state must be a (n_clips, 3, n_bins) float32 tensor on spec's device")
        state = state.contiguous()
    if out is None:
        if col0 != 0:
            raise ValueError("spectral_gain: col0 needs an out buffer")
        out = torch.empty((n, 1, f, t), dtype=torch.float32, device=dev)
    elif (not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[:3]) != (n, 1, f)
          or not out.is_contiguous()):
        raise ValueError("spectral_gain: out must be a contiguous (n_clips, 1, n_bins, width) float32 tensor on spec's device")
    new_state = torch.empty((n, 3, f), dtype=torch.float32, device=dev)
    p = ctypes.byref(params.to_struct()) if params is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().adn_spectral_gain(s.data_ptr(), n, t, f, p, state.data_ptr() if state is not None else None,
                                                 new_state.data_ptr(), out.data_ptr(), int(out.shape[3]), int(col0), _stream(dev)),
                   "adn_spectral_gain")
    return out, new_state


class SpectralDenoiser(Denoiser):
    """``Denoiser`` with the spectral baseline in the network's place: no model, noisy phase only."""

    def __init__(self, device=None, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128,
                 params: SpectralParams = None):
        if not (isinstance(n_fft, int) and 64 <= n_fft <= 4096 and n_fft & (n_fft - 1) == 0):
            raise ValueError("SpectralDenoiser: n_fft must be a power of two in [64, 4096]")
        if not (isinstance(hop_length, int) and 1 <= hop_length <= n_fft // 4):
            raise ValueError("SpectralDenoiser: need 1 <= hop_length <= n_fft / 4 (the inverse transform of the whole input length "
                             "divides by a window sum-of-squares that falls to 2e-8 at n_fft / 2)")
        if not (isinstance(sample_rate, int) and sample_rate >= 1):
            raise ValueError("SpectralDenoiser: sample_rate must be >= 1")
        if params is not None and not isinstance(params, SpectralParams):
            raise TypeError("SpectralDenoiser: params must be a SpectralParams")
        dev = _lib.staging_device() if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("SpectralDenoiser: the device must be a ROCm device; there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.model, self.device = None, dev
        self.sample_rate, self.n_fft, self.hop_length = sample_rate, n_fft, hop_length
        self.params = SpectralParams() if params is None else params
        self.phase = "noisy"
        self.n_bins = n_fft // 2 + 1

    def gain(self, spec: torch.Tensor) -> torch.Tensor:
        """complex64 ``(n_clips, T, F)`` -> the magnitudes ``(n_clips, 1, F, max(T, 16))`` that ``adn_denoise_resynth`` reads as
        one window per clip; the columns at and past ``T`` are zero."""
        n, t, f = spec.shape
        y = torch.zeros((n, 1, f, max(t, 16)), dtype=torch.float32, device=spec.device)
        return spectral_gain(spec, self.params, None, y, 0)[0]

    def _core(self, x: torch.Tensor, rand) -> torch.Tensor:
        """``x`` (n_clips, L) at the working rate -> (n_clips, L)."""
        n, length = x.shape
        spec = stft_complex(x, self.n_fft, self.hop_length)
        y = self.gain(spec)
        out = torch.empty((n, length), dtype=torch.float32, device=x.device)
        s = torch.view_as_real(spec)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().adn_denoise_resynth(y.data_ptr(), s.data_ptr(), n, length, self.n_fft, self.hop_length,
                                                       int(y.shape[3]), 0, out.data_ptr(), _stream(x.device)),
                       "adn_denoise_resynth")
        return out


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.baseline",
                                 description="Denoise a wav file or a folder of wav files with the spectral baseline (no checkpoint).")
    ap.add_argument("src", metavar="IN", help="a wav file, or a folder of wav files")
    ap.add_argument("dst", metavar="OUT", help="the wav file to write, or the folder to write into")
    ap.add_argument("--reference", metavar="CLEAN", default=None,
                    help="the clean wav of IN (or a folder with IN's file names): print one JSON line of metrics per file")
    ap.add_argument("--bias", type=float, default=SpectralParams.bias, help="noise over-estimation factor (0, 100]")
    ap.add_argument("--gain-floor", type=float, default=SpectralParams.gain_floor, help="smallest gain (0, 1]")
    args = ap.parse_args(argv)
    dn = SpectralDenoiser(params=SpectralParams(bias=args.bias, gain_floor=args.gain_floor))
    if os.path.isdir(args.src):
        os.makedirs(args.dst, exist_ok=True)
        jobs = [(os.path.join(args.src, f), os.path.join(args.dst, f)) for f in sorted(os.listdir(args.src)) if f.lower().endswith(".wav")]
    else:
        jobs = [(args.src, args.dst)]
    for src, dst in jobs:
        n, rate = dn.denoise_file(src, dst)
        print(f"{src} -> {dst}: {n} samples at {rate} Hz")
        if args.reference is not None:
            ref = os.path.join(args.reference, os.path.basename(src)) if os.path.isdir(args.reference) else args.reference
            print(_report(src, dst, ref))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
