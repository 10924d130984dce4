"""Dereverberation baseline: weighted prediction error (WPE) per frequency bin, no checkpoint.

    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams, wpe
    dr = Dereverberator()                              # no model: the current ROCm device, 8 kHz, n_fft 512, hop 128
    dry = dr.denoise(reverberant, sr=44100)            # (L,) or (N, L); numpy -> numpy, device tensor -> device tensor
    dr.denoise_file("room.wav", "dry.wav")
    Dereverberator(gain=True)                          # WPE, then the Wiener gain of the spectral baseline on its result

    python -m audiodenoiser_amd.dereverb IN OUT [--reference CLEAN] [--taps K] [--delay D] [--iterations I] [--gain]

The operator is DEFINED in ``include/adn.h`` ("dereverb"; float64 restatement: ``tests/dereverb_ref.py``) and is unpinned against
any package: single-channel WPE, delayed linear prediction per frequency bin with the variance re-estimated from the last result
(Nakatani et al. 2010).  A gain per bin cannot undo a filter, so this -- not ``SpectralDenoiser`` -- is the figure a network trained
on the ``reverb`` noise type has to beat in the ``--reference`` report.  ``Dereverberator`` is ``Denoiser`` with the network replaced:

1. ``adn_stft_complex``: the centred complex STFT, ``T = 1 + L // hop`` frames;
2. ``adn_wpe`` (``csrc/dereverb_kernels.hip``): the dereverberated spectrum ``d``, and its magnitudes into a zeroed
   ``(n, 1, F, max(T, 16))`` buffer -- with ``gain=True`` ``adn_spectral_gain`` on ``d`` writes the magnitudes instead;
3. ``adn_denoise_resynth`` with ``window = max(T, 16)`` and ``overlap = 0``: one window per clip, the plan's exact pass-through
   case, the phase of ``d`` itself, all ``L`` samples back.

``denoise``, ``denoise_file``, the rate handling and the every-channel-a-clip rule are ``Denoiser``'s, unchanged.

What is NOT here: online / recursive WPE for streams, more than one channel, any tuning of the defaults by ear.  There is no CPU
path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os

import torch

from . import _lib
from .baseline import SpectralParams, spectral_gain
from .denoise import Denoiser, _report, _stream
from .griffin_lim import stft_complex

__all__ = ["WpeParams", "wpe", "Dereverberator"]


@dataclasses.dataclass(frozen=True)
class WpeParams:
    """``adn_wpe_params`` of ``include/adn.h`` with its defaults and its legal ranges."""
    taps: int = 20
    delay: int = 3
    iterations: int = 3
    loading: float = 1e-3
    power_floor: float = 1e-3

    def __post_init__(self):
        for name, lo, hi in (("taps", 1, 32), ("delay", 1, 8), ("iterations", 1, 8)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"WpeParams: need an integer {lo} <= {name} <= {hi}")
        for name in ("loading", "power_floor"):
            if math.isnan(float(getattr(self, name))):
                raise ValueError(f"WpeParams: {name} is NaN")
        if not 1e-6 <= float(self.loading) <= 1.0:
            raise ValueError("WpeParams: need 1e-6 <= loading <= 1")
        if not 0.0 < float(self.power_floor) <= 1.0:
            raise ValueError("WpeParams: need 0 < power_floor <= 1")

    def to_struct(self) -> "_lib.WpeParamsStruct":
        return _lib.WpeParamsStruct(int(self.taps), int(self.delay), int(self.iterations), float(self.loading), float(self.power_floor))


def wpe(spec: torch.Tensor, params: WpeParams = None, mag_out: torch.Tensor = None):
    """``adn_wpe`` on the current stream.  ``spec``: complex64 ``(n_clips, T, F)`` on a ROCm device (``stft_complex``).
    ``mag_out``: float32 ``(n_clips, 1, F, width)``, ``width >= T``, whose columns ``[0, T)`` are written and nothing else; None
    allocates ``(n_clips, 1, F, T)``.  The workspace is allocated here.  Returns ``(spec_out, mag_out)``, ``spec_out`` a new
    complex64 tensor of ``spec``'s shape."""
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 3:
        raise ValueError("wpe: expected a (n_clips, n_frames, n_bins) complex64 tensor on a ROCm device")
    if params is not None and not isinstance(params, WpeParams):
        raise TypeError("wpe: params must be a WpeParams")
    n, t, f = spec.shape
    if n < 1 or t < 1 or f < 1:
        raise ValueError("wpe: need at least one clip, one frame and one bin")
    dev = spec.device
    s = torch.view_as_real(spec.contiguous())
    if mag_out is None:
        mag_out = torch.empty((n, 1, f, t), dtype=torch.float32, device=dev)
    elif (not isinstance(mag_out, torch.Tensor) or not mag_out.is_cuda or mag_out.device != dev or mag_out.dtype != torch.float32
          or mag_out.dim() != 4 or tuple(mag_out.shape[:3]) != (n, 1, f) or not mag_out.is_contiguous()):
        raise ValueError("wpe: mag_out must be a contiguous (n_clips, 1, n_bins, width) float32 tensor on spec's device")
    out = torch.empty((n, t, f, 2), dtype=torch.float32, device=dev)
    p = ctypes.byref(params.to_struct()) if params is not None else None
    L = _lib.load()
    need = ctypes.c_size_t(0)
    _lib.check(L.adn_wpe_workspace_bytes(n, t, f, p, ctypes.byref(need)), "adn_wpe_workspace_bytes")
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev) if need.value else None
    with torch.cuda.device(dev):
        _lib.check(L.adn_wpe(s.data_ptr(), n, t, f, p, ws.data_ptr() if ws is not None else None, need.value, out.data_ptr(),
                             mag_out.data_ptr(), int(mag_out.shape[3]), _stream(dev)), "adn_wpe")
    return torch.view_as_complex(out), mag_out


class Dereverberator(Denoiser):
    """``Denoiser`` with WPE in the network's place: no model, the phase of the dereverberated spectrum.  ``gain=True`` runs the
    spectral baseline's Wiener gain (``gain_params``) on the result of WPE: the cascade."""

    def __init__(self, device=None, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128, params: WpeParams = None,
                 gain: bool = False, gain_params: SpectralParams = None):
        if not (isinstance(n_fft, int) and 64 <= n_fft <= 4096 and n_fft & (n_fft - 1) == 0):
            raise ValueError("Dereverberator: n_fft must be a power of two in [64, 4096]")
        if not (isinstance(hop_length, int) and 1 <= hop_length <= n_fft // 4):
            raise ValueError("Dereverberator: need 1 <= hop_length <= n_fft / 4 (the inverse transform of the whole input length "
                             "divides by a window sum-of-squares that falls to 2e-8 at n_fft / 2)")
        if not (isinstance(sample_rate, int) and sample_rate >= 1):
            raise ValueError("Dereverberator: sample_rate must be >= 1")
        if params is not None and not isinstance(params, WpeParams):
            raise TypeError("Dereverberator: params must be a WpeParams")
        if gain_params is not None and not isinstance(gain_params, SpectralParams):
            raise TypeError("Dereverberator: gain_params must be a SpectralParams")
        dev = _lib.staging_device() if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("Dereverberator: the device must be a ROCm device; there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.model, self.device = None, dev
        self.sample_rate, self.n_fft, self.hop_length = sample_rate, n_fft, hop_length
        self.params = WpeParams() if params is None else params
        self.gain = bool(gain)
        self.gain_params = SpectralParams() if gain_params is None else gain_params
        self.phase = "dereverberated"
        self.n_bins = n_fft // 2 + 1

    def _core(self, x: torch.Tensor, rand) -> torch.Tensor:
        """``x`` (n_clips, L) at the working rate -> (n_clips, L)."""
        n, length = x.shape
        spec = stft_complex(x, self.n_fft, self.hop_length)
        t, f = spec.shape[1], spec.shape[2]
        y = torch.zeros((n, 1, f, max(t, 16)), dtype=torch.float32, device=x.device)
        d, _ = wpe(spec, self.params, y)
        if self.gain:
            spectral_gain(d, self.gain_params, None, y, 0)
        out = torch.empty((n, length), dtype=torch.float32, device=x.device)
        s = torch.view_as_real(d)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().adn_denoise_resynth(y.data_ptr(), s.data_ptr(), n, length, self.n_fft, self.hop_length,
                                                       int(y.shape[3]), 0, out.data_ptr(), _stream(x.device)),
                       "adn_denoise_resynth")
        return out


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.dereverb",
                                 description="Dereverberate a wav file or a folder of wav files with per-bin WPE (no checkpoint).")
    ap.add_argument("src", metavar="IN", help="a wav file, or a folder of wav files")
    ap.add_argument("dst", metavar="OUT", help="the wav file to write, or the folder to write into")
    ap.add_argument("--reference", metavar="CLEAN", default=None,
                    help="the dry wav of IN (or a folder with IN's file names): print one JSON line of metrics per file")
    ap.add_argument("--taps", type=int, default=WpeParams.taps, help="prediction taps K, 1 ... 32")
    ap.add_argument("--delay", type=int, default=WpeParams.delay, help="prediction delay D in frames, 1 ... 8")
    ap.add_argument("--iterations", type=int, default=WpeParams.iterations, help="iterations I, 1 ... 8")
    ap.add_argument("--gain", action="store_true", help="run the spectral baseline's Wiener gain on the result of WPE")
    args = ap.parse_args(argv)
    try:
        params = WpeParams(taps=args.taps, delay=args.delay, iterations=args.iterations)
    except ValueError as exc:
        ap.error(str(exc))
    dn = Dereverberator(params=params, gain=args.gain)
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
