"""Denoise audio of any length and rate end to end: wav in, wav out.

    from audiodenoiser_amd.denoise import Denoiser
    dn = Denoiser(model)                              # an audiodenoiser_amd.model.UNet(1, 1) on a ROCm device, .eval()
    clean = dn.denoise(noisy, sr=44100)               # (L,) or (N, L); numpy -> numpy, device tensor -> device tensor
    dn.denoise_file("noisy.wav", "clean.wav")

    python -m audiodenoiser_amd.denoise --model CKPT.pth IN OUT [--phase noisy|griffin_lim] [--window 256] [--overlap 32]
                                        [--dtype f32|f16] [--reference CLEAN]

The reference only ever feeds one fixed 257 x 188 spectrogram per clip to the network (``test.py:100-114``) and returns to
audio through Griffin-Lim from a random phase (``test.py:29-48``).  This module joins the stages that exist on the device --
``adn_resample``, ``adn_stft_complex``, the U-Net, ``adn_griffin_lim`` -- with the three kernels of ``csrc/denoise_kernels.hip``
(definition: ``include/adn.h``, "denoise"; float64 restatement: ``tests/denoise_ref.py``):

1. the centred complex STFT of the clip, ``T = 1 + L // hop`` frames;
2. its magnitude cut into windows of ``window_frames`` frames that share ``overlap_frames`` frames with their neighbour
   (``adn_denoise_windows``); a clip of at most ``window_frames`` frames is one window of its own width (at least 16), so a
   reference-sized clip goes through the network exactly as the reference feeds it;
3. the U-Net over ``batch_windows`` windows at a time, written into slices of one output buffer;
4. the outputs joined with a linear cross-fade over the shared frames;
5. ``phase="noisy"`` (default): the stitched output clamped at zero, given the noisy input's own phase and inverted by an
   overlap-add inverse STFT that returns all ``L`` samples -- steps 4 and 5 are one kernel, ``adn_denoise_resynth``;
   ``phase="griffin_lim"``: the reference's reconstruction (``griffin_lim_reconstruction``) of the unclamped stitched output,
   ``hop * (T - 1)`` samples zero-padded to ``L``;
6. input at another rate is resampled down to ``sample_rate`` first and the result back up, cut / zero-padded to the input's
   sample count.

A multi-channel input is a batch: every channel (every row of an ``(N, L)`` array) is a clip of its own.

What is NOT claimed: parity of the STFT with librosa stays unpinned, as everywhere in this package.  ``window_frames=256`` and
``overlap_frames=32`` are design defaults; their audible quality is not validated (no trained checkpoint exists where this was
written).  The result of overlapping windows differs from one forward over the whole spectrogram by design -- the network's
receptive field is wider than the overlap -- which is why the single-window case is exact and the multi-window case is defined by
the restatement.  ``--reference`` (a clean wav, or a folder with the input folder's file names) prints, after each output is
written, one JSON line with the four metrics of ``audiodenoiser_amd.metrics`` for the noisy input and for the denoised output
against the reference; they measure this run, not the audible quality of a network.  The command line handles a folder file after file; pooling the windows of different files into one batch is out
of scope.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._host import check_stft_plan, current_stream, model_device, run_files, stage, unet_windows
from .griffin_lim import griffin_lim_reconstruction, stft_complex
from .resample import _resample_device
from .wav import read_wav, write_wav

__all__ = ["Denoiser", "denoise_plan"]


def denoise_plan(n_frames: int, window_frames: int = 256, overlap_frames: int = 32):
    """``(n_windows, window_width)`` for a spectrogram of ``n_frames`` frames (``adn_denoise_plan``, host only)."""
    k, w = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().adn_denoise_plan(int(n_frames), int(window_frames), int(overlap_frames), ctypes.byref(k),
                                            ctypes.byref(w)), "adn_denoise_plan")
    return int(k.value), int(w.value)


class Denoiser:
    def __init__(self, model, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128, window_frames: int = 256,
                 overlap_frames: int = 32, phase: str = "noisy", batch_windows: int = 64, gl_iterations: int = 50):
        check_stft_plan("Denoiser", n_fft, hop_length, sample_rate)
        if not (isinstance(window_frames, int) and window_frames >= 16):
            raise ValueError("Denoiser: window_frames must be >= 16 (the network pools four times)")
        if not (isinstance(overlap_frames, int) and 0 <= overlap_frames <= window_frames // 2):
            raise ValueError("Denoiser: need 0 <= overlap_frames <= window_frames / 2")
        if phase not in ("noisy", "griffin_lim"):
            raise ValueError("Denoiser: phase must be 'noisy' or 'griffin_lim'")
        if not (isinstance(batch_windows, int) and batch_windows >= 1):
            raise ValueError("Denoiser: batch_windows must be >= 1")
        if not (isinstance(gl_iterations, int) and gl_iterations >= 0):
            raise ValueError("Denoiser: gl_iterations must be >= 0")
        self.model = model
        self._setup(model_device("Denoiser", model), sample_rate, n_fft, hop_length, phase, window_frames, overlap_frames,
                    batch_windows, gl_iterations)

    def _setup(self, dev, sample_rate, n_fft, hop_length, phase, window_frames=None, overlap_frames=None, batch_windows=None,
               gl_iterations=None):
        """Everything of the constructor that needs no model.  A subclass with an operator in the network's place has no window
        plan: it leaves those four None, sets ``model = None``, and the building blocks below refuse."""
        self.device = dev
        self.sample_rate, self.n_fft, self.hop_length = sample_rate, n_fft, hop_length
        self.window_frames, self.overlap_frames = window_frames, overlap_frames
        self.phase, self.batch_windows, self.gl_iterations = phase, batch_windows, gl_iterations
        self.n_bins = n_fft // 2 + 1

    def _needs_network(self, what: str) -> None:
        if self.model is None:
            raise RuntimeError(f"{type(self).__name__}: there is no network; {what} belongs to the window plan around one "
                               "(here _core runs the operator on the whole spectrogram)")

    # ------------------------------------------------------------------ building blocks (device tensors)
    def plan(self, n_frames: int):
        self._needs_network("plan")
        return denoise_plan(n_frames, self.window_frames, self.overlap_frames)

    def windows(self, spec: torch.Tensor) -> torch.Tensor:
        """complex64 ``(n_clips, T, F)`` (``stft_complex``) -> network input ``(n_clips * K, 1, F, width)``."""
        self._needs_network("windows")
        if not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 3:
            raise ValueError("Denoiser.windows: expected a (n_clips, n_frames, n_bins) complex64 tensor on a ROCm device")
        s = torch.view_as_real(spec.contiguous())
        n, t, f = spec.shape
        k, w = self.plan(t)
        out = torch.empty((n * k, 1, f, w), dtype=torch.float32, device=spec.device)
        with torch.cuda.device(spec.device):
            _lib.check(_lib.load().adn_denoise_windows(s.data_ptr(), n, t, f, self.window_frames, self.overlap_frames,
                                                       out.data_ptr(), current_stream(spec.device)), "adn_denoise_windows")
        return out

    def network(self, x: torch.Tensor) -> torch.Tensor:
        """The U-Net over ``batch_windows`` windows at a time, into slices of one output buffer."""
        self._needs_network("network")
        return unet_windows("Denoiser", self.model, x, self.batch_windows)

    def stitch(self, y: torch.Tensor, n_clips: int, n_frames: int, clamp: bool) -> torch.Tensor:
        """Network output ``(n_clips * K, 1, F, width)`` -> ``(n_clips, F, n_frames)``, cross-faded (``adn_denoise_stitch``)."""
        self._needs_network("stitch")
        y = y.contiguous()
        f = y.shape[2]
        out = torch.empty((n_clips, f, n_frames), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().adn_denoise_stitch(y.data_ptr(), n_clips, n_frames, f, self.window_frames, self.overlap_frames,
                                                      int(bool(clamp)), out.data_ptr(), current_stream(y.device)), "adn_denoise_stitch")
        return out

    def resynth(self, y: torch.Tensor, spec: torch.Tensor, length: int) -> torch.Tensor:
        """Network output + the input's complex STFT -> audio ``(n_clips, length)`` (``adn_denoise_resynth``)."""
        self._needs_network("resynth")
        return self._resynth(y, spec, length, self.window_frames, self.overlap_frames)

    def _resynth(self, y: torch.Tensor, spec: torch.Tensor, length: int, window_frames: int, overlap_frames: int) -> torch.Tensor:
        """``adn_denoise_resynth`` under a window plan given by the caller: the object's, or, for a subclass whose operator wrote
        one window per clip, ``(y.shape[3], 0)`` -- the plan's exact pass-through case, "a frame covered by one window is y itself"."""
        y = y.contiguous()
        s = torch.view_as_real(spec.contiguous())
        n = spec.shape[0]
        out = torch.empty((n, length), dtype=torch.float32, device=y.device)
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().adn_denoise_resynth(y.data_ptr(), s.data_ptr(), n, length, self.n_fft, self.hop_length,
                                                       window_frames, overlap_frames, out.data_ptr(), current_stream(y.device)),
                       "adn_denoise_resynth")
        return out

    def _core(self, x: torch.Tensor, rand) -> torch.Tensor:
        """``x`` (n_clips, L) at the working rate -> (n_clips, L)."""
        n, length = x.shape
        t = 1 + length // self.hop_length
        if self.phase == "griffin_lim" and t < 2:
            raise ValueError("Denoiser: phase='griffin_lim' needs at least hop_length samples at the working rate")
        spec = stft_complex(x, self.n_fft, self.hop_length)
        y = self.network(self.windows(spec))
        if self.phase == "noisy":
            return self.resynth(y, spec, length)
        stitched = self.stitch(y, n, t, clamp=False)
        audio = griffin_lim_reconstruction(stitched, self.n_fft, self.hop_length, self.gl_iterations, rand=rand)
        out = torch.zeros((n, length), dtype=torch.float32, device=x.device)
        out[:, :audio.shape[1]] = audio
        return out

    # ------------------------------------------------------------------ public surface
    # A subclass whose operator treats the channels of a recording jointly sets this: ``denoise`` then takes (C, L) as ONE recording
    # of C channels and (N, C, L) as a batch of recordings, and calls ``_core(x, rand, channels=C)`` on the (N C, L) rows.
    joint_channels = False

    def denoise(self, audio, sr=None, rand=None):
        """``audio`` (L,) or (N, L) float32 at rate ``sr`` (default: the working rate) -> the same shape at the same rate.
        numpy in -> numpy out, tensor on a ROCm device in -> tensor there out; everything between the input copy and the
        output copy runs on the device on the current stream.  ``rand`` (``(N, F, T)`` uniform [0, 1)) makes
        ``phase="griffin_lim"`` reproducible, as in ``griffin_lim_reconstruction``."""
        a, is_np = stage("Denoiser.denoise", audio, self.device)
        single = a.dim() == 1
        x = (a[None] if single else a).contiguous()
        shape, core = x.shape, self._core
        if self.joint_channels:
            if x.dim() not in (2, 3) or min(shape) < 1:
                raise ValueError("Denoiser.denoise: joint channels: audio must be (L,), (C, L) or (N, C, L) with at least one sample")
            x, core = x.reshape(-1, shape[-1]), functools.partial(self._core, channels=int(shape[-2]))
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("Denoiser.denoise: audio must be (L,) or (N, L) with at least one sample")
        rate = self.sample_rate if sr is None else int(sr)
        length = x.shape[1]
        if rate != self.sample_rate:
            low = core(_resample_device(x, rate, self.sample_rate), rand)
            up = _resample_device(low, self.sample_rate, rate)
            if up.shape[1] >= length:
                out = up[:, :length].contiguous()
            else:
                out = torch.zeros_like(x)
                out[:, :up.shape[1]] = up
        else:
            out = core(x, rand)
        out = out.reshape(shape)
        out = out[0] if single else out
        return out.cpu().numpy() if is_np else out

    def denoise_spectrogram(self, mag):
        """Magnitudes ``(F, T)`` or ``(N, F, T)`` of any ``T >= 1`` -> the stitched network output of the same shape (no clamp):
        the reference's ``test.py:100-114`` for spectrograms longer than the network's window.  For ``16 <= T <= window_frames``
        it is ``model(mag[:, None])[:, 0]`` bit for bit."""
        self._needs_network("denoise_spectrogram")
        m, is_np = stage("Denoiser.denoise_spectrogram", mag, self.device, "magnitudes")
        single = m.dim() == 2
        m = (m[None] if single else m).contiguous()
        if m.dim() != 3 or m.shape[1] < 16 or m.shape[2] < 1:
            raise ValueError("Denoiser.denoise_spectrogram: magnitudes must be (F, T) or (N, F, T) with F >= 16, T >= 1")
        n, f, t = m.shape
        k, w = self.plan(t)
        if k == 1 and w == t:
            x = m[:, None]
        else:                                               # cut the windows (copies only; frames past the end stay zero)
            x = torch.zeros((n, k, f, w), dtype=torch.float32, device=m.device)
            stride = self.window_frames - self.overlap_frames
            for i in range(k):
                part = m[:, :, i * stride:i * stride + w]
                x[:, i, :, :part.shape[2]] = part
            x = x.view(n * k, 1, f, w)
        out = self.stitch(self.network(x), n, t, clamp=False)
        out = out[0] if single else out
        return out.cpu().numpy() if is_np else out

    def denoise_file(self, src, dst, subtype: str = "PCM_16"):
        """``read_wav(src)`` -> ``denoise`` at the file's rate, every channel a clip -> ``write_wav(dst)``.  Returns
        ``(n_samples, sample_rate)``."""
        audio, rate = read_wav(src, mono=False)              # (L, channels)
        out = self.denoise(np.ascontiguousarray(audio.T), sr=rate)
        write_wav(dst, np.ascontiguousarray(out.T), rate, subtype)
        return int(audio.shape[0]), int(rate)


def _load_model(path, dtype, device):
    from .model import UNet
    state = torch.load(path, map_location="cpu")
    if isinstance(state, dict) and "state_dict" in state and not any(k.endswith(".weight") for k in state):
        state = state["state_dict"]
    model = UNet(1, 1)
    model.load_state_dict(state, strict=True)
    return model.to(device).eval().set_compute_dtype(dtype)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.denoise", description="Denoise a wav file or a folder of wav files.")
    ap.add_argument("--model", required=True, help="checkpoint: the state_dict of UNet(1, 1) (reference train.py:142)")
    ap.add_argument("src", metavar="IN", help="a wav file, or a folder of wav files")
    ap.add_argument("dst", metavar="OUT", help="the wav file to write, or the folder to write into")
    ap.add_argument("--phase", choices=("noisy", "griffin_lim"), default="noisy")
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--dtype", choices=("f32", "f16"), default="f32")
    ap.add_argument("--reference", metavar="CLEAN", default=None,
                    help="the clean wav of IN (or a folder with IN's file names): print one JSON line of metrics per file")
    args = ap.parse_args(argv)
    dev = _lib.staging_device()
    dn = Denoiser(_load_model(args.model, args.dtype, dev), window_frames=args.window, overlap_frames=args.overlap, phase=args.phase)
    return run_files(dn, args.src, args.dst, args.reference)


if __name__ == "__main__":
    raise SystemExit(main())
