"""Sample-rate conversion and SNR noise mixing on the device: the ingest of the training path.

``load_audio(path, sr=8000)`` has the call shape of the reference's ``librosa.load(path, sr=SAMPLE_RATE)``
(``/root/reference/code/create_train_dataset.py:204,217``): wav decode (:mod:`audiodenoiser_amd.wav`), channels averaged
to mono, then rate conversion by ``adn_resample``.  The filter is this project's own definition (``include/adn.h``): a
Kaiser-windowed-sinc polyphase low-pass (32 zero crossings, beta 12, roll-off 0.88), equal to
``scipy.signal.resample_poly(x, up, down, window=h / up)`` with those taps.  librosa resamples with soxr, whose taps
are not reproduced here: results are NOT bit-compatible with ``librosa.load`` and parity with it is unpinned.

``mix_snr`` is ``add_noise`` for the "white" / "urban" types (``create_train_dataset.py:147-157``) over a batch.

numpy in -> numpy out (staged on the device); a tensor on a ROCm device stays there; a CPU tensor raises.  There is no
CPU arithmetic path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .wav import read_wav

__all__ = ["resample_length", "resample", "prepare_resample", "mix_snr", "load_audio"]


def resample_length(length: int, orig_sr: int, target_sr: int) -> int:
    """``ceil(length * up / down)``: the number of samples ``resample`` returns (librosa's and scipy's rule)."""
    out = ctypes.c_long()
    _lib.check(_lib.load().adn_resample_length(int(length), int(orig_sr), int(target_sr), ctypes.byref(out)),
               "adn_resample_length")
    return int(out.value)


def prepare_resample(orig_sr: int, target_sr: int, device=None) -> None:
    """Build the coefficient table of a rate pair ahead of time (``adn_resample_prepare``): afterwards ``resample`` only
    enqueues on the current stream and can be recorded into a HIP graph."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _lib.check(_lib.load().adn_resample_prepare(dev.index if dev.index is not None else torch.cuda.current_device(),
                                                int(orig_sr), int(target_sr)), "adn_resample_prepare")


def _resample_device(audio: torch.Tensor, orig_sr: int, target_sr: int) -> torch.Tensor:
    if not audio.is_cuda:
        raise RuntimeError("resample: audio must live on a ROCm device (no CPU path)")
    if audio.dtype != torch.float32:
        raise TypeError("resample: expected float32 audio")
    single = audio.dim() == 1
    a = (audio[None] if single else audio).contiguous()
    if a.dim() != 2:
        raise ValueError("resample: audio must be (L,) or (n_clips, L)")
    n_clips, length = a.shape
    if n_clips < 1:
        raise ValueError("resample: empty batch")
    m = resample_length(length, orig_sr, target_sr)
    out = torch.empty((n_clips, m), dtype=torch.float32, device=a.device)
    stream = torch.cuda.current_stream(a.device).cuda_stream
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().adn_resample(a.data_ptr(), n_clips, length, int(orig_sr), int(target_sr), out.data_ptr(), stream),
                   "adn_resample")
    return out[0] if single else out


def resample(audio, orig_sr: int, target_sr: int, device=None):
    """``audio`` (L,) or (n_clips, L) float32 at ``orig_sr`` -> the same clips at ``target_sr``, (..., ceil(L * up / down))."""
    if isinstance(audio, torch.Tensor):
        return _resample_device(audio, orig_sr, target_sr)
    a = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(device or _lib.staging_device())
    return _resample_device(a, orig_sr, target_sr).cpu().numpy()


def _mix_device(clean: torch.Tensor, noise: torch.Tensor, snr_db: float) -> torch.Tensor:
    if not (clean.is_cuda and noise.is_cuda):
        raise RuntimeError("mix_snr: clean and noise must live on a ROCm device (no CPU path)")
    if clean.dtype != torch.float32 or noise.dtype != torch.float32:
        raise TypeError("mix_snr: expected float32 audio")
    if clean.shape != noise.shape or clean.dim() not in (1, 2) or clean.device != noise.device:
        raise ValueError("mix_snr: clean and noise must have one shape, (L,) or (n_clips, L), on one device")
    single = clean.dim() == 1
    c = (clean[None] if single else clean).contiguous()
    n = (noise[None] if single else noise).contiguous()
    n_clips, length = c.shape
    lib = _lib.load()
    need = ctypes.c_size_t()
    _lib.check(lib.adn_mix_snr_workspace_bytes(n_clips, length, ctypes.byref(need)), "adn_mix_snr_workspace_bytes")
    ws = torch.empty((max(1, (need.value + 3) // 4),), dtype=torch.float32, device=c.device)
    out = torch.empty_like(c)
    stream = torch.cuda.current_stream(c.device).cuda_stream
    with torch.cuda.device(c.device):
        _lib.check(lib.adn_mix_snr(c.data_ptr(), n.data_ptr(), n_clips, length, float(snr_db), ws.data_ptr(), ws.numel() * 4,
                                   out.data_ptr(), stream), "adn_mix_snr")
    return out[0] if single else out


def mix_snr(clean, noise, snr_db: float = 8.0, device=None):
    """Per clip ``clip(clean + s * noise, -1, 1)`` with ``s`` scaling the noise to ``snr_db`` below the clean RMS."""
    if isinstance(clean, torch.Tensor) or isinstance(noise, torch.Tensor):
        if not (isinstance(clean, torch.Tensor) and isinstance(noise, torch.Tensor)):
            raise TypeError("mix_snr: clean and noise must both be tensors or both be arrays")
        return _mix_device(clean, noise, snr_db)
    dev = device or _lib.staging_device()
    c = torch.from_numpy(np.ascontiguousarray(clean, dtype=np.float32)).to(dev)
    n = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float32)).to(dev)
    return _mix_device(c, n, snr_db).cpu().numpy()


def load_audio(path, sr=None, mono: bool = True, device=None):
    """``librosa.load(path, sr=sr, mono=mono)``'s call shape -> ``(float32 ndarray, rate)``.  ``sr=None`` returns the file as
    it is; otherwise the audio is resampled on the device when ``sr`` differs from the file's rate.  ``mono=False`` returns
    ``(channels, L)`` as librosa does."""
    audio, rate = read_wav(path, mono=mono)
    if not mono:
        audio = np.ascontiguousarray(audio.T)
    if sr is None or int(sr) == rate:
        return audio, rate
    return resample(audio, rate, int(sr), device=device), int(sr)
