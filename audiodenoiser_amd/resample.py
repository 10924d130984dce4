"""Sample-rate conversion and SNR noise mixing on the device: the ingest of the training path.

``load_audio(path, sr=8000)`` has the call shape of the reference's ``librosa.load(path, sr=SAMPLE_RATE)``
(``/root/reference/code/create_train_dataset.py:204,217``): wav decode (:mod:`audiodenoiser_amd.wav`), channels averaged
to mono, then rate conversion by ``adn_resample``.  The filter is this project's own definition (``include/adn.h``): a
Kaiser-windowed-sinc polyphase low-pass (32 zero crossings, beta 12, roll-off 0.88), equal to
``scipy.signal.resample_poly(x, up, down, window=h / up)`` with those taps.  librosa resamples with soxr, whose taps
are not reproduced here: results are NOT bit-compatible with ``librosa.load`` and parity with it is unpinned.

``mix_snr`` is ``add_noise`` for the "white" / "urban" types (``create_train_dataset.py:147-157``) over a batch.

``StreamResampler`` is ``resample`` for audio that is still arriving (``adn_resample_stream``; definition: ``include/adn.h``,
"resample stream"): ``push`` returns the samples that have become final, ``flush`` the rest, and their concatenation is, bit for
bit, ``resample`` of the finished signal however it was cut into pushes.  The filter's history lives on the device between calls.

numpy in -> numpy out (staged on the device); a tensor on a ROCm device stays there; a CPU tensor raises.  There is no
CPU arithmetic path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._host import current_stream, stage
from .wav import read_wav

__all__ = ["resample_length", "resample", "prepare_resample", "mix_snr", "load_audio", "StreamResampler", "resample_stream_plan"]


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
    stream = current_stream(a.device)
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


def resample_stream_plan(received: int, orig_sr: int, target_sr: int, final: bool = False):
    """``(emitted, history, latency)`` of a stream that has received ``received`` samples at ``orig_sr`` (``adn_resample_stream_plan``,
    host only): outputs that are final (all of them with ``final``), input samples carried between calls, and the latency in input
    samples."""
    e, h, lat = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.load().adn_resample_stream_plan(int(orig_sr), int(target_sr), int(received), 1 if final else 0, ctypes.byref(e),
                                                    ctypes.byref(h), ctypes.byref(lat)), "adn_resample_stream_plan")
    return int(e.value), int(h.value), int(lat.value)


class StreamResampler:
    """``n_streams`` streams at ``orig_sr`` -> the same streams at ``target_sr``, block by block; all streams advance in lockstep."""

    def __init__(self, orig_sr: int, target_sr: int, n_streams: int = 1, device=None):
        if not (isinstance(orig_sr, int) and isinstance(target_sr, int) and orig_sr >= 1 and target_sr >= 1):
            raise ValueError("StreamResampler: rates must be integers >= 1")
        if not (isinstance(n_streams, int) and n_streams >= 1):
            raise ValueError("StreamResampler: n_streams must be >= 1")
        self.orig_sr, self.target_sr, self.n_streams = orig_sr, target_sr, n_streams
        need = ctypes.c_size_t()
        _lib.check(_lib.load().adn_resample_stream_state_bytes(n_streams, orig_sr, target_sr, ctypes.byref(need)),
                   "adn_resample_stream_state_bytes")
        self._state_bytes = need.value
        self._device = torch.device(device) if device is not None else None
        self._state = None                 # allocated with the first block: on its device, or the staging device for numpy
        self._numpy = True
        self.reset()

    @property
    def latency_samples(self) -> int:
        """Input samples that at worst lie between a sample's arrival and the output it feeds: ``ceil(half / up)``."""
        return resample_stream_plan(0, self.orig_sr, self.target_sr)[2]

    @property
    def received(self) -> int:
        return self._received

    @property
    def emitted(self) -> int:
        return self._emitted

    def reset(self):
        """Forget the running stream.  Call 0 of a stream reads no state, so nothing is enqueued."""
        self._received = self._emitted = self._calls = 0

    def _to_device(self, block) -> torch.Tensor:
        x, self._numpy = stage("StreamResampler.push", block, None)
        if self._device is None:               # the first block names the device: its own, or the staging device for numpy
            self._device = _lib.staging_device() if self._numpy else x.device
        x = x.to(self._device)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[0] != self.n_streams:
            raise ValueError(f"StreamResampler.push: audio must be (m,) for one stream or (n_streams, m) = ({self.n_streams}, m)")
        return x if x.stride(1) == 1 or x.shape[1] == 0 else x.contiguous()

    def _call(self, x, final: bool) -> torch.Tensor:
        """One ``adn_resample_stream`` call on the device tensor ``x`` (n_streams, n_new), or the last one with ``x`` None."""
        dev = self._device
        n_new = 0 if x is None else x.shape[1]
        total = resample_stream_plan(self._received + n_new, self.orig_sr, self.target_sr, final)[0]
        out = torch.empty((self.n_streams, total - self._emitted), dtype=torch.float32, device=dev)
        if self._state is None:
            self._state = torch.empty(max(self._state_bytes, 8), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().adn_resample_stream(self._state.data_ptr(), self._state_bytes, x.data_ptr() if n_new else None,
                                                       x.stride(0) if n_new else 0, self.n_streams, self._calls, self._received, n_new,
                                                       1 if final else 0, self.orig_sr, self.target_sr,
                                                       out.data_ptr() if out.shape[1] else None, out.shape[1],
                                                       current_stream(dev)), "adn_resample_stream")
        self._received += n_new
        self._emitted = total
        self._calls += 1
        return out

    def _empty(self):
        out = torch.empty((self.n_streams, 0), dtype=torch.float32, device=self._device)
        return out.cpu().numpy() if self._numpy else out

    def push(self, block):
        """``block``: the next ``m >= 0`` samples of every stream at ``orig_sr``, ``(m,)`` for one stream or ``(n_streams, m)``, float32.
        Returns ``(n_streams, emitted(received) - emitted(before))`` samples at ``target_sr``: those no later input can change.  One
        kernel launch on the current stream; a push of nothing returns nothing and launches nothing."""
        x = self._to_device(block)
        if x.shape[1] == 0:
            return self._empty()
        if self._received + x.shape[1] >= 1 << 31:
            raise ValueError("StreamResampler.push: a stream holds fewer than 2^31 samples; flush() it before")
        out = self._call(x, False)
        return out.cpu().numpy() if self._numpy else out

    def flush(self):
        """The stream has ended: returns the rest, so that it has produced ``resample_length(received)`` samples in all, in the kind
        (numpy / tensor) of the last ``push``.  The object is then ready for a new stream."""
        if self._received == 0:
            out = self._empty() if self._device is not None else np.empty((self.n_streams, 0), dtype=np.float32)
        else:
            out = self._call(None, True)
            out = out.cpu().numpy() if self._numpy else out
        self.reset()
        return out


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
    stream = current_stream(c.device)
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
