"""Host code the class modules share (``denoise``, ``stream``, ``baseline``, ``dereverb``, ``resample``, ``metrics``): one
definition of each argument check, of how an input reaches the device, of the U-Net loop and of the command lines' file loops.

Every check takes ``who``, the name its message starts with.  Nothing here is public and nothing here launches a kernel of its
own except ``unet_windows``; the functional modules (``stft``, ``loss``, ``reverb``, ``griffin_lim``, ``data_loader``) keep their
own refusals, which use other sentences.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib


def current_stream(dev):
    """The raw handle of torch's current stream on ``dev``: what every ``adn_*`` launcher takes as its last argument."""
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------------------------------------------------- argument checks
def check_stft_plan(who, n_fft, hop_length, sample_rate) -> None:
    """The transform every class is built on: the sizes the library's FFT serves, a hop the inverse transform can divide by."""
    if not (isinstance(n_fft, int) and 64 <= n_fft <= 4096 and n_fft & (n_fft - 1) == 0):
        raise ValueError(f"{who}: n_fft must be a power of two in [64, 4096]")
    if not (isinstance(hop_length, int) and 1 <= hop_length <= n_fft // 4):
        raise ValueError(f"{who}: need 1 <= hop_length <= n_fft / 4 (the inverse transform of the whole input length divides by a "
                         "window sum-of-squares that falls to 2e-8 at n_fft / 2)")
    if not (isinstance(sample_rate, int) and sample_rate >= 1):
        raise ValueError(f"{who}: sample_rate must be >= 1")


def model_device(who, model):
    """``model`` is a ``UNet(1, 1)`` in eval mode on a ROCm device -> that device."""
    from .model import UNet
    if not isinstance(model, UNet) or model.in_channels != 1 or model.num_classes != 1:
        raise ValueError(f"{who}: model must be an audiodenoiser_amd.model.UNet(1, 1)")
    if model.training:
        raise RuntimeError(f"{who}: the model is in train mode; call .eval() (the HIP forward is the eval forward)")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the model must live on a ROCm device (model.to('cuda')); there is no CPU path")
    return dev


def rocm_device(who, device):
    """The device of a class without a model: ``device``, or the staging device for None, always with an index."""
    dev = _lib.staging_device() if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the device must be a ROCm device; there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def stage(who, audio, device, what: str = "audio"):
    """-> ``(tensor, was_numpy)``.  numpy (anything that is no tensor) becomes a float32 tensor and is copied to ``device`` --
    or stays on the host with ``device=None``, for a caller that has more to join before one copy; a tensor is taken as it is
    unless it lives on the CPU or is not float32.  Shapes are the caller's business."""
    if not isinstance(audio, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
        return (x if device is None else x.to(device)), True
    if not audio.is_cuda:
        raise RuntimeError(f"{who}: a tensor must live on a ROCm device (no CPU path); pass numpy to have it staged")
    if audio.dtype != torch.float32:
        raise TypeError(f"{who}: expected float32 {what}")
    return audio, False


# ---------------------------------------------------------------------------------------------------------------- the network
def unet_windows(who, model, x: torch.Tensor, batch_windows: int) -> torch.Tensor:
    """The U-Net over ``batch_windows`` windows of ``x`` ``(n_windows, 1, F, W)`` at a time, into slices of one output buffer."""
    x = x.contiguous()
    nw, _, f, w = x.shape
    dev = x.device
    y = torch.empty_like(x)
    if model.training:
        raise RuntimeError(f"{who}: the model is in train mode; call .eval()")
    L = _lib.load()
    handle = model._ensure_handle(dev)
    per = f * w * 4
    with torch.cuda.device(dev):
        for i in range(0, nw, batch_windows):
            n = min(batch_windows, nw - i)
            ws = model._workspace_for(n, f, w, dev)
            _lib.check(L.adn_unet_forward(handle, x.data_ptr() + i * per, y.data_ptr() + i * per, n, f, w, ws.data_ptr(),
                                          ws.numel(), current_stream(dev)), "adn_unet_forward")
    return y


# ---------------------------------------------------------------------------------------------------------------- command lines
def report(src, dst, ref_path, per_channel: bool = False) -> str:
    """One JSON line: the four metrics of the noisy input and of the denoised output against the clean reference, at the
    file's rate, each pair cut to the shorter of the two (mono mixes).  ``per_channel`` adds ``si_sdr_per_channel`` to both: the
    SI-SDR of every channel of the file against the (mono) reference."""
    import json
    from .metrics import evaluate
    from .wav import read_wav
    ref, ref_rate = read_wav(ref_path, mono=True)
    row = {"file": src, "reference": ref_path, "sample_rate": int(ref_rate)}
    for key, path in (("noisy", src), ("denoised", dst)):
        audio, rate = read_wav(path, mono=True)
        if rate != ref_rate:
            raise ValueError(f"--reference: {ref_path} is at {ref_rate} Hz, {path} at {rate} Hz")
        n = min(len(audio), len(ref))
        m = evaluate(audio[:n], ref[:n], sr=int(rate))
        row[key] = {k: float(v[0]) for k, v in m.items()}
        if per_channel:
            chans = np.ascontiguousarray(read_wav(path, mono=False)[0].T[:, :n], dtype=np.float32)
            each = evaluate(chans, np.broadcast_to(ref[:n], chans.shape).copy(), sr=int(rate))["si_sdr"]
            row[key]["si_sdr_per_channel"] = [float(v) for v in each]
    return json.dumps(row)


def wav_jobs(src, dst):
    """``(in, out)`` per file: a folder gives its wav files in name order into the folder ``dst`` (made here), a file itself."""
    if not os.path.isdir(src):
        return [(src, dst)]
    os.makedirs(dst, exist_ok=True)
    return [(os.path.join(src, f), os.path.join(dst, f)) for f in sorted(os.listdir(src)) if f.lower().endswith(".wav")]


def run_files(dn, src, dst, reference) -> int:
    """``dn.denoise_file`` over ``wav_jobs``, a line per file; ``reference`` (a clean wav, or a folder with the inputs' names)
    adds the ``report`` line after each."""
    for s, d in wav_jobs(src, dst):
        n, rate = dn.denoise_file(s, d)
        print(f"{s} -> {d}: {n} samples at {rate} Hz")
        if reference is not None:
            print(report(s, d, os.path.join(reference, os.path.basename(s)) if os.path.isdir(reference) else reference))
    return 0


def run_live(make, src, dst, chunk, reference, per_channel: bool = False) -> int:
    """The wav file ``src`` pushed ``chunk`` samples at a time, at its own rate, through the stream object that
    ``make(device, n_streams, rate)`` returns -- every channel a stream -- and written to ``dst``.  An object that returns one
    row of samples per push (``StreamBeamformer`` on one recording) gives a mono file."""
    from .wav import read_wav, write_wav
    audio, rate = read_wav(src, mono=False)                  # (L, channels)
    dev = _lib.staging_device()
    x = torch.from_numpy(np.ascontiguousarray(audio.T, dtype=np.float32)).to(dev)
    sd = make(dev, x.shape[0], int(rate))
    outs = [sd.push(x[:, i:i + chunk]) for i in range(0, x.shape[1], chunk)]
    latency = sd.latency_input_samples
    outs.append(sd.flush())
    out = torch.cat(outs, dim=-1)
    write_wav(dst, np.ascontiguousarray(out.cpu().numpy().T), rate)
    print(f"{src} -> {dst}: {x.shape[1]} samples at {rate} Hz in pushes of {chunk} at its own rate, latency {latency} samples")
    if reference is not None:
        print(report(src, dst, reference, per_channel))
    return 0
