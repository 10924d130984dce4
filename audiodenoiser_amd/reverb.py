"""The "reverb" noise type of the reference's train-set builder on the device: ``adn_reverb``.

The reference renders it with Pedalboard (``Reverb(room_size=0.9, damping=0.9, wet_level=0.33)`` over every 2 s chunk, then
``np.clip``: ``/root/reference/code/create_train_dataset.py:87-102,116-121``).  Pedalboard's ``Reverb`` wraps JUCE's, which is
Freeverb (public domain): eight parallel low-pass-feedback combs, four all-pass filters in series, an input gain and a wet /
dry mix.  The effect here is this project's own definition of it (``include/adn.h``; float64 restatement in
``tests/reverb_ref.py``): mono, constant parameters, zero state at each clip's first sample.  Its constants have NOT been
checked against JUCE or Pedalboard, and parity with ``pedalboard.Reverb`` is unpinned; JUCE's parameter smoothing, denormal
nudge, freeze mode and stereo pair are not reproduced.

Calling conventions as :func:`audiodenoiser_amd.resample.mix_snr`: numpy in -> numpy out (staged on the device); a tensor on a
ROCm device stays there; a CPU tensor raises.  There is no CPU arithmetic path.

``python -m audiodenoiser_amd.reverb in.wav out.wav [--room-size 0.9 ...]`` renders a file so that the effect can be listened
to (the reference's debug wavs, ``create_train_dataset.py:233-239``).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib

__all__ = ["ReverbSettings", "delay_lengths", "reverb", "MIN_SAMPLE_RATE", "MAX_SAMPLE_RATE"]

COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_TUNING = (556, 441, 341, 225)
MIN_SAMPLE_RATE, MAX_SAMPLE_RATE = 2000, 128000     # adn_reverb's range: the delay lines of a clip are held in LDS


@dataclasses.dataclass(frozen=True)
class ReverbSettings:
    """The five parameters of the effect, each in [0, 1].  The defaults are the reference's call plus Pedalboard's own defaults
    for the two it leaves out."""
    room_size: float = 0.9
    damping: float = 0.9
    wet_level: float = 0.33
    dry_level: float = 0.4
    width: float = 1.0

    def __post_init__(self):
        for name, value in dataclasses.asdict(self).items():
            if not 0.0 <= float(value) <= 1.0:
                raise ValueError(f"ReverbSettings.{name} must be in [0, 1], got {value!r}")


def delay_lengths(sample_rate: int):
    """``(comb delays, all-pass delays)`` in samples at ``sample_rate``: ``(sample_rate * tuning) // 44100``."""
    sr = int(sample_rate)
    return [sr * t // 44100 for t in COMB_TUNING], [sr * t // 44100 for t in ALLPASS_TUNING]


def _reverb_device(audio: torch.Tensor, sample_rate: int, s: ReverbSettings, clip: bool, out=None) -> torch.Tensor:
    if not audio.is_cuda:
        raise RuntimeError("reverb: audio must live on a ROCm device (no CPU path)")
    if audio.dtype != torch.float32:
        raise TypeError("reverb: expected float32 audio")
    if audio.dim() not in (1, 2):
        raise ValueError("reverb: audio must be (L,) or (n_clips, L)")
    single = audio.dim() == 1
    a = (audio[None] if single else audio).contiguous()
    n_clips, length = a.shape
    if n_clips < 1:
        raise ValueError("reverb: empty batch")
    y = torch.empty_like(a) if out is None else out.view(a.shape)
    stream = torch.cuda.current_stream(a.device).cuda_stream
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().adn_reverb(a.data_ptr(), n_clips, length, int(sample_rate), s.room_size, s.damping, s.wet_level,
                                          s.dry_level, s.width, int(bool(clip)), y.data_ptr(), stream), "adn_reverb")
    return y[0] if single else y


def reverb(audio, sample_rate: int, room_size: float = 0.9, damping: float = 0.9, wet_level: float = 0.33,
           dry_level: float = 0.4, width: float = 1.0, clip: bool = True, device=None):
    """``audio`` (L,) or (n_clips, L) float32 at ``sample_rate`` -> the reverberated clips, same shape and kind; each clip is
    rendered on its own from zero state.  ``clip=True`` limits the result to [-1, 1] as ``add_noise`` does."""
    s = ReverbSettings(room_size, damping, wet_level, dry_level, width)
    if isinstance(audio, torch.Tensor):
        return _reverb_device(audio, sample_rate, s, clip)
    a = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(device or _lib.staging_device())
    return _reverb_device(a, sample_rate, s, clip, out=a).cpu().numpy()          # (the staged copy is rendered in place)


def main(argv=None) -> int:
    import argparse

    from .wav import read_wav, write_wav
    d = ReverbSettings()
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.reverb",
                                 description="Render a wav file through this project's Freeverb (mono) on the GPU.")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--room-size", type=float, default=d.room_size)
    ap.add_argument("--damping", type=float, default=d.damping)
    ap.add_argument("--wet-level", type=float, default=d.wet_level)
    ap.add_argument("--dry-level", type=float, default=d.dry_level)
    ap.add_argument("--width", type=float, default=d.width)
    ap.add_argument("--no-clip", action="store_true", help="do not limit the result to [-1, 1]")
    ap.add_argument("--float", action="store_true", help="write 32-bit float samples instead of 16-bit PCM")
    args = ap.parse_args(argv)
    audio, rate = read_wav(args.input, mono=True)
    out = reverb(audio, rate, args.room_size, args.damping, args.wet_level, args.dry_level, args.width, clip=not args.no_clip)
    write_wav(args.output, out, rate, "FLOAT" if args.float else "PCM_16")
    print(f"{args.input}: {len(audio)} samples at {rate} Hz -> {args.output}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
