"""Spectral baseline denoiser: noise tracking + Wiener gain, no checkpoint.

    from audiodenoiser_amd.baseline import SpectralDenoiser, SpectralParams, spectral_gain
    dn = SpectralDenoiser()                            # no model: the current ROCm device, 8 kHz, n_fft 512, hop 128
    clean = dn.denoise(noisy, sr=44100)                # (L,) or (N, L); numpy -> numpy, device tensor -> device tensor
    dn.denoise_file("noisy.wav", "clean.wav")

    sd = StreamSpectralDenoiser()                      # the same operator on audio that is still arriving: a StreamDenoiser
    out = sd.push(block); out = sd.flush()             # without a network, 112 ms behind the feed at the defaults
    pool = SpectralStreamPool(max_streams=64)          # a StreamPool of such feeds: open / push / close / step

    python -m audiodenoiser_amd.baseline IN OUT [--reference CLEAN] [--bias 1.0] [--gain-floor 0.1]
    python -m audiodenoiser_amd.baseline IN OUT --live [--chunk 1024] [--block 4] [--reference CLEAN]

The operator is DEFINED in ``include/adn.h`` ("baseline"; float64 restatement: ``tests/baseline_ref.py``) and is unpinned against
any package: Doblinger's continuous minimum tracking for the noise power, the decision-directed a-priori SNR of Ephraim and Malah,
a Wiener gain with a floor.  It is causal, carries three floats per bin and needs no weights, which makes it the figure a trained
network has to beat in the ``--reference`` report.  ``SpectralDenoiser`` is ``Denoiser`` with the network replaced:

1. ``adn_stft_complex``: the centred complex STFT, ``T = 1 + L // hop`` frames;
2. ``adn_spectral_gain`` (``csrc/baseline_kernels.hip``) into a zeroed ``(n, 1, F, max(T, 16))`` buffer;
3. ``adn_denoise_resynth`` with ``window = max(T, 16)`` and ``overlap = 0``: one window per clip, the plan's exact pass-through
   case ("a frame covered by one window is y itself, bit for bit"), the noisy input's own phase, all ``L`` samples back.

``denoise``, ``denoise_file``, the rate handling and the every-channel-a-clip rule are ``Denoiser``'s, unchanged.

Streaming: ``adn_spectral_gain_windows`` (``spectral_gain_windows``) is the same operator in its magnitude form (``adn.h``, "The
magnitude form": ``X = m + 0i`` through the same one step) on the bin-major windows the stream kernels write and read, in place
on the ``block_frames`` columns a step keeps, with the three floats per bin carried in a state the caller owns.
``StreamSpectralDenoiser`` is ``StreamDenoiser`` and ``SpectralStreamPool`` is ``StreamPool`` with that call in the network's
place; everything those classes claim about cuts into pushes, neighbours, rates and slot reuse holds bit for bit, since the
gain is a function of a row's own frames in order.  A stream's result is NOT bit-equal to ``SpectralDenoiser``'s on the same
audio: the stream hands over ``|X| = sqrtf(p)`` and ``sqrtf(p)^2 != p`` in the last bits (the float64 restatements agree to 4e-16).

What is NOT here: Griffin-Lim phase, log-MMSE gains, any tuning of the defaults by ear (``block_frames = 4`` included).  There is
no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os

import torch

from . import _lib
from .denoise import Denoiser, _report, _stream
from .griffin_lim import stft_complex
from .stream import PoolBook, StreamDenoiser, StreamPool, _check_stream_args

__all__ = ["SpectralParams", "spectral_gain", "SpectralDenoiser", "spectral_gain_windows", "StreamSpectralDenoiser",
           "SpectralStreamPool"]

SPECTRAL_MAX_ROWS = 256      # ADN_SPECTRAL_MAX_ROWS of include/adn.h: the rows of one call that names its slots


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


def spectral_gain_windows(windows: torch.Tensor, state: torch.Tensor, col0: int, n_cols: int, n_steps: int = 1,
                          params: SpectralParams = None, rows=None, out: torch.Tensor = None) -> torch.Tensor:
    """``adn_spectral_gain_windows`` on the current stream.  ``windows``: contiguous float32 ``(n_rows * n_steps, 1, F, W)`` on a
    ROCm device, a row's steps consecutive (what ``StreamDenoiser.analyze`` / ``StreamPool.analyze`` return).  Columns
    ``[col0, col0 + n_cols)`` of every step are a row's frames in order; their gained magnitudes go to the same columns of ``out``
    and nothing else is written: ``out=None`` allocates a buffer (its other columns hold nothing), ``out=windows`` runs in place.
    ``state``: contiguous float32 ``(n_slots, 3, F)`` there, updated IN PLACE (rows ``P``, ``Pmin``, ``S``; a negative ``P``
    starts fresh).  ``rows=None``: row i uses slot i; otherwise ``(slot, fresh)`` per row, at most 256, no slot twice, and a row
    with ``fresh`` true starts fresh whatever its slot holds.  Returns ``out``."""
    if (not isinstance(windows, torch.Tensor) or not windows.is_cuda or windows.dtype != torch.float32 or windows.dim() != 4
            or windows.shape[1] != 1 or not windows.is_contiguous()):
        raise ValueError("spectral_gain_windows: expected a contiguous (n_rows * n_steps, 1, n_bins, window) float32 tensor on a ROCm device")
    nw, _, f, w = windows.shape
    if not (isinstance(n_steps, int) and n_steps >= 1) or nw < 1 or nw % n_steps or f < 1 or w < 1:
        raise ValueError("spectral_gain_windows: need n_steps >= 1 dividing the number of windows, and at least one row, bin and frame")
    if not (isinstance(col0, int) and isinstance(n_cols, int) and col0 >= 0 and n_cols >= 1 and col0 + n_cols <= w):
        raise ValueError("spectral_gain_windows: need col0 >= 0, n_cols >= 1 and col0 + n_cols <= window")
    n_rows, dev = nw // n_steps, windows.device
    if (not isinstance(state, torch.Tensor) or not state.is_cuda or state.device != dev or state.dtype != torch.float32
            or state.dim() != 3 or tuple(state.shape[1:]) != (3, f) or state.shape[0] < 1 or not state.is_contiguous()):
        raise ValueError("spectral_gain_windows: state must be a contiguous (n_slots, 3, n_bins) float32 tensor on windows' device")
    if out is None:
        out = torch.empty((nw, 1, f, w), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float32
          or out.shape != windows.shape or not out.is_contiguous()):
        raise ValueError("spectral_gain_windows: out must be a contiguous float32 tensor of windows' shape on its device")
    table = None
    if rows is not None:
        if len(rows) != n_rows:
            raise ValueError("spectral_gain_windows: rows must name a (slot, fresh) for each of the n_rows rows")
        # the table as the 2 n_rows ints it is (adn_spectral_row = {int slot; int fresh;}): a tick builds one per call
        table = (ctypes.c_int * (2 * n_rows))(*[v for slot, fresh in rows for v in (int(slot), 1 if fresh else 0)])
    p = ctypes.byref(params.to_struct()) if params is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().adn_spectral_gain_windows(windows.data_ptr(), out.data_ptr(), n_rows, n_steps, f, w, col0, n_cols, p,
                                                         state.data_ptr(), int(state.shape[0]), table, _stream(dev)),
                   "adn_spectral_gain_windows")
    return out


def _spectral_device(who, device, params):
    if params is not None and not isinstance(params, SpectralParams):
        raise TypeError(f"{who}: params must be a SpectralParams")
    dev = _lib.staging_device() if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the device must be a ROCm device; there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class StreamSpectralDenoiser(StreamDenoiser):
    """``StreamDenoiser`` with the spectral baseline in the network's place: no model, noisy phase only, the same surface --
    ``push``, ``flush``, ``reset``, ``received``, ``emitted``, ``latency_samples``, ``analyze``, ``emit``, ``input_rate``.

    The operator is causal, so ``lookahead_frames`` is 0 and ``window_frames = max(16, block_frames)`` is only the carrier the
    stream geometry needs: each run of steps calls ``adn_spectral_gain_windows`` in place on the analysed windows, on the
    ``block_frames`` columns ``adn_stream_emit`` reads, and the gain's three floats per bin live in ``(n_streams, 3, F)`` on the
    device (``reset`` fills it with the fresh-start sentinel).  ``block_frames = 4`` gives a latency of 896 samples, 112 ms at
    8 kHz; it is a design value and has not been tuned by ear."""

    def __init__(self, device=None, n_streams: int = 1, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128,
                 block_frames: int = 4, params: SpectralParams = None, input_rate=None):
        window = max(16, block_frames) if isinstance(block_frames, int) else 16
        _check_stream_args("StreamSpectralDenoiser", n_streams, sample_rate, n_fft, hop_length, window, block_frames, 0, 64, input_rate)
        dev = _spectral_device("StreamSpectralDenoiser", device, params)
        self.model = None
        self.params = SpectralParams() if params is None else params
        self._gain_state = torch.empty((n_streams, 3, n_fft // 2 + 1), dtype=torch.float32, device=dev)
        self._setup(dev, n_streams, sample_rate, n_fft, hop_length, window, block_frames, 0, 64, input_rate)

    def reset(self):
        """Forget the running stream, the noise estimate included: the object is ready for a new one."""
        super().reset()
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("StreamSpectralDenoiser: there is no network; the gain runs between analyze and emit (spectral_gain_windows)")

    def _net(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        w, b = self.window_frames, self.block_frames
        return spectral_gain_windows(x, self._gain_state, w - b, b, n_steps, self.params, None, x)


class SpectralStreamPool(StreamPool):
    """``StreamPool`` with the spectral baseline in the network's place: ``open``, ``push``, ``push_many``, ``close``, ``step``,
    ``drain``, ``room``, ``received`` and the rates are the parent's.  A tick calls ``adn_spectral_gain_windows`` once per group of
    up to 256 rows, in place on the analysed windows, with ``rows = (slot, step == 0)``: a stream's first step starts its slot's
    noise estimate afresh, so a slot is reusable without a reset here as well.  Each stream is, bit for bit, what a solo
    ``StreamSpectralDenoiser`` (at its ``input_rate``) returns for the same samples.  ``block_frames = 4``: as there."""

    def __init__(self, device=None, max_streams: int = 64, backlog_steps: int = 4, sample_rate: int = 8000, n_fft: int = 512,
                 hop_length: int = 128, block_frames: int = 4, params: SpectralParams = None, input_rates=None):
        window = max(16, block_frames) if isinstance(block_frames, int) else 16
        self.book = PoolBook(max_streams, backlog_steps, n_fft, hop_length, window, block_frames, 0, input_rates, sample_rate)
        dev = _spectral_device("SpectralStreamPool", device, params)
        self.model, self.batch_windows = None, SPECTRAL_MAX_ROWS
        self.params = SpectralParams() if params is None else params
        self._gain_state = torch.empty((max_streams, 3, n_fft // 2 + 1), dtype=torch.float32, device=dev)
        self._setup(dev)

    def reset(self):
        """Forget every stream, the noise estimates included: all slots are free."""
        super().reset()
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("SpectralStreamPool: there is no network; the gain runs between analyze and emit (spectral_gain_windows)")

    def _net(self, x: torch.Tensor, rows) -> torch.Tensor:
        w, b = self.book.window_frames, self.book.block_frames
        for i in range(0, len(rows), SPECTRAL_MAX_ROWS):
            part = x[i:i + SPECTRAL_MAX_ROWS]
            spectral_gain_windows(part, self._gain_state, w - b, b, 1, self.params,
                                  [(slot, step == 0) for slot, step, _ in rows[i:i + SPECTRAL_MAX_ROWS]], part)
        return x


def _live(args, params) -> int:
    """``--live``: the file pushed through ``StreamSpectralDenoiser`` at its own rate, ``--chunk`` samples at a time."""
    import numpy as np

    from .wav import read_wav, write_wav
    audio, rate = read_wav(args.src, mono=False)             # (L, channels): every channel is a stream
    dev = _lib.staging_device()
    x = torch.from_numpy(np.ascontiguousarray(audio.T, dtype=np.float32)).to(dev)
    sd = StreamSpectralDenoiser(dev, n_streams=x.shape[0], block_frames=args.block, params=params, input_rate=int(rate))
    outs = [sd.push(x[:, i:i + args.chunk]) for i in range(0, x.shape[1], args.chunk)]
    latency = sd.latency_input_samples
    outs.append(sd.flush())
    out = torch.cat(outs, dim=1)
    write_wav(args.dst, np.ascontiguousarray(out.cpu().numpy().T), rate)
    print(f"{args.src} -> {args.dst}: {x.shape[1]} samples at {rate} Hz in pushes of {args.chunk} at its own rate, "
          f"latency {latency} samples")
    if args.reference is not None:
        print(_report(args.src, args.dst, args.reference))
    return 0


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
    ap.add_argument("--live", action="store_true",
                    help="push the file (not a folder) through the streaming form at its own rate, as a live feed arrives")
    ap.add_argument("--chunk", type=int, default=1024, help="with --live: samples per push, at the file's rate")
    ap.add_argument("--block", type=int, default=4, help="with --live: frames per step (latency (block - 1) hop + n_fft samples)")
    args = ap.parse_args(argv)
    params = SpectralParams(bias=args.bias, gain_floor=args.gain_floor)
    if args.live:
        if args.chunk < 1 or args.block < 1:
            ap.error("--chunk and --block must be >= 1")
        if os.path.isdir(args.src):
            ap.error("--live takes one wav file")
        return _live(args, params)
    dn = SpectralDenoiser(params=params)
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
