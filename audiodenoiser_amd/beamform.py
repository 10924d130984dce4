"""Mask-driven MVDR beamformer: the C microphones of a recording to ONE enhanced channel, no checkpoint needed.

    from audiodenoiser_amd.beamform import Beamformer, MvdrParams, mvdr
    bf = Beamformer()                                  # no model: the current ROCm device, 8 kHz, n_fft 512, hop 128
    mono = bf.denoise(recording, sr=44100)             # (C, L) -> (L,); (N, C, L) -> (N, L); numpy -> numpy, tensor -> tensor
    bf.denoise_file("room4ch.wav", "out.wav")          # the wav's channels are one recording; a mono wav is written
    Beamformer(gain=True)                              # MVDR, then the Wiener gain of the spectral baseline on its result
    Beamformer(wpe=True, gain=True)                    # joint WPE, then MVDR, then the gain
    Beamformer(mask="model", model=unet)               # the mask from a trained U-Net: a neural beamformer
    y, mag = mvdr(spec, mag_estimate, channels)        # the operator on spectrograms

    python -m audiodenoiser_amd.beamform IN OUT [--reference CLEAN] [--ref-channel R] [--wpe] [--gain] [--model CKPT]
    python -m audiodenoiser_amd.beamform IN OUT --live [--chunk N] [--block B] [--forget A] [--refresh R] [--wpe] [--gain]

The operator is DEFINED in ``include/adn.h`` ("beamform"; float64 restatement: ``tests/beamform_ref.py``;
``csrc/beamform_kernels.hip``) and is unpinned against any package: the MVDR beamformer in Souden's form,
``w = Phi_n^-1 Phi_s u / tr(Phi_n^-1 Phi_s)``, per (recording, bin), with the two spatial covariance matrices weighted by a
time-frequency mask.  The mask comes from any per-channel magnitude estimate ``M`` of the wanted signal,
``m_t = clip(sum_c M^2 / sum_c |X|^2, rho, 1 - rho)``.  ``Beamformer`` is ``Denoiser`` with this in the network's place:

1. ``adn_stft_complex`` of every channel, ``T = 1 + L // hop`` frames;
2. with ``wpe=True`` ``adn_wpe_mc`` on the channels jointly (``wpe_params=None``: ``taps = 32 // C``);
3. the mask magnitudes: ``mask="spectral"`` runs ``adn_spectral_gain`` on every channel (``mask_params``); ``mask="model"`` runs the
   given U-Net on every channel through the window plan of ``Denoiser`` (windows, network, stitch, clamped at zero);
4. ``adn_mvdr``: one spectrogram per recording, and its magnitudes into a zeroed ``(n, 1, F, max(T, 16))`` buffer;
5. with ``gain=True`` ``adn_spectral_gain`` on that spectrogram writes the magnitudes instead (``gain_params``);
6. ``adn_denoise_resynth`` with one window per recording and the phase of the beamformer's output.

The live form is ``StreamBeamformer`` ("beamform stream" in ``include/adn.h``; float64 restatement:
``tests/beamform_stream_ref.py``; ``csrc/beamform_stream_kernels.hip``): the two covariances carried on the device with a forgetting
factor, updated once per frame, the same filter solved from them every ``refresh`` frames.  It is ``StreamDenoiser`` over
``n_streams = groups * C`` microphone feeds with, between ``analyze`` and ``emit`` and in place on the analysed windows,

1. with ``wpe=True`` ``adn_wpe_mc_stream`` (``wpe_params=None``: ``taps = 32 // C``);
2. ``adn_spectral_gain_windows`` on the kept columns of every channel: the mask's magnitudes (``mask_params``);
3. ``adn_mvdr_stream``: ``Y_t`` and ``|Y_t|`` over the group's first stream;
4. with ``gain=True`` the spectral gain again, with a state of its own (``gain_params``);

``adn_stream_emit`` then resynthesises every stream and the object keeps row ``g C`` of each group.  ``mvdr_online`` is the
recursion on spectrograms.

``BeamformStreamPool`` is the same chain for many recordings with independent timing (``adn_wpe_mc_stream_pool``,
``adn_mvdr_stream_pool``): a recording is ``C`` consecutive streams of a ``StreamPool``, the ready recordings of a tick go through
one launch per kernel, and only the first row of each is resynthesised -- the pool's emit takes a row table, so the ``C - 1``
unused channels are never emitted.

    pool = BeamformStreamPool(max_recordings=16, channels=4)
    rid = pool.open(); pool.push(rid, block); pool.close(rid)        # block (4, m)
    for rid, mono, finished in pool.step(): ...                      # mono (k,)

    sb = StreamBeamformer(n_streams=4, channels=4)     # one recording of four microphones, 8 kHz, block of 4 frames
    mono = sb.push(block)                              # (4, m) -> (k,): what has become final
    tail = sb.flush()
    python -m audiodenoiser_amd.beamform IN OUT --live [--chunk N] [--block B] [--forget A] [--refresh R] [--wpe] [--gain]

The rate handling is ``Denoiser``'s: resample in, resample out, the input's sample count.  The defaults (reference channel 0,
loading 1e-3, mask floor 1e-3) are the values of the host prototype (``profiles/bench_beamform.md``); they were not tuned by ear.

What is NOT here: pools that mix channel counts, look-ahead, GEV or rank-one variants, WPD, more than 8 channels.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from ._host import check_stft_plan, current_stream, model_device, rocm_device, run_files, run_live, stage
from .baseline import SpectralParams, _gain_kept_columns, _spectral_params, spectral_gain
from .denoise import Denoiser
from .dereverb import (WpeParams, WpeStreamParams, _check_channels, _joint_params, _joint_stream_params, _mag_buffer, _need_cells,
                       _spec_dims, _state_bytes, wpe_joint)
from .stream import POOL_MAX_ROWS, RecordingBook, StreamDenoiser, StreamPool, _check_stream_args, causal_carrier
from .griffin_lim import stft_complex
from .resample import _resample_device
from .wav import read_wav, write_wav

__all__ = ["MvdrParams", "mvdr", "Beamformer", "MvdrStreamParams", "mvdr_stream_state_bytes", "mvdr_online", "StreamBeamformer",
           "BeamformStreamPool"]


@dataclasses.dataclass(frozen=True)
class MvdrParams:
    """``adn_mvdr_params`` of ``include/adn.h`` with its defaults and its legal ranges (``ref_channel < channels`` is the call's)."""
    ref_channel: int = 0
    loading: float = 1e-3
    mask_floor: float = 1e-3

    def __post_init__(self):
        v = self.ref_channel
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 7:
            raise ValueError("MvdrParams: need an integer 0 <= ref_channel <= 7")
        for name in ("loading", "mask_floor"):
            if math.isnan(float(getattr(self, name))):
                raise ValueError(f"MvdrParams: {name} is NaN")
        if not 1e-6 <= float(self.loading) <= 1.0:
            raise ValueError("MvdrParams: need 1e-6 <= loading <= 1")
        if not 1e-6 <= float(self.mask_floor) <= 0.25:
            raise ValueError("MvdrParams: need 1e-6 <= mask_floor <= 0.25")

    def to_struct(self) -> "_lib.MvdrParamsStruct":
        return _lib.MvdrParamsStruct(int(self.ref_channel), float(self.loading), float(self.mask_floor))


def _mvdr_params(who, params, channels):
    """The parameters of a call on ``channels`` channels: a ``MvdrParams`` whose reference channel exists, None for the defaults."""
    _check_channels(who, channels)
    if params is None:
        return None
    if not isinstance(params, MvdrParams):
        raise TypeError(f"{who}: params must be a MvdrParams")
    if params.ref_channel >= channels:
        raise ValueError(f"{who}: need ref_channel < channels (ref_channel {params.ref_channel}, channels {channels})")
    return params


def mvdr(spec: torch.Tensor, mag: torch.Tensor, channels: int, params: MvdrParams = None, mag_out: torch.Tensor = None):
    """``adn_mvdr`` on the current stream.  ``spec``: complex64 ``(n_groups * channels, T, F)`` on a ROCm device, the ``channels``
    channels of a recording consecutive clips (``stft_complex`` of an ``(n_groups * channels, L)`` batch).  ``mag``: float32
    ``(n_groups * channels, 1, F, mag_width)``, ``mag_width >= T``, a magnitude estimate of the wanted signal per channel whose
    columns ``[0, T)`` are read -- what ``spectral_gain``, ``wpe_joint`` and the U-Net return.  ``mag_out``: float32
    ``(n_groups, 1, F, width)``, ``width >= T``, whose columns ``[0, T)`` are written and nothing else; None allocates
    ``(n_groups, 1, F, T)``.  The workspace is allocated here.  Returns ``(spec_out, mag_out)``, ``spec_out`` a new complex64
    ``(n_groups, T, F)``.  ValueError, before any device call, if the leading dimension is no multiple of ``channels``, the
    reference channel does not exist, or a shape, dtype or device does not fit."""
    who = "mvdr"
    params = _mvdr_params(who, params, channels)
    if isinstance(spec, torch.Tensor) and spec.dim() == 3 and spec.shape[0] % channels:
        raise ValueError(f"{who}: the leading dimension {spec.shape[0]} is not a multiple of channels = {channels}")
    n, t, f = _spec_dims(who, "clip", spec)
    _need_cells(who, "clip", n, t, f)
    dev = spec.device
    if (not isinstance(mag, torch.Tensor) or not mag.is_cuda or mag.device != dev or mag.dtype != torch.float32 or mag.dim() != 4
            or tuple(mag.shape[:3]) != (n, 1, f) or mag.shape[3] < t):
        raise ValueError(f"{who}: mag must be a (n_clips, 1, n_bins, mag_width >= n_frames) float32 tensor on spec's device")
    groups = n // channels
    mag_out = _mag_buffer(who, "group", mag_out, groups, t, f, dev)
    if mag_out.shape[3] < t:
        raise ValueError(f"{who}: mag_out must be at least n_frames wide")
    s, m = torch.view_as_real(spec.contiguous()), mag.contiguous()
    out = torch.empty((groups, t, f, 2), dtype=torch.float32, device=dev)
    p = ctypes.byref(params.to_struct()) if params is not None else None
    L = _lib.load()
    need = ctypes.c_size_t(0)
    _lib.check(L.adn_mvdr_workspace_bytes(groups, channels, t, f, p, ctypes.byref(need)), "adn_mvdr_workspace_bytes")
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev) if need.value else None
    with torch.cuda.device(dev):
        _lib.check(L.adn_mvdr(s.data_ptr(), m.data_ptr(), int(m.shape[3]), groups, channels, t, f, p,
                              ws.data_ptr() if ws is not None else None, need.value, out.data_ptr(), mag_out.data_ptr(),
                              int(mag_out.shape[3]), current_stream(dev)), "adn_mvdr")
    return torch.view_as_complex(out), mag_out


@dataclasses.dataclass(frozen=True)
class MvdrStreamParams:
    """``adn_mvdr_stream_params`` of ``include/adn.h`` ("beamform stream") with its defaults and its legal ranges
    (``ref_channel < channels`` is the call's).  ``forget = 0.99`` is a window of 100 frames, 1.6 s at hop 128 and 8 kHz: a design
    value, not tuned by ear."""
    ref_channel: int = 0
    refresh: int = 1
    forget: float = 0.99
    loading: float = 1e-3
    mask_floor: float = 1e-3

    def __post_init__(self):
        for name, lo, hi in (("ref_channel", 0, 7), ("refresh", 1, 64)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"MvdrStreamParams: need an integer {lo} <= {name} <= {hi}")
        # the ranges hold for the fp32 values the library sees; a NaN fails every comparison
        for name, lo, hi in (("forget", 0.9, 1.0), ("loading", 1e-6, 1.0), ("mask_floor", 1e-6, 0.25)):
            v = float(getattr(self, name))
            f32 = ctypes.c_float(v).value
            if not lo <= v <= hi or not ctypes.c_float(lo).value <= f32 <= ctypes.c_float(hi).value:
                raise ValueError(f"MvdrStreamParams: need {lo:g} <= {name} <= {hi:g}")

    def to_struct(self) -> "_lib.MvdrStreamParamsStruct":
        return _lib.MvdrStreamParamsStruct(int(self.ref_channel), int(self.refresh), float(self.forget), float(self.loading),
                                           float(self.mask_floor))


def _mvdr_stream_params(who, params, channels):
    """The parameters of a live call on ``channels`` channels: a ``MvdrStreamParams`` whose reference channel exists, None for the
    defaults."""
    _check_channels(who, channels)
    if params is None:
        return None
    if not isinstance(params, MvdrStreamParams):
        raise TypeError(f"{who}: params must be a MvdrStreamParams")
    if params.ref_channel >= channels:
        raise ValueError(f"{who}: need ref_channel < channels (ref_channel {params.ref_channel}, channels {channels})")
    return params


def mvdr_stream_state_bytes(n_slots: int, channels: int, n_bins: int, params: MvdrStreamParams = None) -> int:
    """``adn_mvdr_stream_state_bytes``: the bytes of the opaque state of ``n_slots`` groups of ``channels`` channels and ``n_bins``
    bins (no device needed)."""
    if params is not None and not isinstance(params, MvdrStreamParams):
        raise TypeError("mvdr_stream_state_bytes: params must be a MvdrStreamParams")
    need = ctypes.c_size_t(0)
    p = ctypes.byref(params.to_struct()) if params is not None else None
    _lib.check(_lib.load().adn_mvdr_stream_state_bytes(n_slots, channels, n_bins, p, ctypes.byref(need)), "adn_mvdr_stream_state_bytes")
    return int(need.value)


def mvdr_online(spec: torch.Tensor, mag: torch.Tensor, channels: int, state: torch.Tensor = None, first_frame: int = 0,
                params: MvdrStreamParams = None, mag_out: torch.Tensor = None, col0: int = 0, mag_col0: int = 0):
    """``adn_mvdr_online`` on the current stream.  ``spec``: complex64 ``(n_groups * channels, T, F)`` on a ROCm device, the frames
    ``first_frame ... first_frame + T - 1`` of every row, the ``channels`` channels of a recording consecutive rows.  ``mag``:
    float32 ``(n_groups * channels, 1, F, mag_width)`` whose columns ``[mag_col0, mag_col0 + T)`` are read.  ``state``: the uint8
    tensor an earlier call returned for the frames before them (None allocates one; with ``first_frame = 0`` every group starts
    fresh whatever it holds); it is updated IN PLACE, a slot per GROUP.  ``mag_out``: float32 ``(n_groups, 1, F, width)`` whose
    columns ``[col0, col0 + T)`` are written and nothing else; None allocates ``(n_groups, 1, F, T)``.  Returns ``(y, mag_out,
    state)``, ``y`` a new complex64 ``(n_groups, T, F)``.  ValueError, before any device call, if the leading dimension is no
    multiple of ``channels``, the reference channel does not exist, or a shape, dtype or device does not fit."""
    who = "mvdr_online"
    params = _mvdr_stream_params(who, params, channels)
    if isinstance(spec, torch.Tensor) and spec.dim() == 3 and spec.shape[0] % channels:
        raise ValueError(f"{who}: the leading dimension {spec.shape[0]} is not a multiple of channels = {channels}")
    n, t, f = _spec_dims(who, "row", spec)
    _need_cells(who, "row", n, t, f)
    if not (isinstance(first_frame, int) and first_frame >= 0 and isinstance(col0, int) and col0 >= 0 and isinstance(mag_col0, int)
            and mag_col0 >= 0):
        raise ValueError(f"{who}: need integers first_frame >= 0, col0 >= 0 and mag_col0 >= 0")
    dev = spec.device
    if (not isinstance(mag, torch.Tensor) or not mag.is_cuda or mag.device != dev or mag.dtype != torch.float32 or mag.dim() != 4
            or tuple(mag.shape[:3]) != (n, 1, f) or mag.shape[3] < mag_col0 + t):
        raise ValueError(f"{who}: mag must be a (n_rows, 1, n_bins, mag_width >= mag_col0 + n_frames) float32 tensor on spec's device")
    groups = n // channels
    need = mvdr_stream_state_bytes(groups, channels, f, params)
    if state is None:
        if first_frame != 0:
            raise ValueError(f"{who}: first_frame > 0 continues a group: pass the state of the call before")
        state = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif (not isinstance(state, torch.Tensor) or not state.is_cuda or state.device != dev or state.dtype != torch.uint8
          or state.dim() != 1 or state.numel() < need or not state.is_contiguous()):
        raise ValueError(f"{who}: state must be a contiguous uint8 tensor of at least mvdr_stream_state_bytes on spec's device")
    if mag_out is None and col0 != 0:
        raise ValueError(f"{who}: col0 needs a mag_out buffer")
    mag_out = _mag_buffer(who, "group", mag_out, groups, t, f, dev)
    if mag_out.shape[3] < col0 + t:
        raise ValueError(f"{who}: mag_out must hold columns [col0, col0 + n_frames)")
    s, m = torch.view_as_real(spec.contiguous()), mag.contiguous()
    out = torch.empty((groups, t, f, 2), dtype=torch.float32, device=dev)
    p = ctypes.byref(params.to_struct()) if params is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().adn_mvdr_online(s.data_ptr(), m.data_ptr(), int(m.shape[3]), mag_col0, groups, channels, t, f,
                                               first_frame, p, state.data_ptr(), state.numel(), groups, out.data_ptr(),
                                               mag_out.data_ptr(), int(mag_out.shape[3]), col0, current_stream(dev)), "adn_mvdr_online")
    return torch.view_as_complex(out), mag_out, state


class StreamBeamformer(StreamDenoiser):
    """``StreamDenoiser`` with the streaming beamformer in the network's place: ``n_streams`` is a multiple of ``channels`` and
    ``channels`` consecutive streams are the microphones of ONE recording.  ``push`` and ``flush`` take ``(n_streams, m)`` and return
    ``(n_streams // channels, k)``, or ``(k,)`` for one group; ``reset``, ``received``, ``emitted``, ``latency_samples`` and
    ``input_rate`` are the parent's.

    The operator is causal, so ``lookahead_frames`` is 0 and ``window_frames = max(16, block_frames)`` is only the carrier the
    stream geometry needs.  Each run of steps works in place on the analysed windows: with ``wpe=True`` ``adn_wpe_mc_stream``
    (``wpe_params=None``: ``taps = 32 // channels``); ``adn_spectral_gain_windows`` on the kept columns of every channel, the mask's
    magnitudes (``mask_params``, its own ``(n_streams, 3, F)`` state); ``adn_mvdr_stream`` (``params``); with ``gain=True`` the
    spectral gain again with a second state (``gain_params``).  ``adn_stream_emit`` resynthesises every stream and row ``g C`` of each
    group is kept.  The MVDR and the WPE states need no reset: a stream's frame 0 starts them afresh; ``reset`` forgets both gain
    states.  A ``params`` whose reference channel ``channels`` does not have is a ValueError here."""

    def __init__(self, device=None, n_streams: int = 1, channels: int = 1, sample_rate: int = 8000, n_fft: int = 512,
                 hop_length: int = 128, block_frames: int = 4, params: MvdrStreamParams = None, mask_params: SpectralParams = None,
                 wpe: bool = False, wpe_params: WpeStreamParams = None, gain: bool = False, gain_params: SpectralParams = None,
                 input_rate=None):
        who = "StreamBeamformer"
        window, ahead, batch = causal_carrier(block_frames)
        _check_stream_args(who, n_streams, sample_rate, n_fft, hop_length, window, block_frames, ahead, batch, input_rate)
        self.params = _mvdr_stream_params(who, params, channels)
        if n_streams % channels:
            raise ValueError(f"{who}: n_streams = {n_streams} is not a multiple of channels = {channels}")
        self.mask_params = _spectral_params(who, mask_params, "mask_params")
        self.gain_params = _spectral_params(who, gain_params, "gain_params")
        self.wpe, self.gain, self.channels = bool(wpe), bool(gain), channels
        if wpe_params is not None and not isinstance(wpe_params, WpeStreamParams):
            raise TypeError(f"{who}: wpe_params must be a WpeStreamParams")
        self.wpe_params = _joint_stream_params(who, wpe_params, channels) if self.wpe else None
        dev = rocm_device(who, device)
        self.model = None
        f, groups = n_fft // 2 + 1, n_streams // channels
        self._mvdr_state = torch.empty((mvdr_stream_state_bytes(groups, channels, f, self.params),), dtype=torch.uint8, device=dev)
        self._mask_state = torch.empty((n_streams, 3, f), dtype=torch.float32, device=dev)
        self._gain_state = torch.empty((n_streams, 3, f), dtype=torch.float32, device=dev)
        self._wpe_state = None
        if self.wpe:
            need = _state_bytes(who, groups, None if channels == 1 else channels, f, self.wpe_params)
            self._wpe_state = torch.empty((need,), dtype=torch.uint8, device=dev)
        self._setup(dev, n_streams, sample_rate, n_fft, hop_length, window, block_frames, ahead, batch, input_rate)

    def reset(self):
        """Forget the running recording, both gains' noise estimates included: the object is ready for a new one."""
        super().reset()
        self._mask_state.fill_(-1.0)
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("StreamBeamformer: there is no network; the beamformer runs between analyze and emit (adn_mvdr_stream)")

    def _steps(self, first_step, n_steps, final_length):
        return (first_step, n_steps, final_length, *self._plan, self.max_steps)

    def _beamform(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        """``adn_mvdr_stream`` in place on the windows ``x`` whose kept columns hold the mask's magnitudes."""
        p = ctypes.byref(self.params.to_struct()) if self.params is not None else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_mvdr_stream(self._state.data_ptr(), self._state.numel(), x.data_ptr(), self.n_streams,
                                                   self.channels, *self._steps(first_step, n_steps, final_length), p,
                                                   self._mvdr_state.data_ptr(), self._mvdr_state.numel(), current_stream(self.device)),
                       "adn_mvdr_stream")
        return x

    def _net(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        if self.wpe:
            joint = self.channels != 1
            run = _lib.load().adn_wpe_mc_stream if joint else _lib.load().adn_wpe_stream
            lead = (self.n_streams, self.channels) if joint else (self.n_streams,)
            with torch.cuda.device(self.device):
                _lib.check(run(self._state.data_ptr(), self._state.numel(), x.data_ptr(), *lead,
                               *self._steps(first_step, n_steps, final_length), ctypes.byref(self.wpe_params.to_struct()),
                               self._wpe_state.data_ptr(), self._wpe_state.numel(), current_stream(self.device)), run.__name__)
        _gain_kept_columns(x, None, n_steps, self._mask_state, self._plan, self.mask_params)
        self._beamform(x, first_step, n_steps, final_length)
        if self.gain:
            _gain_kept_columns(x, None, n_steps, self._gain_state, self._plan, self.gain_params)
        return x

    def _result(self, outs):
        """Row ``g C`` of every group of what the streams returned: ``(n_groups, k)``, or ``(k,)`` for one group."""
        out = self._cat(outs)[::self.channels]
        out = out[0] if out.shape[0] == 1 else out.contiguous()
        return out.cpu().numpy() if self._numpy else out


class BeamformStreamPool(StreamPool):
    """``StreamPool`` over RECORDINGS of ``channels`` microphones with the streaming beamformer in the network's place: recordings
    that open, stall, close and run at their own rates, the ready ones batched into one launch per kernel.

        pool = BeamformStreamPool(max_recordings=16, channels=4)
        rid = pool.open()                                  # or open(input_rate=48000) with input_rates=(48000,)
        pool.push(rid, block)                              # (4, m): the next samples of every microphone
        for rid, mono, finished in pool.step(): ...        # (k,): what has become final of the ONE enhanced channel

    Recording ``r`` owns the stream slots ``r C ... r C + C - 1`` of the pool state and slot ``r`` of the MVDR (and WPE) state
    (``stream.RecordingBook``; ``include/adn.h``, ``adn_mvdr_stream_pool``).  A tick analyses the ``C`` rows of every ready
    recording and then, in place on the windows and ``256 // C`` recordings a call: with ``wpe=True``
    ``adn_wpe_mc_stream_pool`` (``wpe_params=None``: ``taps = 32 // C``); ``adn_spectral_gain_windows`` on every row, the mask's
    magnitudes (``mask_params``); ``adn_mvdr_stream_pool`` (``params``).  It keeps the first window of each recording, runs the
    optional output gain (``gain_params``, a state per recording) and ``adn_stream_pool_emit`` on those rows alone: the other
    ``C - 1`` channels are never resynthesised, which is safe because an emit writes nothing but its own slot's overlap-add tail and
    only that slot's later emits read it.  A recording at an ``input_rate`` comes in through ``C`` rows of
    ``adn_stream_pool_push_rate`` and goes out through one of ``adn_stream_pool_emit_rate``.

    Claimed: every recording is, bit for bit, what a solo ``StreamBeamformer(n_streams=C, channels=C, input_rate=...)`` returns for
    the same samples, whatever its neighbours do; it returns as many samples as came in; a recording's slots are reusable without a
    reset.  Not claimed: pools that mix channel counts; more than one step per recording and tick; graph capture of a tick."""

    def __init__(self, device=None, max_recordings: int = 16, channels: int = 2, backlog_steps: int = 4, sample_rate: int = 8000,
                 n_fft: int = 512, hop_length: int = 128, block_frames: int = 4, params: MvdrStreamParams = None,
                 mask_params: SpectralParams = None, wpe: bool = False, wpe_params: WpeStreamParams = None, gain: bool = False,
                 gain_params: SpectralParams = None, input_rates=None):
        who = "BeamformStreamPool"
        window, ahead, _ = causal_carrier(block_frames)
        self.params = _mvdr_stream_params(who, params, channels)
        self.book = RecordingBook(max_recordings, channels, backlog_steps, n_fft, hop_length, window, block_frames, ahead, input_rates,
                                  sample_rate)
        self.mask_params = _spectral_params(who, mask_params, "mask_params")
        self.gain_params = _spectral_params(who, gain_params, "gain_params")
        self.wpe, self.gain = bool(wpe), bool(gain)
        if wpe_params is not None and not isinstance(wpe_params, WpeStreamParams):
            raise TypeError(f"{who}: wpe_params must be a WpeStreamParams")
        self.wpe_params = _joint_stream_params(who, wpe_params, channels) if self.wpe else None
        dev = rocm_device(who, device)
        self.model = None
        self.batch_windows = POOL_MAX_ROWS
        f = n_fft // 2 + 1
        self._mvdr_state = torch.empty((mvdr_stream_state_bytes(max_recordings, channels, f, self.params),), dtype=torch.uint8, device=dev)
        self._mask_state = torch.empty((max_recordings * channels, 3, f), dtype=torch.float32, device=dev)
        self._gain_state = torch.empty((max_recordings, 3, f), dtype=torch.float32, device=dev)
        self._wpe_state = None
        if self.wpe:
            need = _state_bytes(who, max_recordings, None if channels == 1 else channels, f, self.wpe_params)
            self._wpe_state = torch.empty((need,), dtype=torch.uint8, device=dev)
        self._setup(dev)

    def reset(self):
        """Forget every recording, both gains' noise estimates included: all slots are free."""
        super().reset()
        self._mask_state.fill_(-1.0)
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("BeamformStreamPool: there is no network; the beamformer runs between analyze and emit (adn_mvdr_stream_pool)")

    def _emit_rows(self, rows):
        return rows[::self.channels]

    def _net(self, x: torch.Tensor, rows) -> torch.Tensor:
        """The tick's stream rows ``rows`` (``C`` per recording) and their windows ``x`` -> the first window of each recording,
        compacted, holding ``|Y|`` (or the output gain's result) in the kept columns."""
        L, C, plan = _lib.load(), self.channels, self.book.plan
        lead = (self._state.data_ptr(), self._state.numel(), self._args[0], C) + self._args[1:]
        p = ctypes.byref(self.params.to_struct()) if self.params is not None else None
        per = POOL_MAX_ROWS // C * C                         # whole recordings
        for i in range(0, len(rows), per):
            part, group = x[i:i + per], rows[i:i + per]
            with torch.cuda.device(self.device):
                if self.wpe:
                    _lib.check(L.adn_wpe_mc_stream_pool(*lead, self._rows(group), len(group), part.data_ptr(),
                                                        ctypes.byref(self.wpe_params.to_struct()), self._wpe_state.data_ptr(),
                                                        self._wpe_state.numel(), current_stream(self.device)), "adn_wpe_mc_stream_pool")
                _gain_kept_columns(part, group, 1, self._mask_state, plan, self.mask_params)
                _lib.check(L.adn_mvdr_stream_pool(*lead, self._rows(group), len(group), part.data_ptr(), p, self._mvdr_state.data_ptr(),
                                                  self._mvdr_state.numel(), current_stream(self.device)), "adn_mvdr_stream_pool")
        y = x[::C].contiguous()
        if self.gain:                                        # a state per recording: slot // C
            _gain_kept_columns(y, [(slot // C, k, final) for slot, k, final in rows[::C]], 1, self._gain_state, plan, self.gain_params)
        return y


class Beamformer(Denoiser):
    """``Denoiser`` with the beamformer in the network's place: ``(C, L)`` is ONE recording of ``C <= 8`` microphones and comes
    back as ``(L,)``, ``(N, C, L)`` a batch of recordings that comes back as ``(N, L)``; ``(L,)`` is one channel and goes
    through the same pipeline.  ``mask="spectral"``: the spectral baseline's gain of every channel drives the mask
    (``mask_params``); ``mask="model"``: ``model``, a ``UNet(1, 1)`` in eval mode on a ROCm device, does.  ``wpe=True`` runs joint
    WPE first (``wpe_params=None``: ``taps = 32 // C``), ``gain=True`` the spectral gain on the result (``gain_params``).  A
    ``params`` whose reference channel the input does not have is a ValueError of the call."""

    def __init__(self, device=None, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128, params: MvdrParams = None,
                 mask: str = "spectral", mask_params: SpectralParams = None, wpe: bool = False, wpe_params: WpeParams = None,
                 gain: bool = False, gain_params: SpectralParams = None, model=None):
        check_stft_plan("Beamformer", n_fft, hop_length, sample_rate)
        if params is not None and not isinstance(params, MvdrParams):
            raise TypeError("Beamformer: params must be a MvdrParams")
        if wpe_params is not None and not isinstance(wpe_params, WpeParams):
            raise TypeError("Beamformer: wpe_params must be a WpeParams")
        if mask not in ("spectral", "model"):
            raise ValueError("Beamformer: mask must be 'spectral' or 'model'")
        if (mask == "model") != (model is not None):
            raise ValueError("Beamformer: mask='model' needs a model, and a model needs mask='model'")
        self.params, self.mask = params, mask
        self.mask_params = _spectral_params("Beamformer", mask_params, "mask_params")
        self.gain_params = _spectral_params("Beamformer", gain_params, "gain_params")
        self.wpe, self.wpe_params, self.gain = bool(wpe), wpe_params, bool(gain)
        self.model = None                                    # the beamformer itself has no window plan; the mask network has its own
        self._net = None
        if model is not None:
            dev = model_device("Beamformer", model)
            if device is not None and torch.device(device).type != "cuda":
                raise RuntimeError("Beamformer: the device must be a ROCm device; there is no CPU path")
            self._net = Denoiser(model, sample_rate, n_fft, hop_length)
        else:
            dev = rocm_device("Beamformer", device)
        self._setup(dev, sample_rate, n_fft, hop_length, "beamformed")

    def mask_magnitudes(self, spec: torch.Tensor) -> torch.Tensor:
        """complex64 ``(n_clips, T, F)`` -> the magnitude estimate ``(n_clips, 1, F, T)`` that drives the mask, per channel."""
        if self._net is None:
            return spectral_gain(spec, self.mask_params)[0]
        n, t, _ = spec.shape
        return self._net.stitch(self._net.network(self._net.windows(spec)), n, t, clamp=True)[:, None]

    def _core(self, x: torch.Tensor, rand, channels: int = 1) -> torch.Tensor:
        """``x`` (n_groups * channels, L) at the working rate, ``channels`` consecutive clips one recording -> (n_groups, L)."""
        length = x.shape[1]
        params = _mvdr_params("Beamformer", self.params, channels)
        spec = stft_complex(x, self.n_fft, self.hop_length)
        n, t, f = spec.shape
        if self.wpe:
            spec, _ = wpe_joint(spec, channels, _joint_params("Beamformer", self.wpe_params, channels))
        y = torch.zeros((n // channels, 1, f, max(t, 16)), dtype=torch.float32, device=x.device)
        out, _ = mvdr(spec, self.mask_magnitudes(spec), channels, params, y)
        if self.gain:
            spectral_gain(out, self.gain_params, None, y, 0)
        return self._resynth(y, out, length, int(y.shape[3]), 0)

    def denoise(self, audio, sr=None, rand=None):
        """``audio`` float32 at rate ``sr`` (default: the working rate): ``(C, L)`` -> ``(L,)``, ``(N, C, L)`` -> ``(N, L)``,
        ``(L,)`` -> ``(L,)``, at the same rate and sample count.  numpy in -> numpy out, tensor on a ROCm device in -> tensor
        there out; everything between the input copy and the output copy runs on the device on the current stream."""
        a, is_np = stage("Beamformer.denoise", audio, self.device)
        if a.dim() not in (1, 2, 3) or min(a.shape) < 1:
            raise ValueError("Beamformer.denoise: audio must be (L,), (C, L) or (N, C, L) with at least one sample")
        channels = 1 if a.dim() == 1 else int(a.shape[-2])
        _mvdr_params("Beamformer.denoise", self.params, channels)
        length = int(a.shape[-1])
        x = a.reshape(-1, length).contiguous()
        rate = self.sample_rate if sr is None else int(sr)
        if rate != self.sample_rate:
            low = self._core(_resample_device(x, rate, self.sample_rate), rand, channels)
            up = _resample_device(low, self.sample_rate, rate)
            if up.shape[1] >= length:
                out = up[:, :length].contiguous()
            else:
                out = torch.zeros((up.shape[0], length), dtype=torch.float32, device=x.device)
                out[:, :up.shape[1]] = up
        else:
            out = self._core(x, rand, channels)
        out = out if a.dim() == 3 else out[0]
        return out.cpu().numpy() if is_np else out

    def denoise_file(self, src, dst, subtype: str = "PCM_16"):
        """``read_wav(src)``, its channels one recording -> ``denoise`` at the file's rate -> a mono ``write_wav(dst)``.  Returns
        ``(n_samples, sample_rate)``."""
        audio, rate = read_wav(src, mono=False)              # (L, channels)
        out = self.denoise(np.ascontiguousarray(audio.T), sr=rate)
        write_wav(dst, out, rate, subtype)
        return int(audio.shape[0]), int(rate)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.beamform",
                                 description="Beamform a multichannel wav file, or a folder of them, to mono (mask-driven MVDR).")
    ap.add_argument("src", metavar="IN", help="a wav file whose channels are the microphones, or a folder of such files")
    ap.add_argument("dst", metavar="OUT", help="the mono wav file to write, or the folder to write into")
    ap.add_argument("--reference", metavar="CLEAN", default=None,
                    help="the clean wav of IN (or a folder with IN's file names): print one JSON line of metrics per file")
    ap.add_argument("--ref-channel", type=int, default=MvdrParams.ref_channel, help="the microphone the output is aligned to, 0 ... 7")
    ap.add_argument("--wpe", action="store_true", help="run joint WPE (taps = 32 // channels) before the beamformer")
    ap.add_argument("--gain", action="store_true", help="run the spectral baseline's Wiener gain on the beamformer's result")
    ap.add_argument("--model", metavar="CKPT", default=None,
                    help="take the mask from this U-Net checkpoint instead of the spectral gain (the state_dict of UNet(1, 1))")
    ap.add_argument("--live", action="store_true",
                    help="push the file (not a folder) through the streaming beamformer at its own rate, as a live feed arrives")
    ap.add_argument("--chunk", type=int, default=1024, help="with --live: samples per push, at the file's rate")
    ap.add_argument("--block", type=int, default=4, help="with --live: frames per step (latency (block - 1) hop + n_fft samples)")
    ap.add_argument("--forget", type=float, default=MvdrStreamParams.forget, help="with --live: forgetting factor, 0.9 ... 1")
    ap.add_argument("--refresh", type=int, default=MvdrStreamParams.refresh, help="with --live: frames between two solves, 1 ... 64")
    args = ap.parse_args(argv)
    if args.live:
        import os
        if args.chunk < 1 or args.block < 1:
            ap.error("--chunk and --block must be >= 1")
        if os.path.isdir(args.src):
            ap.error("--live takes one wav file")
        if args.model is not None:
            ap.error("--live takes its mask from the spectral gain: no --model")

        def make(dev, n_streams, rate):
            if not 1 <= n_streams <= 8:
                raise ValueError(f"--live: {n_streams} channels; the beamformer takes 1 ... 8")
            live = MvdrStreamParams(ref_channel=args.ref_channel, refresh=args.refresh, forget=args.forget)
            return StreamBeamformer(dev, n_streams=n_streams, channels=n_streams, block_frames=args.block, params=live, wpe=args.wpe,
                                    gain=args.gain, input_rate=rate)
        try:
            return run_live(make, args.src, args.dst, args.chunk, args.reference)
        except ValueError as exc:
            ap.error(str(exc))
    try:
        params = MvdrParams(ref_channel=args.ref_channel)
    except ValueError as exc:
        ap.error(str(exc))
    model = None
    if args.model is not None:
        from .denoise import _load_model
        model = _load_model(args.model, "f32", _lib.staging_device())
    bf = Beamformer(params=params, mask="model" if model is not None else "spectral", wpe=args.wpe, gain=args.gain, model=model)
    try:
        return run_files(bf, args.src, args.dst, args.reference)
    except ValueError as exc:
        ap.error(str(exc))


if __name__ == "__main__":
    raise SystemExit(main())
