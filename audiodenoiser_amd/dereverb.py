"""Dereverberation baseline: weighted prediction error (WPE) per frequency bin, no checkpoint.

    from audiodenoiser_amd.dereverb import Dereverberator, WpeParams, wpe
    dr = Dereverberator()                              # no model: the current ROCm device, 8 kHz, n_fft 512, hop 128
    dry = dr.denoise(reverberant, sr=44100)            # (L,) or (N, L); numpy -> numpy, device tensor -> device tensor
    dr.denoise_file("room.wav", "dry.wav")
    Dereverberator(gain=True)                          # WPE, then the Wiener gain of the spectral baseline on its result
    Dereverberator(channels="joint")                   # (C, L) is ONE recording of C microphones, (N, C, L) a batch of them

    live = StreamDereverberator(n_streams=2)           # audio that is still arriving: recursive WPE, one update per frame
    out = live.push(block); ...; out = live.flush()    # the surface of StreamDenoiser; DereverbStreamPool: that of StreamPool
    d, mag, state = wpe_online(spec)                   # the recursion on a spectrogram; pass state and first_frame to go on
    live = StreamDereverberator(n_streams=2, channels=2)   # the two streams are ONE recording: the recursive joint form
    d, mag, state = wpe_online_joint(spec, 2)          # the joint recursion, (n_groups * 2, T, F)

    python -m audiodenoiser_amd.dereverb IN OUT [--reference CLEAN] [--taps K] [--delay D] [--iterations I] [--gain] [--joint]
    python -m audiodenoiser_amd.dereverb IN OUT --live [--chunk N] [--block B] [--forget A] [--gain] [--joint] [--reference CLEAN]

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

``channels="joint"`` replaces that rule: the channels of a recording are dereverberated together by ``adn_wpe_mc``
(``csrc/dereverb_mc_kernels.hip``), DEFINED in ``include/adn.h`` ("dereverb multichannel"; float64 restatement:
``tests/dereverb_mc_ref.py``) and unpinned against any package like its sibling: every channel's late reverberation is predicted
from the past frames of all channels, ``taps`` per channel, ``channels * taps <= 32``.  A ``(C, L)`` input is one recording of
``C <= 8`` channels, ``(N, C, L)`` a batch of recordings, ``denoise_file`` takes the wav's channels as one recording, and
``params=None`` takes ``taps = 32 // C`` -- a design value from the host figures in ``profiles/bench_dereverb_mc.md``, not tuned
by ear.  A mono input is the single-channel path.  ``wpe_joint`` is the operator on spectrograms.

The streaming form is a different algorithm with its own kernel, DEFINED in ``include/adn.h`` ("dereverb stream"; float64
restatement: ``tests/dereverb_stream_ref.py``; ``csrc/dereverb_stream_kernels.hip``): recursive least squares per (stream, bin), a
K x K inverse correlation matrix and K taps carried on the device and updated once per frame.  ``StreamDereverberator`` is
``StreamDenoiser`` and ``DereverbStreamPool`` is ``StreamPool`` with ``adn_wpe_stream`` / ``adn_wpe_stream_pool`` in the network's
place, exactly as ``StreamSpectralDenoiser`` / ``SpectralStreamPool`` carry the spectral gain; ``gain=True`` runs that gain on the
same columns afterwards, the streaming form of the cascade.  A row that starts at frame 0 starts fresh whatever the WPE state
holds, so there is nothing to reset.

``StreamDereverberator(channels=C)`` is the joint form of that recursion, DEFINED in ``include/adn.h`` ("dereverb stream
multichannel"; float64 restatement: ``tests/dereverb_mc_stream_ref.py``; ``csrc/dereverb_mc_stream_kernels.hip``): ``C``
consecutive streams are one recording, an N x N matrix with ``N = C * taps <= 32`` and N x C taps per (recording, bin), one
variance shared by the channels; ``adn_wpe_mc_stream`` stands in ``adn_wpe_stream``'s place and nothing else changes.
``params=None`` takes ``taps = 32 // C``.  With more than one channel ``2 N (1 - forget) <= 1`` must hold (the header says why).
``wpe_online_joint`` is the recursion on spectrograms.  ``DereverbStreamPool(channels=C)`` serves many such recordings with
independent timing: recording ``r`` owns ``C`` consecutive stream slots of the pool and one slot of the joint state, and
``adn_wpe_mc_stream_pool`` runs the ready ones in one launch (``stream.RecordingBook``).

What is NOT here: pools that mix channel counts, look-ahead or iterated online
variants, any tuning of the defaults by ear.  Combining the channels into one is ``audiodenoiser_amd.beamform`` (``Beamformer``,
``wpe=True`` puts ``wpe_joint`` in front of it).  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os

import torch

from . import _lib
from ._host import check_stft_plan, current_stream, rocm_device, run_files, run_live
from .baseline import SpectralParams, _gain_kept_columns, _spectral_params, spectral_gain
from .denoise import Denoiser
from .griffin_lim import stft_complex
from .stream import POOL_MAX_ROWS, PoolBook, RecordingBook, StreamDenoiser, StreamPool, _check_stream_args, causal_carrier

__all__ = ["WpeParams", "wpe", "wpe_joint", "Dereverberator", "WpeStreamParams", "wpe_online", "wpe_stream_state_bytes",
           "wpe_online_joint", "wpe_stream_state_bytes_joint", "StreamDereverberator", "DereverbStreamPool"]


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


def _spec_dims(who, row, spec):
    """``spec`` is a complex64 ``(rows, frames, bins)`` tensor on a ROCm device: its shape.  ``row``: what ``who`` calls a row."""
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 3:
        raise ValueError(f"{who}: expected a (n_{row}s, n_frames, n_bins) complex64 tensor on a ROCm device")
    return spec.shape


def _need_cells(who, row, n, t, f):
    if n < 1 or t < 1 or f < 1:
        raise ValueError(f"{who}: need at least one {row}, one frame and one bin")


def _mag_buffer(who, row, mag_out, n, t, f, dev):
    """``mag_out`` checked against ``spec``'s ``(n, t, f)`` and device; None allocates ``(n, 1, f, t)``."""
    if mag_out is None:
        return torch.empty((n, 1, f, t), dtype=torch.float32, device=dev)
    if (not isinstance(mag_out, torch.Tensor) or not mag_out.is_cuda or mag_out.device != dev or mag_out.dtype != torch.float32
            or mag_out.dim() != 4 or tuple(mag_out.shape[:3]) != (n, 1, f) or not mag_out.is_contiguous()):
        raise ValueError(f"{who}: mag_out must be a contiguous (n_{row}s, 1, n_bins, width) float32 tensor on spec's device")
    return mag_out


def _entry(name, count, channels):
    """The C function of an operator and the arguments that size its batch: ``adn_wpe<name>`` and ``(count,)`` for the
    single-channel form (``channels=None``), ``adn_wpe_mc<name>`` and ``(count, channels)`` for the joint one.  The library treats
    the joint function at one channel like its sibling; the names in its messages and the taps of ``params=NULL`` differ, so each
    Python function keeps calling its own."""
    L = _lib.load()
    return (getattr(L, "adn_wpe" + name), (count,)) if channels is None else (getattr(L, "adn_wpe_mc" + name), (count, channels))


def _wpe(who, spec, channels, params, mag_out):
    """``adn_wpe`` (``channels=None``) or ``adn_wpe_mc`` on the current stream, the workspace allocated here."""
    n, t, f = _spec_dims(who, "clip", spec)
    _need_cells(who, "clip", n, t, f)
    dev = spec.device
    s = torch.view_as_real(spec.contiguous())
    mag_out = _mag_buffer(who, "clip", mag_out, n, t, f, dev)
    out = torch.empty((n, t, f, 2), dtype=torch.float32, device=dev)
    p = ctypes.byref(params.to_struct()) if params is not None else None
    groups = n if channels is None else n // channels
    (size, shape), (run, _) = _entry("_workspace_bytes", groups, channels), _entry("", groups, channels)
    need = ctypes.c_size_t(0)
    _lib.check(size(*shape, t, f, p, ctypes.byref(need)), size.__name__)
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev) if need.value else None
    with torch.cuda.device(dev):
        _lib.check(run(s.data_ptr(), *shape, t, f, p, ws.data_ptr() if ws is not None else None, need.value, out.data_ptr(),
                       mag_out.data_ptr(), int(mag_out.shape[3]), current_stream(dev)), run.__name__)
    return torch.view_as_complex(out), mag_out


def wpe(spec: torch.Tensor, params: WpeParams = None, mag_out: torch.Tensor = None):
    """``adn_wpe`` on the current stream.  ``spec``: complex64 ``(n_clips, T, F)`` on a ROCm device (``stft_complex``).
    ``mag_out``: float32 ``(n_clips, 1, F, width)``, ``width >= T``, whose columns ``[0, T)`` are written and nothing else; None
    allocates ``(n_clips, 1, F, T)``.  The workspace is allocated here.  Returns ``(spec_out, mag_out)``, ``spec_out`` a new
    complex64 tensor of ``spec``'s shape."""
    if params is not None and not isinstance(params, WpeParams):
        raise TypeError("wpe: params must be a WpeParams")
    return _wpe("wpe", spec, None, params, mag_out)


def _check_channels(who, channels):
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= 8:
        raise ValueError(f"{who}: need an integer 1 <= channels <= 8")


def _joint_rules(cls, who, params, channels):
    """The parameters (a ``cls``: ``WpeParams`` or ``WpeStreamParams``) of a joint call on ``channels`` channels: ``params``, or
    the defaults with ``taps = 32 // channels``.  ValueError for a channel count outside 1 ... 8, for ``channels * taps > 32`` and
    -- the streaming form only, with more than one channel -- for ``2 channels taps (1 - forget) > 1`` on the fp32 value of
    ``forget``: the rules of "dereverb multichannel" and "dereverb stream multichannel", checked here because here the channel
    count is known, before anything looks at a device."""
    _check_channels(who, channels)
    if params is None:
        return cls(taps=32 // channels)
    if not isinstance(params, cls):
        raise TypeError(f"{who}: params must be a {cls.__name__}")
    n = channels * params.taps
    if n > 32:
        raise ValueError(f"{who}: need channels * taps <= 32 (channels {channels}, taps {params.taps})")
    if cls is WpeStreamParams and channels > 1 and not 2.0 * n * (1.0 - ctypes.c_float(float(params.forget)).value) <= 1.0:
        raise ValueError(f"{who}: need 2 channels taps (1 - forget) <= 1 with more than one channel: forget >= {1 - 1 / (2 * n):.6f} "
                         f"at channels * taps = {n} (forget {params.forget})")
    return params


def _joint_params(who, params, channels):
    return _joint_rules(WpeParams, who, params, channels)


def wpe_joint(spec: torch.Tensor, channels: int, params: WpeParams = None, mag_out: torch.Tensor = None):
    """``adn_wpe_mc`` on the current stream: ``wpe`` with the leading dimension ``n_groups * channels``, the ``channels`` channels
    of a recording consecutive clips (``stft_complex`` of an ``(n_groups * channels, L)`` batch), dereverberated jointly.
    ``params=None``: the defaults with ``taps = 32 // channels``.  ValueError if the leading dimension is no multiple of
    ``channels`` or ``channels * taps > 32``.  ``channels = 1`` returns ``wpe``'s bits."""
    params = _joint_params("wpe_joint", params, channels)
    if isinstance(spec, torch.Tensor) and spec.dim() == 3 and spec.shape[0] % channels:
        raise ValueError(f"wpe_joint: the leading dimension {spec.shape[0]} is not a multiple of channels = {channels}")
    return _wpe("wpe_joint", spec, channels, params, mag_out)


class Dereverberator(Denoiser):
    """``Denoiser`` with WPE in the network's place: no model, the phase of the dereverberated spectrum.  ``gain=True`` runs the
    spectral baseline's Wiener gain (``gain_params``) on the result of WPE: the cascade.

    ``channels="separate"`` (default): every channel a clip of its own, ``Denoiser``'s rule.  ``channels="joint"``: the channels
    of a recording are dereverberated together (``wpe_joint``): ``(C, L)`` is one recording of ``C <= 8`` channels, ``(N, C, L)``
    a batch, ``denoise_file`` takes the wav's channels as one recording; ``params=None`` then takes ``taps = 32 // C``, and a
    ``params`` with ``C * taps > 32`` is a ValueError of the call.  A mono input is the single-channel path; the gain runs per
    channel on the joint result.  ``joint_default_taps=True`` (keyword only; the command line's "no ``--taps``") keeps that
    ``32 // C`` rule with a ``params`` that sets the other fields; None: exactly when ``params`` is None."""

    def __init__(self, device=None, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128, params: WpeParams = None,
                 gain: bool = False, gain_params: SpectralParams = None, channels: str = "separate", *,
                 joint_default_taps: bool = None):
        check_stft_plan("Dereverberator", n_fft, hop_length, sample_rate)
        if params is not None and not isinstance(params, WpeParams):
            raise TypeError("Dereverberator: params must be a WpeParams")
        if channels not in ("separate", "joint"):
            raise ValueError("Dereverberator: channels must be 'separate' or 'joint'")
        self.params = WpeParams() if params is None else params
        self.channels = channels
        self.joint_channels = channels == "joint"            # Denoiser.denoise: (C, L) is one recording, _core is told C
        self._default_taps = params is None if joint_default_taps is None else bool(joint_default_taps)   # joint: taps = 32 // C
        self.gain = bool(gain)
        self.gain_params = _spectral_params("Dereverberator", gain_params, "gain_params")
        self.model = None
        self._setup(rocm_device("Dereverberator", device), sample_rate, n_fft, hop_length, "dereverberated")

    def _core(self, x: torch.Tensor, rand, channels: int = 1) -> torch.Tensor:
        """``x`` (n_clips, L) at the working rate -> (n_clips, L); ``channels`` consecutive clips are one recording."""
        n, length = x.shape
        joint = None
        if channels != 1:
            joint = _joint_params("Dereverberator", None if self._default_taps else self.params, channels)
            if self._default_taps:
                joint = dataclasses.replace(self.params, taps=joint.taps)
        spec = stft_complex(x, self.n_fft, self.hop_length)
        t, f = spec.shape[1], spec.shape[2]
        y = torch.zeros((n, 1, f, max(t, 16)), dtype=torch.float32, device=x.device)
        d, _ = wpe(spec, self.params, y) if joint is None else wpe_joint(spec, channels, joint, y)
        if self.gain:
            spectral_gain(d, self.gain_params, None, y, 0)
        return self._resynth(y, d, length, int(y.shape[3]), 0)


@dataclasses.dataclass(frozen=True)
class WpeStreamParams:
    """``adn_wpe_stream_params`` of ``include/adn.h`` ("dereverb stream") with its defaults and its legal ranges."""
    taps: int = 20
    delay: int = 3
    forget: float = 0.99
    loading: float = 300.0
    power_floor: float = 0.01
    smooth: float = 0.9

    def __post_init__(self):
        for name, lo, hi in (("taps", 1, 32), ("delay", 1, 8)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"WpeStreamParams: need an integer {lo} <= {name} <= {hi}")
        # the ranges hold for the fp32 values the library sees; a NaN fails every comparison
        f32 = {name: ctypes.c_float(float(getattr(self, name))).value for name in ("forget", "loading", "power_floor", "smooth")}
        if not 0.95 <= float(self.forget) <= 1.0 or not ctypes.c_float(0.95).value <= f32["forget"]:
            raise ValueError("WpeStreamParams: need 0.95 <= forget <= 1")
        if not 1.0 <= float(self.loading) <= 1e6:
            raise ValueError("WpeStreamParams: need 1 <= loading <= 1e6")
        if not 0.0 < float(self.power_floor) <= 1.0 or not f32["power_floor"] > 0.0:
            raise ValueError("WpeStreamParams: need 0 < power_floor <= 1")
        if not 0.0 <= float(self.smooth) < 1.0 or not f32["smooth"] < 1.0:
            raise ValueError("WpeStreamParams: need 0 <= smooth < 1")

    def to_struct(self) -> "_lib.WpeStreamParamsStruct":
        return _lib.WpeStreamParamsStruct(int(self.taps), int(self.delay), float(self.forget), float(self.loading),
                                          float(self.power_floor), float(self.smooth))


def _stream_params(who, params):
    if params is not None and not isinstance(params, WpeStreamParams):
        raise TypeError(f"{who}: params must be a WpeStreamParams")
    return ctypes.byref(params.to_struct()) if params is not None else None


def _state_bytes(who, n_slots, channels, n_bins, params):
    """``adn_wpe_stream_state_bytes`` (``channels=None``) or ``adn_wpe_mc_stream_state_bytes``."""
    size, lead = _entry("_stream_state_bytes", n_slots, channels)
    need = ctypes.c_size_t(0)
    _lib.check(size(*lead, n_bins, _stream_params(who, params), ctypes.byref(need)), size.__name__)
    return int(need.value)


def wpe_stream_state_bytes(n_slots: int, n_bins: int, params: WpeStreamParams = None) -> int:
    """``adn_wpe_stream_state_bytes``: the bytes of the opaque WPE state of ``n_slots`` rows of ``n_bins`` bins (no device needed)."""
    return _state_bytes("wpe_stream_state_bytes", n_slots, None, n_bins, params)


def _joint_stream_params(who, params, channels):
    return _joint_rules(WpeStreamParams, who, params, channels)


def wpe_stream_state_bytes_joint(n_slots: int, channels: int, n_bins: int, params: WpeStreamParams = None) -> int:
    """``adn_wpe_mc_stream_state_bytes``: the bytes of the opaque joint WPE state of ``n_slots`` groups of ``channels`` channels
    and ``n_bins`` bins (no device needed).  ``params=None``: the defaults with ``taps = 32 // channels``."""
    return _state_bytes("wpe_stream_state_bytes_joint", n_slots, channels, n_bins, params)


def wpe_online(spec: torch.Tensor, state: torch.Tensor = None, first_frame: int = 0, params: WpeStreamParams = None,
               mag_out: torch.Tensor = None, col0: int = 0):
    """``adn_wpe_online`` on the current stream.  ``spec``: complex64 ``(n_rows, T, F)`` on a ROCm device, the frames
    ``first_frame ... first_frame + T - 1`` of every row.  ``state``: the uint8 tensor an earlier call returned for the frames before
    them (None allocates one; with ``first_frame = 0`` every row starts fresh whatever it holds); it is updated IN PLACE.
    ``mag_out``: float32 ``(n_rows, 1, F, width)`` whose columns ``[col0, col0 + T)`` are written and nothing else; None allocates
    ``(n_rows, 1, F, T)``.  Returns ``(d, mag_out, state)``, ``d`` a new complex64 tensor of ``spec``'s shape."""
    return _wpe_online("wpe_online", spec, None, state, first_frame, params, mag_out, col0)


def wpe_online_joint(spec: torch.Tensor, channels: int, state: torch.Tensor = None, first_frame: int = 0,
                     params: WpeStreamParams = None, mag_out: torch.Tensor = None, col0: int = 0):
    """``adn_wpe_mc_online`` on the current stream: ``wpe_online`` with the leading dimension ``n_groups * channels``, the
    ``channels`` channels of a recording consecutive rows, dereverberated jointly; the state (``wpe_stream_state_bytes_joint``)
    has a slot per GROUP.  ``params=None``: the defaults with ``taps = 32 // channels``.  ValueError if the leading dimension is
    no multiple of ``channels``, ``channels * taps > 32`` or the forget rule is broken.  ``channels = 1`` returns ``wpe_online``'s
    bits, state included."""
    params = _joint_stream_params("wpe_online_joint", params, channels)
    if isinstance(spec, torch.Tensor) and spec.dim() == 3 and spec.shape[0] % channels:
        raise ValueError(f"wpe_online_joint: the leading dimension {spec.shape[0]} is not a multiple of channels = {channels}")
    return _wpe_online("wpe_online_joint", spec, channels, state, first_frame, params, mag_out, col0)


def _wpe_online(who, spec, channels, state, first_frame, params, mag_out, col0):
    """``adn_wpe_online`` (``channels=None``) or ``adn_wpe_mc_online`` on the current stream."""
    n, t, f = _spec_dims(who, "row", spec)
    p = _stream_params(who, params)
    _need_cells(who, "row", n, t, f)
    if not (isinstance(first_frame, int) and first_frame >= 0 and isinstance(col0, int) and col0 >= 0):
        raise ValueError(f"{who}: need integers first_frame >= 0 and col0 >= 0")
    dev = spec.device
    slots = n if channels is None else n // channels
    need = _state_bytes(who, slots, channels, f, params)
    if state is None:
        if first_frame != 0:
            raise ValueError(f"{who}: first_frame > 0 continues a row: pass the state of the call before")
        state = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif (not isinstance(state, torch.Tensor) or not state.is_cuda or state.device != dev or state.dtype != torch.uint8
          or state.dim() != 1 or state.numel() < need or not state.is_contiguous()):
        raise ValueError(f"{who}: state must be a contiguous uint8 tensor of at least wpe_stream_state_bytes on spec's device")
    s = torch.view_as_real(spec.contiguous())
    if mag_out is None and col0 != 0:
        raise ValueError(f"{who}: col0 needs a mag_out buffer")
    mag_out = _mag_buffer(who, "row", mag_out, n, t, f, dev)
    out = torch.empty((n, t, f, 2), dtype=torch.float32, device=dev)
    run, shape = _entry("_online", slots, channels)
    with torch.cuda.device(dev):
        _lib.check(run(s.data_ptr(), *shape, t, f, first_frame, p, state.data_ptr(), state.numel(), slots, out.data_ptr(),
                       mag_out.data_ptr(), int(mag_out.shape[3]), col0, current_stream(dev)), run.__name__)
    return torch.view_as_complex(out), mag_out, state


def _wpe_setup(sd, who, device, n_slots, n_fft, params, gain, gain_params, channels=1):
    """What both stream classes carry for the operator, ``n_slots`` rows of it: the parameters, the WPE state and the gain's three
    floats per bin, on the device this returns.  Refuses parameter types before it looks at the device.  ``channels > 1``:
    ``channels`` consecutive rows are one recording, a WPE slot per recording; the gain stays per row."""
    _stream_params(who, params)
    joint = _joint_stream_params(who, params, channels) if channels != 1 else None
    if n_slots % channels:
        raise ValueError(f"{who}: n_streams = {n_slots} is not a multiple of channels = {channels}")
    sd.gain_params = _spectral_params(who, gain_params, "gain_params")
    dev = rocm_device(who, device)
    sd.model = None
    sd.channels = channels
    sd.params = joint if joint is not None else WpeStreamParams() if params is None else params
    sd.gain = bool(gain)
    f = n_fft // 2 + 1
    need = _state_bytes(who, n_slots // channels, None if channels == 1 else channels, f, sd.params)
    sd._wpe_state = torch.empty((need,), dtype=torch.uint8, device=dev)
    sd._gain_state = torch.empty((n_slots, 3, f), dtype=torch.float32, device=dev)
    return dev


def _wpe_then_gain(sd, x: torch.Tensor, rows, n_steps: int, first_step: int = 0, final_length: int = -1) -> torch.Tensor:
    """The operator of both stream classes between ``analyze`` and ``emit``, in place on the analysed windows ``x``; every state
    is read from ``sd`` when it runs.  ``rows=None``: the lockstep object's steps ``first_step ..``, ``n_steps`` per stream
    (``adn_wpe_stream``, or ``adn_wpe_mc_stream`` when ``sd.channels`` consecutive streams are one recording).  Otherwise a pool tick's rows ``(slot, step, final_length)``, one step each, ``POOL_MAX_ROWS`` a call
    (``adn_wpe_stream_pool``); in a pool of recordings ``sd.channels`` consecutive rows are one, ``256 // channels`` recordings a
    call (``adn_wpe_mc_stream_pool``).  With ``sd.gain`` the spectral gain follows each call on the columns it wrote."""
    L = _lib.load()
    state = (sd._state.data_ptr(), sd._state.numel())
    wpe_args = (ctypes.byref(sd.params.to_struct()), sd._wpe_state.data_ptr(), sd._wpe_state.numel(), current_stream(sd.device))
    if rows is None:
        plan, groups = sd._plan, [(x, None)]
    else:
        per = POOL_MAX_ROWS // sd.channels * sd.channels          # whole recordings
        plan, groups = sd.book.plan, [(x[i:i + per], rows[i:i + per]) for i in range(0, len(rows), per)]
    for part, group in groups:
        with torch.cuda.device(sd.device):
            if group is None:
                run, lead = _entry("_stream", sd.n_streams, None if sd.channels == 1 else sd.channels)
                _lib.check(run(*state, part.data_ptr(), *lead, first_step, n_steps, final_length, *plan, sd.max_steps, *wpe_args),
                           run.__name__)
            elif sd.channels == 1:
                _lib.check(L.adn_wpe_stream_pool(*state, *sd._args, sd._rows(group), len(group), part.data_ptr(), *wpe_args),
                           "adn_wpe_stream_pool")
            else:
                _lib.check(L.adn_wpe_mc_stream_pool(*state, sd._args[0], sd.channels, *sd._args[1:], sd._rows(group), len(group),
                                                    part.data_ptr(), *wpe_args), "adn_wpe_mc_stream_pool")
        if sd.gain:
            _gain_kept_columns(part, group, n_steps, sd._gain_state, plan, sd.gain_params)
    return x


class StreamDereverberator(StreamDenoiser):
    """``StreamDenoiser`` with recursive WPE in the network's place: no model, the phase of the dereverberated spectrum, the same
    surface -- ``push``, ``flush``, ``reset``, ``received``, ``emitted``, ``latency_samples``, ``analyze``, ``emit``, ``input_rate``.

    The operator is causal, so ``lookahead_frames`` is 0 and ``window_frames = max(16, block_frames)`` is only the carrier the
    stream geometry needs: each run of steps calls ``adn_wpe_stream`` in place on the analysed windows -- ``d`` into the frames the
    steps emit, ``|d|`` into the ``block_frames`` columns ``adn_stream_emit`` reads -- and with ``gain=True`` then
    ``adn_spectral_gain_windows`` on the same columns (``gain_params``), whose three floats per bin live beside the WPE state.  The
    WPE state needs no reset: a stream's frame 0 starts it afresh.  ``block_frames = 4``: as ``StreamSpectralDenoiser``.

    ``channels = C > 1``: ``n_streams`` is a multiple of ``C`` and ``C`` consecutive streams are the microphones of ONE recording,
    dereverberated jointly (``adn_wpe_mc_stream``, "dereverb stream multichannel").  ``params=None`` then takes ``taps = 32 // C``;
    a ``params`` with ``C * taps > 32`` or ``2 C taps (1 - forget) > 1`` is a ValueError here.  The gain, the resamplers of
    ``input_rate`` and everything else stay per stream.  ``channels = 1`` is the single-channel object, bit for bit."""

    def __init__(self, device=None, n_streams: int = 1, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128,
                 block_frames: int = 4, params: WpeStreamParams = None, gain: bool = False, gain_params: SpectralParams = None,
                 input_rate=None, channels: int = 1):
        window, ahead, batch = causal_carrier(block_frames)
        _check_stream_args("StreamDereverberator", n_streams, sample_rate, n_fft, hop_length, window, block_frames, ahead, batch,
                           input_rate)
        _check_channels("StreamDereverberator", channels)
        dev = _wpe_setup(self, "StreamDereverberator", device, n_streams, n_fft, params, gain, gain_params, channels)
        self._setup(dev, n_streams, sample_rate, n_fft, hop_length, window, block_frames, ahead, batch, input_rate)

    def reset(self):
        """Forget the running stream, the gain's noise estimate included: the object is ready for a new one."""
        super().reset()
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("StreamDereverberator: there is no network; WPE runs between analyze and emit (adn_wpe_stream)")

    def _net(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        return _wpe_then_gain(self, x, None, n_steps, first_step, final_length)


class DereverbStreamPool(StreamPool):
    """``StreamPool`` with recursive WPE in the network's place: ``open``, ``push``, ``push_many``, ``close``, ``step``, ``drain``,
    ``room``, ``received`` and the rates are the parent's.  A tick calls ``adn_wpe_stream_pool`` once per group of up to 256 rows,
    in place on the analysed windows (and with ``gain=True`` ``adn_spectral_gain_windows`` with ``rows = (slot, step == 0)``).  A
    stream's frame 0 starts its slot afresh, so a slot is reusable without a reset.  Each stream is, bit for bit, what a solo
    ``StreamDereverberator`` (at its ``input_rate``) returns for the same samples.

    ``channels = C > 1``: a pool of RECORDINGS of ``C`` microphones, dereverberated jointly (``adn_wpe_mc_stream_pool``;
    ``RecordingBook``).  ``max_streams`` counts recordings, ``open`` returns a recording id, ``push(rid, block)`` takes ``(C, m)``,
    ``step`` returns ``(rid, samples (C, k), finished)``; ``params=None`` takes ``taps = 32 // C``, with the rules of
    ``StreamDereverberator(channels=C)``; the gain stays per channel.  Each recording is, bit for bit, what a solo
    ``StreamDereverberator(n_streams=C, channels=C)`` returns.  ``channels = 1`` is the pool of single streams."""

    def __init__(self, device=None, max_streams: int = 64, backlog_steps: int = 4, sample_rate: int = 8000, n_fft: int = 512,
                 hop_length: int = 128, block_frames: int = 4, params: WpeStreamParams = None, gain: bool = False,
                 gain_params: SpectralParams = None, input_rates=None, channels: int = 1):
        window, ahead, _ = causal_carrier(block_frames)
        _check_channels("DereverbStreamPool", channels)
        if channels == 1:
            self.book = PoolBook(max_streams, backlog_steps, n_fft, hop_length, window, block_frames, ahead, input_rates, sample_rate)
        else:
            self.book = RecordingBook(max_streams, channels, backlog_steps, n_fft, hop_length, window, block_frames, ahead, input_rates,
                                      sample_rate)
        dev = _wpe_setup(self, "DereverbStreamPool", device, max_streams * channels, n_fft, params, gain, gain_params, channels)
        self.batch_windows = POOL_MAX_ROWS
        self._setup(dev)

    def reset(self):
        """Forget every stream, the gain's noise estimates included: all slots are free."""
        super().reset()
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("DereverbStreamPool: there is no network; WPE runs between analyze and emit (adn_wpe_stream_pool, "
                           "adn_wpe_mc_stream_pool)")

    def _net(self, x: torch.Tensor, rows) -> torch.Tensor:
        return _wpe_then_gain(self, x, rows, 1)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.dereverb",
                                 description="Dereverberate a wav file or a folder of wav files with per-bin WPE (no checkpoint).")
    ap.add_argument("src", metavar="IN", help="a wav file, or a folder of wav files")
    ap.add_argument("dst", metavar="OUT", help="the wav file to write, or the folder to write into")
    ap.add_argument("--reference", metavar="CLEAN", default=None,
                    help="the dry wav of IN (or a folder with IN's file names): print one JSON line of metrics per file")
    ap.add_argument("--taps", type=int, default=None,
                    help=f"prediction taps K, 1 ... 32 (default {WpeParams.taps}; with --joint 32 // channels, per channel, --live too)")
    ap.add_argument("--delay", type=int, default=WpeParams.delay, help="prediction delay D in frames, 1 ... 8")
    ap.add_argument("--iterations", type=int, default=WpeParams.iterations, help="iterations I, 1 ... 8")
    ap.add_argument("--gain", action="store_true", help="run the spectral baseline's Wiener gain on the result of WPE")
    ap.add_argument("--joint", action="store_true",
                    help="dereverberate the channels of a file together (multichannel WPE, channels * taps <= 32), not one by one; "
                         "with --live the recursive joint form (forget >= 1 - 1 / (2 channels taps))")
    ap.add_argument("--live", action="store_true",
                    help="push the file (not a folder) through the streaming form (recursive WPE) at its own rate, as a live feed arrives")
    ap.add_argument("--chunk", type=int, default=1024, help="with --live: samples per push, at the file's rate")
    ap.add_argument("--block", type=int, default=4, help="with --live: frames per step (latency (block - 1) hop + n_fft samples)")
    ap.add_argument("--forget", type=float, default=WpeStreamParams.forget, help="with --live: forgetting factor, 0.95 ... 1")
    args = ap.parse_args(argv)
    taps = WpeParams.taps if args.taps is None else args.taps
    if args.live:
        if args.chunk < 1 or args.block < 1:
            ap.error("--chunk and --block must be >= 1")
        if os.path.isdir(args.src):
            ap.error("--live takes one wav file")

        def make(dev, n_streams, rate):
            channels = n_streams if args.joint else 1            # --joint: the wav's channels are one recording
            if not 1 <= channels <= 8:
                raise ValueError(f"--joint: {channels} channels; the joint form takes 1 ... 8")
            k = 32 // channels if args.joint and args.taps is None else taps
            params = WpeStreamParams(taps=k, delay=args.delay, forget=args.forget)
            return StreamDereverberator(dev, n_streams=n_streams, block_frames=args.block, params=params, gain=args.gain, input_rate=rate,
                                        channels=channels)
        try:
            return run_live(make, args.src, args.dst, args.chunk, args.reference, per_channel=args.joint)
        except ValueError as exc:
            ap.error(str(exc))
    try:
        params = WpeParams(taps=taps, delay=args.delay, iterations=args.iterations)
    except ValueError as exc:
        ap.error(str(exc))
    # --joint without --taps: 32 // channels of each file
    dn = Dereverberator(params=params, gain=args.gain, channels="joint" if args.joint else "separate",
                        joint_default_taps=args.taps is None)
    try:
        return run_files(dn, args.src, args.dst, args.reference)
    except ValueError as exc:
        ap.error(str(exc))


if __name__ == "__main__":
    raise SystemExit(main())
