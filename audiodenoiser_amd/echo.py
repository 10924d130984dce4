"""Acoustic echo cancellation: what the loudspeaker played, taken out of the microphone.  No checkpoint needed.

    from audiodenoiser_amd.echo import EchoCanceller, AecParams, aec_online
    ec = EchoCanceller()                               # no model: the current ROCm device, 8 kHz, n_fft 512, hop 128
    near = ec.cancel(mic, far, sr=48000)               # (L,) or (N, L), numpy -> numpy, tensor -> tensor, any rate
    ec.cancel_file("mic.wav", "far.wav", "out.wav")
    EchoCanceller(gain=True)                           # then the Wiener gain of the spectral baseline: residual echo and noise
    e, mag, state = aec_online(mic_spec, far_spec)     # the operator on spectrograms

    python -m audiodenoiser_amd.echo MIC.wav FAR.wav OUT.wav [--reference NEAR.wav] [--taps K] [--delay D] [--forget A] [--gain]
    python -m audiodenoiser_amd.echo MIC.wav FAR.wav OUT.wav --live [--chunk N] [--block B] [--taps K] [--delay D] [--forget A] [--gain]
    python -m audiodenoiser_amd.echo MIC.wav FAR.wav OUT.wav --refs Q [--live] ...     # FAR.wav has Q channels: stereo, surround

The operator is DEFINED in ``include/adn_echo.h`` ("echo stream"; float64 restatement: ``tests/echo_ref.py``;
``csrc/echo_stream_kernels.hip``; its three entry points are ``libadn_echo.so``'s, a library beside ``libadn.so`` built with it, and
the pool form's is ``libadn_call.so``'s, ``include/adn_call.h``) and is
unpinned against any package: per (pair, bin) an exponentially forgetting RLS filter of
``taps`` STFT frames from the far-end reference ``R`` to the microphone ``Y``, ``e_t = Y_t - sum_j conj(h_j) R_{t-D-j}``, updated
once per frame -- except on a frame whose far-end power is at most ``quiet``, which leaves the filter untouched: a silent far end is
the normal state of a call.  There is no variance weighting and no double-talk detector.  ``loading`` and ``quiet`` are absolute
powers: the operator is not scale invariant, and the defaults suit audio at a peak of about 0.5.

``EchoCanceller`` is ``Denoiser`` with this in the network's place:

1. both inputs resampled to the working rate, as ``Denoiser`` does;
2. ``adn_stft_complex`` of both, ``T = 1 + L // hop`` frames;
3. ``adn_aec_online``: ``e`` and its magnitudes into a zeroed ``(n, 1, F, max(T, 16))`` buffer;
4. with ``gain=True`` ``adn_spectral_gain`` on ``e`` writes the magnitudes instead (``gain_params``);
5. ``adn_denoise_resynth`` with one window per clip and the phase of ``e``; resampled back, the input's sample count.

The live form is ``StreamEchoCanceller``: ``StreamDenoiser`` over ``n_streams = 2 * pairs`` feeds, stream ``2 g`` the microphone and
``2 g + 1`` the far end of pair ``g``, with ``adn_aec_stream`` between ``analyze`` and ``emit`` in place on the analysed windows
(and with ``gain=True`` then ``adn_spectral_gain_windows`` on the kept columns); the object keeps row ``2 g`` of each pair.

    se = StreamEchoCanceller(pairs=1)                  # 8 kHz, block of 4 frames
    near = se.push(block)                              # (2, m): microphone, far end -> (k,): what has become final
    tail = se.flush()

The pool form is ``EchoStreamPool``: ``StreamPool`` over CALLS of ``mics`` microphones that share one far end, calls that open,
stall and hang up on their own clocks, the ready ones batched into one ``adn_aec_stream_pool`` launch per tick; only the
microphone rows are resynthesised.  With ``mics=1`` a call is the pair above, bit for bit.

    pool = EchoStreamPool(max_calls=64, mics=1)        # or mics=4: a speakerphone, one loudspeaker
    cid = pool.open()                                  # or open(input_rate=48000) with input_rates=(48000,)
    pool.push(cid, block)                              # (mics + 1, m): the microphones first, the far end last
    for cid, near, finished in pool.step(): ...        # (k,), or (mics, k) for mics > 1
    pool.close(cid)

A stereo or surround far end -- ``Q`` loudspeakers, ``Q`` rooms, one microphone -- is ``refs=Q`` (2 ... 8): ONE filter of ``Q *
taps`` taps over all ``Q`` references ("echo stream multireference" of ``include/adn_call.h``; float64 restatement
``tests/echo_mr_ref.py``; ``csrc/call/echo_mr_kernels.hip``; ``adn_aec_mr_online`` and ``adn_aec_mr_stream`` of ``libadn_call.so``).
``refs * taps <= 32``, and ``params=None`` then means ``16 // Q`` taps per channel: on the host recipe a stacked filter of 32
unknowns misadjusts in double talk at ``forget`` 0.995 (``profiles/bench_echo_mr.md``).

    ec = EchoCanceller(refs=2)
    near = ec.cancel(mic, far)                         # mic (L,) | (N, L), far (2, L) | (N, 2, L)
    se = StreamEchoCanceller(pairs=1, refs=2)          # three feeds: the microphone, left, right
    near = se.push(block)                              # (3, m) -> (k,)
    e, mag, state = aec_mr_online(mic_spec, far_spec, 2)   # far_spec (n_rows, 2, T, F)

A reference channel that stays digitally silent while another plays is not protected by the gate and winds its block of ``P`` up
(``include/adn_call.h``): a caller with a mono signal uses ``refs=1``.

The defaults (8 taps, no delay, forget 0.995, loading 10, quiet 1e-8) are the values of the host prototype
(``profiles/bench_echo.md``); they were not tuned by ear.

What is NOT here: pools that mix ``mics``; a lockstep object with several microphones per far end; echo cancellation chained into
``BeamformStreamPool``; more than one reference channel in ``EchoStreamPool``; a guard against the wind-up of a reference that stays
silent while others play; more than 32 stacked taps; partitioned time-domain filters;
double-talk detectors; non-linear echo; any tuning by ear.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib
from ._host import check_stft_plan, current_stream, report, rocm_device, run_files, stage
from .baseline import SpectralParams, _gain_kept_columns, _spectral_params, spectral_gain
from .denoise import Denoiser
from .dereverb import _mag_buffer, _need_cells, _spec_dims
from .griffin_lim import stft_complex
from .resample import _resample_device
from .stream import POOL_MAX_ROWS, RecordingBook, StreamDenoiser, StreamPool, _check_stream_args, causal_carrier
from .wav import read_wav, write_wav

__all__ = ["AecParams", "aec_stream_state_bytes", "aec_pool_state_bytes", "aec_online", "EchoCanceller", "StreamEchoCanceller",
           "EchoStreamPool", "aec_mr_state_bytes", "aec_mr_online"]

MAX_REFS = 8                                                 # ADN_CALL_MAX_REFS of include/adn_call.h


@dataclasses.dataclass(frozen=True)
class AecParams:
    """``adn_aec_params`` of ``include/adn_echo.h`` ("echo stream") with its defaults and its legal ranges.  ``loading`` and ``quiet`` are
    absolute powers of STFT values; the defaults are the host prototype's and were not tuned by ear."""
    taps: int = 8
    delay: int = 0
    forget: float = 0.995
    loading: float = 10.0
    quiet: float = 1e-8

    def __post_init__(self):
        for name, lo, hi in (("taps", 1, 32), ("delay", 0, 8)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"AecParams: need an integer {lo} <= {name} <= {hi}")
        # the ranges hold for the fp32 values the library sees; a NaN fails every comparison
        for name, lo, hi in (("forget", 0.95, 1.0), ("loading", 1e-3, 1e6), ("quiet", 0.0, 1.0)):
            v = float(getattr(self, name))
            f32 = ctypes.c_float(v).value
            if not lo <= v <= hi or not ctypes.c_float(lo).value <= f32 <= ctypes.c_float(hi).value:
                raise ValueError(f"AecParams: need {lo:g} <= {name} <= {hi:g}")
        if not 2.0 * self.taps * (1.0 - ctypes.c_float(float(self.forget)).value) <= 1.0:
            raise ValueError(f"AecParams: need 2 taps (1 - forget) <= 1: forget >= {1 - 1 / (2 * self.taps):.6f} at taps = {self.taps} "
                             f"(forget {self.forget})")

    def to_struct(self) -> "_lib.AecParamsStruct":
        return _lib.AecParamsStruct(int(self.taps), int(self.delay), float(self.forget), float(self.loading), float(self.quiet))


def _aec_params(who, params):
    if params is not None and not isinstance(params, AecParams):
        raise TypeError(f"{who}: params must be an AecParams")
    return ctypes.byref(params.to_struct()) if params is not None else None


def aec_stream_state_bytes(n_slots: int, n_bins: int, params: AecParams = None) -> int:
    """``adn_aec_stream_state_bytes``: the bytes of the opaque state of ``n_slots`` pairs of ``n_bins`` bins (no device needed)."""
    need = ctypes.c_size_t(0)
    _lib.check_echo(_lib.load_echo().adn_aec_stream_state_bytes(n_slots, n_bins, _aec_params("aec_stream_state_bytes", params), ctypes.byref(need)),
               "adn_aec_stream_state_bytes")
    return int(need.value)


def _check_mics(who, mics):
    if isinstance(mics, bool) or not isinstance(mics, int) or not 1 <= mics <= 7:
        raise ValueError(f"{who}: need an integer 1 <= mics <= 7 (a call is mics + 1 <= 8 streams)")


def aec_pool_state_bytes(max_calls: int, mics: int, n_bins: int, params: AecParams = None) -> int:
    """The bytes of the echo state of an ``adn_aec_stream_pool`` over ``max_calls`` calls of ``mics`` microphones: a slot per
    microphone, ``aec_stream_state_bytes(max_calls * mics, n_bins, params)`` (no device needed)."""
    _check_mics("aec_pool_state_bytes", mics)
    if isinstance(max_calls, bool) or not isinstance(max_calls, int) or max_calls < 1:
        raise ValueError("aec_pool_state_bytes: need an integer max_calls >= 1")
    return aec_stream_state_bytes(max_calls * mics, n_bins, params)


def aec_online(mic_spec: torch.Tensor, far_spec: torch.Tensor, state: torch.Tensor = None, first_frame: int = 0,
               params: AecParams = None, mag_out: torch.Tensor = None, col0: int = 0):
    """``adn_aec_online`` on the current stream.  ``mic_spec``, ``far_spec``: complex64 ``(n_rows, T, F)`` on one ROCm device, the
    frames ``first_frame ... first_frame + T - 1`` of the microphone and of the far end of every row.  ``state``: the uint8 tensor an
    earlier call returned for the frames before them (None allocates one; with ``first_frame = 0`` every row starts fresh whatever it
    holds); it is updated IN PLACE.  ``mag_out``: float32 ``(n_rows, 1, F, width)`` whose columns ``[col0, col0 + T)`` are written
    and nothing else; None allocates ``(n_rows, 1, F, T)``.  Returns ``(e, mag_out, state)``, ``e`` a new complex64 tensor of
    ``mic_spec``'s shape."""
    who = "aec_online"
    n, t, f = _spec_dims(who, "row", mic_spec)
    if (not isinstance(far_spec, torch.Tensor) or far_spec.dtype != torch.complex64 or far_spec.shape != mic_spec.shape
            or far_spec.device != mic_spec.device):
        raise ValueError(f"{who}: far_spec must be a complex64 tensor of mic_spec's shape on its device")
    p = _aec_params(who, params)
    _need_cells(who, "row", n, t, f)
    if not (isinstance(first_frame, int) and first_frame >= 0 and isinstance(col0, int) and col0 >= 0):
        raise ValueError(f"{who}: need integers first_frame >= 0 and col0 >= 0")
    dev = mic_spec.device
    need = aec_stream_state_bytes(n, f, params)
    if state is None:
        if first_frame != 0:
            raise ValueError(f"{who}: first_frame > 0 continues a row: pass the state of the call before")
        state = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif (not isinstance(state, torch.Tensor) or not state.is_cuda or state.device != dev or state.dtype != torch.uint8
          or state.dim() != 1 or state.numel() < need or not state.is_contiguous()):
        raise ValueError(f"{who}: state must be a contiguous uint8 tensor of at least aec_stream_state_bytes on mic_spec's device")
    if mag_out is None and col0 != 0:
        raise ValueError(f"{who}: col0 needs a mag_out buffer")
    mag_out = _mag_buffer(who, "row", mag_out, n, t, f, dev)
    if mag_out.shape[3] < col0 + t:
        raise ValueError(f"{who}: mag_out must hold columns [col0, col0 + n_frames)")
    m, r = torch.view_as_real(mic_spec.contiguous()), torch.view_as_real(far_spec.contiguous())
    out = torch.empty((n, t, f, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check_echo(_lib.load_echo().adn_aec_online(m.data_ptr(), r.data_ptr(), n, t, f, first_frame, p, state.data_ptr(), state.numel(), n,
                                              out.data_ptr(), mag_out.data_ptr(), int(mag_out.shape[3]), col0, current_stream(dev)),
                   "adn_aec_online")
    return torch.view_as_complex(out), mag_out, state


def _check_refs(who, refs):
    if isinstance(refs, bool) or not isinstance(refs, int) or not 1 <= refs <= MAX_REFS:
        raise ValueError(f"{who}: need an integer 1 <= refs <= {MAX_REFS} (far-end reference channels)")


def _mr_params(who, refs, params):
    """The checks of "echo stream multireference" on top of ``AecParams``' own: ``refs`` and the two rules on ``N = refs * taps``.
    ``params=None`` is the header's default, 8 taps for one reference and ``16 // refs`` per channel for more."""
    _check_refs(who, refs)
    p = _aec_params(who, params)
    taps = params.taps if params is not None else mr_default_taps(refs)
    forget = ctypes.c_float(float(params.forget if params is not None else AecParams.forget)).value
    if refs * taps > 32:
        raise ValueError(f"{who}: need refs * taps <= 32 (taps is per reference channel; refs {refs}, taps {taps})")
    if not 2.0 * refs * taps * (1.0 - forget) <= 1.0:
        raise ValueError(f"{who}: need 2 refs taps (1 - forget) <= 1: forget >= {1 - 1 / (2 * refs * taps):.6f} at refs * taps = {refs * taps}")
    return p


def mr_default_taps(refs: int) -> int:
    """The taps per channel ``params=None`` means with ``refs`` references (``include/adn_call.h``): 8, then ``16 // refs``."""
    return 8 if refs == 1 else 16 // refs


def aec_mr_state_bytes(n_slots: int, n_bins: int, refs: int, params: AecParams = None) -> int:
    """``adn_aec_mr_state_bytes``: the bytes of the opaque state of ``n_slots`` groups of one microphone and ``refs`` far-end channels,
    ``n_bins`` bins (no device needed).  With ``refs = 1`` it is ``aec_stream_state_bytes``."""
    need = ctypes.c_size_t(0)
    p = _mr_params("aec_mr_state_bytes", refs, params)
    _lib.check_call(_lib.load_call().adn_aec_mr_state_bytes(n_slots, n_bins, refs, p, ctypes.byref(need)), "adn_aec_mr_state_bytes")
    return int(need.value)


def aec_mr_online(mic_spec: torch.Tensor, far_spec: torch.Tensor, refs: int, state: torch.Tensor = None, first_frame: int = 0,
                  params: AecParams = None, mag_out: torch.Tensor = None, col0: int = 0):
    """``adn_aec_mr_online`` on the current stream: ``aec_online`` with ``refs`` far-end channels per row, ONE filter of ``refs *
    taps`` taps over all of them ("echo stream multireference", ``include/adn_call.h``).  ``mic_spec``: complex64 ``(n_rows, T, F)``;
    ``far_spec``: complex64 ``(n_rows, refs, T, F)`` on the same device.  ``state``, ``first_frame``, ``mag_out`` and ``col0`` are
    ``aec_online``'s, the state sized by ``aec_mr_state_bytes``.  Returns ``(e, mag_out, state)``.  With ``refs = 1`` the result and
    the state are ``aec_online``'s bits."""
    who = "aec_mr_online"
    p = _mr_params(who, refs, params)
    n, t, f = _spec_dims(who, "row", mic_spec)
    if (not isinstance(far_spec, torch.Tensor) or far_spec.dtype != torch.complex64 or far_spec.shape != (n, refs, t, f)
            or far_spec.device != mic_spec.device):
        raise ValueError(f"{who}: far_spec must be a complex64 tensor (n_rows, refs, T, F) = {(n, refs, t, f)} on mic_spec's device")
    _need_cells(who, "row", n * refs, t, f)
    if not (isinstance(first_frame, int) and first_frame >= 0 and isinstance(col0, int) and col0 >= 0):
        raise ValueError(f"{who}: need integers first_frame >= 0 and col0 >= 0")
    dev = mic_spec.device
    need = aec_mr_state_bytes(n, f, refs, params)
    if state is None:
        if first_frame != 0:
            raise ValueError(f"{who}: first_frame > 0 continues a row: pass the state of the call before")
        state = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif (not isinstance(state, torch.Tensor) or not state.is_cuda or state.device != dev or state.dtype != torch.uint8
          or state.dim() != 1 or state.numel() < need or not state.is_contiguous()):
        raise ValueError(f"{who}: state must be a contiguous uint8 tensor of at least aec_mr_state_bytes on mic_spec's device")
    if mag_out is None and col0 != 0:
        raise ValueError(f"{who}: col0 needs a mag_out buffer")
    mag_out = _mag_buffer(who, "row", mag_out, n, t, f, dev)
    if mag_out.shape[3] < col0 + t:
        raise ValueError(f"{who}: mag_out must hold columns [col0, col0 + n_frames)")
    m, r = torch.view_as_real(mic_spec.contiguous()), torch.view_as_real(far_spec.contiguous())
    out = torch.empty((n, t, f, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check_call(_lib.load_call().adn_aec_mr_online(m.data_ptr(), r.data_ptr(), n, refs, t, f, first_frame, p, state.data_ptr(),
                                                           state.numel(), n, out.data_ptr(), mag_out.data_ptr(), int(mag_out.shape[3]),
                                                           col0, current_stream(dev)), "adn_aec_mr_online")
    return torch.view_as_complex(out), mag_out, state


class EchoCanceller(Denoiser):
    """``Denoiser`` with the echo canceller in the network's place: no model, two inputs, the phase of the cancelled spectrum.
    ``gain=True`` runs the spectral baseline's Wiener gain (``gain_params``) on the result: residual-echo and noise suppression.
    ``refs=Q`` (2 ... 8) is a stereo or surround far end: ``cancel`` then takes the ``Q`` loudspeaker signals of every microphone
    and runs ``adn_aec_mr_online``, one filter of ``Q * taps`` taps over all of them; ``params=None`` then means ``16 // Q`` taps per
    channel."""

    def __init__(self, device=None, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128, params: AecParams = None,
                 gain: bool = False, gain_params: SpectralParams = None, refs: int = 1):
        check_stft_plan("EchoCanceller", n_fft, hop_length, sample_rate)
        _mr_params("EchoCanceller", refs, params)
        self.params, self.refs = params, refs
        self.gain = bool(gain)
        self.gain_params = _spectral_params("EchoCanceller", gain_params, "gain_params")
        self.model = None
        self._setup(rocm_device("EchoCanceller", device), sample_rate, n_fft, hop_length, "cancelled")

    def _core(self, x: torch.Tensor, rand=None) -> torch.Tensor:
        raise RuntimeError("EchoCanceller: two inputs are needed; call cancel(mic, far)")

    def _cancel_core(self, mic: torch.Tensor, far: torch.Tensor) -> torch.Tensor:
        """``mic``, ``far`` (n_clips, L) at the working rate -> (n_clips, L)."""
        n, length = mic.shape
        spec = stft_complex(torch.cat([mic, far.reshape(-1, length)]), self.n_fft, self.hop_length)
        t, f = spec.shape[1], spec.shape[2]
        y = torch.zeros((n, 1, f, max(t, 16)), dtype=torch.float32, device=mic.device)
        if self.refs == 1:
            e, _, _ = aec_online(spec[:n], spec[n:], None, 0, self.params, y, 0)
        else:                                                # far (n_clips, refs, L): the references of a clip follow each other
            e, _, _ = aec_mr_online(spec[:n], spec[n:].reshape(n, self.refs, t, f), self.refs, None, 0, self.params, y, 0)
        if self.gain:
            spectral_gain(e, self.gain_params, None, y, 0)
        return self._resynth(y, e, length, int(y.shape[3]), 0)

    def cancel(self, mic, far, sr=None):
        """``mic`` and ``far`` float32 of one shape, ``(L,)`` or ``(N, L)``, at rate ``sr`` (default: the working rate): the
        microphone and what the loudspeaker played -> the microphone without the echo, same shape, rate and sample count.  numpy in
        -> numpy out, tensors on the ROCm device in -> a tensor there out.  With ``refs = Q >= 2`` ``far`` holds the ``Q`` loudspeaker
        signals of every microphone: ``(Q, L)`` for ``mic (L,)``, ``(N, Q, L)`` for ``mic (N, L)``."""
        a, is_np = stage("EchoCanceller.cancel", mic, self.device)
        b, _ = stage("EchoCanceller.cancel", far, self.device, "far")
        Q = self.refs
        if Q == 1:
            if a.shape != b.shape or a.dim() not in (1, 2) or min(a.shape) < 1:
                raise ValueError("EchoCanceller.cancel: mic and far must have one shape, (L,) or (N, L), with at least one sample")
        elif a.dim() not in (1, 2) or min(a.shape) < 1 or tuple(b.shape) != tuple(a.shape[:-1]) + (Q, a.shape[-1]):
            raise ValueError(f"EchoCanceller.cancel: with refs = {Q}, mic must be (L,) or (N, L) with at least one sample and far "
                             f"(refs, L) or (N, refs, L)")
        single = a.dim() == 1
        x, r = (v[None] if single else v for v in (a.contiguous(), b.contiguous()))
        rate = self.sample_rate if sr is None else int(sr)
        length = x.shape[1]
        if rate != self.sample_rate:
            far_low = _resample_device(r.reshape(-1, length), rate, self.sample_rate)
            low = self._cancel_core(_resample_device(x, rate, self.sample_rate), far_low.reshape(r.shape[:-1] + far_low.shape[-1:]))
            up = _resample_device(low, self.sample_rate, rate)
            if up.shape[1] >= length:
                out = up[:, :length].contiguous()
            else:
                out = torch.zeros_like(x)
                out[:, :up.shape[1]] = up
        else:
            out = self._cancel_core(x, r)
        out = out[0] if single else out
        return out.cpu().numpy() if is_np else out

    def denoise(self, audio, sr=None, rand=None):
        raise RuntimeError("EchoCanceller: two inputs are needed; call cancel(mic, far)")

    def denoise_file(self, src, dst, subtype: str = "PCM_16"):
        raise RuntimeError("EchoCanceller: two inputs are needed; call cancel_file(mic_wav, far_wav, out_wav)")

    def cancel_file(self, mic_wav, far_wav, out_wav, subtype: str = "PCM_16"):
        """``read_wav`` of both (one rate, one channel count; the shorter one is padded with silence), every channel a pair ->
        ``cancel`` at the files' rate -> ``write_wav(out_wav)``.  Returns ``(n_samples, sample_rate)``.  With ``refs = Q >= 2`` the far
        wav must have ``Q`` channels, and they are the references of EVERY microphone channel."""
        if self.refs == 1:
            mic, far, rate = _read_pair("EchoCanceller.cancel_file", mic_wav, far_wav)
        else:
            mic, far, rate = _read_group("EchoCanceller.cancel_file", mic_wav, far_wav, self.refs)
            far = np.ascontiguousarray(np.broadcast_to(far, (mic.shape[0],) + far.shape))
        out = self.cancel(mic, far, sr=rate)
        write_wav(out_wav, np.ascontiguousarray(out.T), rate, subtype)
        return int(mic.shape[1]), int(rate)


def _read_pair(who, mic_wav, far_wav):
    """-> mic, far ``(channels, L)`` float32 and the rate: ``L`` is the microphone's, the far end cut or padded with silence to it."""
    mic, rate = read_wav(mic_wav, mono=False)                # (L, channels)
    far, far_rate = read_wav(far_wav, mono=False)
    if rate != far_rate:
        raise ValueError(f"{who}: {mic_wav} is at {rate} Hz, {far_wav} at {far_rate} Hz")
    if far.shape[1] != mic.shape[1]:
        if far.shape[1] != 1:
            raise ValueError(f"{who}: {far_wav} must have one channel or as many as {mic_wav}")
        far = np.repeat(far, mic.shape[1], axis=1)
    length = mic.shape[0]
    fit = np.zeros((length, mic.shape[1]), np.float32)
    fit[:min(length, far.shape[0])] = far[:length]
    return np.ascontiguousarray(mic.T, dtype=np.float32), np.ascontiguousarray(fit.T), int(rate)


def _read_group(who, mic_wav, far_wav, refs):
    """-> mic ``(channels, L)``, far ``(refs, L)`` float32 and the rate: the far wav's ``refs`` channels, cut or padded with silence
    to the microphone's length."""
    mic, rate = read_wav(mic_wav, mono=False)                # (L, channels)
    far, far_rate = read_wav(far_wav, mono=False)
    if rate != far_rate:
        raise ValueError(f"{who}: {mic_wav} is at {rate} Hz, {far_wav} at {far_rate} Hz")
    if far.shape[1] != refs:
        raise ValueError(f"{who}: with refs = {refs}, {far_wav} must have {refs} channels (it has {far.shape[1]})")
    length = mic.shape[0]
    fit = np.zeros((length, refs), np.float32)
    fit[:min(length, far.shape[0])] = far[:length]
    return np.ascontiguousarray(mic.T, dtype=np.float32), np.ascontiguousarray(fit.T), int(rate)


class StreamEchoCanceller(StreamDenoiser):
    """``StreamDenoiser`` with the echo canceller in the network's place over ``n_streams = 2 * pairs`` feeds: stream ``2 g`` is
    the microphone and ``2 g + 1`` the far end of pair ``g``.  ``push`` and ``flush`` take ``(2 * pairs, m)`` and return
    ``(pairs, k)``, or ``(k,)`` for one pair; ``reset``, ``received``, ``emitted``, ``latency_samples`` and ``input_rate`` are the
    parent's, and so are its guarantees: any cut into pushes gives the same bits, and a pair does not depend on its neighbours.

    The operator is causal, so ``lookahead_frames`` is 0 and ``window_frames = max(16, block_frames)`` is only the carrier the
    stream geometry needs.  Each run of steps calls ``adn_aec_stream`` in place on the analysed windows -- ``e`` into the microphone
    streams' frames, ``|e|`` into the ``block_frames`` columns ``adn_stream_emit`` reads, nothing of a far-end stream touched -- and
    with ``gain=True`` then ``adn_spectral_gain_windows`` on the kept columns (``gain_params``; it runs on every row with a state
    per stream, rows are independent there, so a microphone row is bit for bit what the gain gives on its windows alone).
    ``adn_stream_emit`` resynthesises every stream and row ``2 g`` of each pair is kept.  The echo state needs no reset: a stream's
    frame 0 starts it afresh; ``reset`` forgets the gain's noise estimates.

    ``refs=Q`` (2 ... 8) is a stereo or surround far end: ``n_streams = pairs * (Q + 1)`` feeds, in each group the microphone first
    and its ``Q`` loudspeaker signals after it; ``push`` and ``flush`` take ``(pairs * (Q + 1), m)`` and return ``(pairs, k)`` or
    ``(k,)`` as before, the operator is ``adn_aec_mr_stream`` (``include/adn_call.h``) and the kept rows are ``g (Q + 1)``."""

    def __init__(self, device=None, pairs: int = 1, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128,
                 block_frames: int = 4, params: AecParams = None, gain: bool = False, gain_params: SpectralParams = None,
                 input_rate=None, refs: int = 1):
        who = "StreamEchoCanceller"
        if isinstance(pairs, bool) or not isinstance(pairs, int) or pairs < 1:
            raise ValueError(f"{who}: need an integer pairs >= 1")
        _mr_params(who, refs, params)
        n_streams = (refs + 1) * pairs
        window, ahead, batch = causal_carrier(block_frames)
        _check_stream_args(who, n_streams, sample_rate, n_fft, hop_length, window, block_frames, ahead, batch, input_rate)
        self.params, self.pairs, self.gain, self.refs = params, pairs, bool(gain), refs
        self.gain_params = _spectral_params(who, gain_params, "gain_params")
        dev = rocm_device(who, device)
        self.model = None
        f = n_fft // 2 + 1
        need = aec_stream_state_bytes(pairs, f, params) if refs == 1 else aec_mr_state_bytes(pairs, f, refs, params)
        self._aec_state = torch.empty((need,), dtype=torch.uint8, device=dev)
        self._gain_state = torch.empty((n_streams, 3, f), dtype=torch.float32, device=dev)
        self._setup(dev, n_streams, sample_rate, n_fft, hop_length, window, block_frames, ahead, batch, input_rate)

    def reset(self):
        """Forget the running call, the gain's noise estimates included: the object is ready for a new one."""
        super().reset()
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("StreamEchoCanceller: there is no network; the canceller runs between analyze and emit (adn_aec_stream)")

    def _cancel(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        """``adn_aec_stream`` in place on the windows ``x`` and on the microphone streams' ring cells."""
        p = ctypes.byref(self.params.to_struct()) if self.params is not None else None
        with torch.cuda.device(self.device):
            if self.refs == 1:
                _lib.check_echo(_lib.load_echo().adn_aec_stream(self._state.data_ptr(), self._state.numel(), x.data_ptr(), self.n_streams, first_step,
                                                      n_steps, final_length, *self._plan, self.max_steps, p, self._aec_state.data_ptr(),
                                                      self._aec_state.numel(), current_stream(self.device)), "adn_aec_stream")
            else:
                _lib.check_call(_lib.load_call().adn_aec_mr_stream(self._state.data_ptr(), self._state.numel(), x.data_ptr(), self.n_streams,
                                                                   self.refs, first_step, n_steps, final_length, *self._plan, self.max_steps,
                                                                   p, self._aec_state.data_ptr(), self._aec_state.numel(),
                                                                   current_stream(self.device)), "adn_aec_mr_stream")
        return x

    def _net(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        self._cancel(x, first_step, n_steps, final_length)
        if self.gain:
            _gain_kept_columns(x, None, n_steps, self._gain_state, self._plan, self.gain_params)
        return x

    def _result(self, outs):
        """Row ``g (refs + 1)`` of every group of what the streams returned: ``(pairs, k)``, or ``(k,)`` for one pair."""
        out = self._cat(outs)[::self.refs + 1]
        out = out[0] if out.shape[0] == 1 else out.contiguous()
        return out.cpu().numpy() if self._numpy else out


class EchoStreamPool(StreamPool):
    """``StreamPool`` over CALLS with the echo canceller in the network's place: a call is ``mics`` microphones and the ONE far end
    they share, ``mics + 1`` streams; calls open, stall, close and run at their own rates, and a tick batches whatever is ready
    into one launch per kernel.

        pool = EchoStreamPool(max_calls=64, mics=4)
        cid = pool.open()                                  # or open(input_rate=48000) with input_rates=(48000,)
        pool.push(cid, block)                              # (5, m): the next samples of the four microphones, then of the far end
        for cid, near, finished in pool.step(): ...        # (4, k): what has become final of every microphone; (k,) for mics = 1

    Call ``c`` owns the stream slots ``c (mics + 1) ... c (mics + 1) + mics`` of the pool state, the far end the last one, and the
    slots ``c mics ... c mics + mics - 1`` of the echo state (``stream.RecordingBook`` with ``mics + 1`` channels;
    ``include/adn_call.h``, ``adn_aec_stream_pool``, a function of ``libadn_call.so``).  A tick analyses the ``mics + 1`` rows of
    every ready call, runs ``adn_aec_stream_pool`` in place on the windows, ``256 // (mics + 1)`` calls a library call, and drops
    the far-end windows; with ``gain=True`` then ``adn_spectral_gain_windows`` on the kept columns of the microphone rows
    (``gain_params``, a state per microphone, ``cid * mics + m``).  ``adn_stream_pool_emit`` -- and ``adn_stream_pool_emit_rate``
    for a call at an ``input_rate`` -- run on the microphone rows alone: the far end is pushed, ring-buffered and analysed once
    per call and never resynthesised, which is safe because an emit writes nothing but its own slot's overlap-add tail and only
    that slot's later emits read it.  The echo state needs no reset: a call's step 0 starts its pairs afresh.

    Claimed: every microphone of every call is, bit for bit, what a solo ``StreamEchoCanceller(pairs=1, input_rate=...)`` with the
    same parameters returns for that microphone and the call's far end, whatever its neighbours do; a call returns as many samples
    as came in; a call's slots are reusable without a reset.  Not claimed: pools that mix ``mics``; more than one step per call
    and tick; graph capture of a tick; anything ``StreamEchoCanceller`` does not claim."""

    def __init__(self, device=None, max_calls: int = 16, mics: int = 1, backlog_steps: int = 4, sample_rate: int = 8000,
                 n_fft: int = 512, hop_length: int = 128, block_frames: int = 4, params: AecParams = None, gain: bool = False,
                 gain_params: SpectralParams = None, input_rates=None):
        who = "EchoStreamPool"
        _check_mics(who, mics)
        if isinstance(max_calls, bool) or not isinstance(max_calls, int) or max_calls < 1:
            raise ValueError(f"{who}: need an integer max_calls >= 1")
        window, ahead, _ = causal_carrier(block_frames)
        _aec_params(who, params)
        self.book = RecordingBook(max_calls, mics + 1, backlog_steps, n_fft, hop_length, window, block_frames, ahead, input_rates,
                                  sample_rate)
        self.params, self.mics, self.max_calls, self.gain = params, mics, max_calls, bool(gain)
        self.gain_params = _spectral_params(who, gain_params, "gain_params")
        dev = rocm_device(who, device)
        self.model = None
        self.batch_windows = POOL_MAX_ROWS
        f = n_fft // 2 + 1
        self._aec_state = torch.empty((aec_pool_state_bytes(max_calls, mics, f, params),), dtype=torch.uint8, device=dev)
        self._gain_state = torch.empty((max_calls * mics, 3, f), dtype=torch.float32, device=dev)
        self._setup(dev)

    def reset(self):
        """Forget every call, the gain's noise estimates included: all slots are free."""
        super().reset()
        self._gain_state.fill_(-1.0)

    def network(self, x):
        raise RuntimeError("EchoStreamPool: there is no network; the canceller runs between analyze and emit (adn_aec_stream_pool)")

    def _mic_rows(self, rows):
        C = self.channels
        return [r for i, r in enumerate(rows) if i % C != C - 1]

    def _emit_rows(self, rows):
        """The microphone rows: the far end of a call is never resynthesised."""
        return self._mic_rows(rows)

    def _net(self, x: torch.Tensor, rows) -> torch.Tensor:
        """The tick's stream rows ``rows`` (``mics + 1`` per call) and their windows ``x`` -> the microphone windows, compacted,
        holding ``|e|`` (or the gain's result) in the kept columns."""
        L, C, M, plan = _lib.load_call(), self.channels, self.mics, self.book.plan
        lead = (self._state.data_ptr(), self._state.numel(), self._args[0], M) + self._args[1:]
        p = ctypes.byref(self.params.to_struct()) if self.params is not None else None
        per = POOL_MAX_ROWS // C * C                         # whole calls
        for i in range(0, len(rows), per):
            part, group = x[i:i + per], rows[i:i + per]
            with torch.cuda.device(self.device):
                _lib.check_call(L.adn_aec_stream_pool(*lead, self._rows(group), len(group), part.data_ptr(), p, self._aec_state.data_ptr(),
                                                      self._aec_state.numel(), current_stream(self.device)), "adn_aec_stream_pool")
        y = x.reshape(len(rows) // C, C, *x.shape[1:])[:, :M].reshape(-1, *x.shape[1:]).contiguous()
        if self.gain:                                        # a state per microphone: cid mics + m
            _gain_kept_columns(y, [(slot // C * M + slot % C, k, final) for slot, k, final in self._mic_rows(rows)], 1,
                               self._gain_state, plan, self.gain_params)
        return y


class _FilePair:
    """What ``_host.run_files`` drives: ``denoise_file(mic, out)`` with the far-end file fixed."""

    def __init__(self, ec, far_wav):
        self.ec, self.far_wav = ec, far_wav

    def denoise_file(self, src, dst):
        return self.ec.cancel_file(src, self.far_wav, dst)


def _run_live(args, params) -> int:
    """The two files pushed ``--chunk`` samples at a time, at their own rate, through a ``StreamEchoCanceller`` with a pair per
    channel.  (``_host.run_live`` reads ONE file whose channels are the streams; here the streams interleave two files.)"""
    refs = args.refs or 1
    if refs == 1:
        mic, far, rate = _read_pair("--live", args.mic, args.far)
        far = far[:, None]
    else:                                                    # the far wav's channels are the references of every microphone channel
        mic, far, rate = _read_group("--live", args.mic, args.far, refs)
        far = np.broadcast_to(far, (mic.shape[0],) + far.shape)
    dev = _lib.staging_device()
    pairs = mic.shape[0]
    x = torch.from_numpy(np.concatenate([mic[:, None], far], axis=1).reshape((refs + 1) * pairs, -1)).to(dev)
    se = StreamEchoCanceller(dev, pairs=pairs, block_frames=args.block, params=params, gain=args.gain, input_rate=rate, refs=refs)
    outs = [se.push(x[:, i:i + args.chunk]) for i in range(0, x.shape[1], args.chunk)]
    latency = se.latency_input_samples
    outs.append(se.flush())
    out = torch.cat(outs, dim=-1)
    write_wav(args.out, np.ascontiguousarray(out.cpu().numpy().T), rate)
    print(f"{args.mic} -> {args.out}: {x.shape[1]} samples at {rate} Hz in pushes of {args.chunk} at its own rate, latency {latency} samples")
    if args.reference is not None:
        print(report(args.mic, args.out, args.reference))
    return 0


def main(argv=None) -> int:
    import argparse
    import os
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.echo",
                                 description="Remove the far-end signal FAR.wav (what the loudspeaker played) from the microphone MIC.wav.")
    ap.add_argument("mic", metavar="MIC.wav", help="the microphone recording")
    ap.add_argument("far", metavar="FAR.wav", help="the far-end signal, at MIC's rate: one channel, or one per channel of MIC")
    ap.add_argument("out", metavar="OUT.wav", help="the wav file to write")
    ap.add_argument("--reference", metavar="NEAR.wav", default=None, help="the near-end signal alone: print one JSON line of metrics")
    ap.add_argument("--refs", type=int, default=None, metavar="Q",
                    help="a stereo or surround far end: FAR.wav has Q channels (1 ... 8), all of them the references of every channel of MIC")
    ap.add_argument("--taps", type=int, default=None,
                    help="filter length in STFT frames per reference channel, 1 ... 32 with refs * taps <= 32 (default 8; 16 // Q with --refs Q >= 2)")
    ap.add_argument("--delay", type=int, default=AecParams.delay, help="frames the echo lags the far end at least, 0 ... 8")
    ap.add_argument("--forget", type=float, default=AecParams.forget, help="forgetting factor, 0.95 ... 1 with 2 taps (1 - forget) <= 1")
    ap.add_argument("--gain", action="store_true", help="run the spectral baseline's Wiener gain on the result")
    ap.add_argument("--live", action="store_true", help="push the files through the streaming canceller at their own rate, as a call arrives")
    ap.add_argument("--chunk", type=int, default=1024, help="with --live: samples per push, at the files' rate")
    ap.add_argument("--block", type=int, default=4, help="with --live: frames per step (latency (block - 1) hop + n_fft samples)")
    args = ap.parse_args(argv)
    if os.path.isdir(args.mic) or os.path.isdir(args.far):
        ap.error("MIC.wav and FAR.wav are files")
    try:
        refs = 1 if args.refs is None else args.refs
        _check_refs("--refs", refs)
        params = AecParams(taps=mr_default_taps(refs) if args.taps is None else args.taps, delay=args.delay, forget=args.forget)
        if args.live:
            if args.chunk < 1 or args.block < 1:
                ap.error("--chunk and --block must be >= 1")
            return _run_live(args, params)
        return run_files(_FilePair(EchoCanceller(params=params, gain=args.gain, refs=refs), args.far), args.mic, args.out, args.reference)
    except ValueError as exc:
        ap.error(str(exc))


if __name__ == "__main__":
    raise SystemExit(main())
