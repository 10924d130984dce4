"""ctypes binding of libadn.so (include/adn.h).  There is no fallback: if the HIP library cannot be loaded
or built, every entry point raises."""
from __future__ import annotations

import ctypes
import os
import threading

from . import build as _build

_lock = threading.Lock()
_lib = None

c_float_p = ctypes.POINTER(ctypes.c_float)


class AdnError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load (building first if the in-tree library is missing or stale) libadn.so."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        variant = os.environ.get("ADN_LIBADN_PATH")       # variant sweeps of tools/ (build.build_variant); unset in production
        try:
            path = variant if variant else _build.build()
        except Exception as exc:  # noqa: BLE001 - re-raised with context
            raise AdnError(f"libadn.so (MI355X HIP kernels) is missing and could not be built: {exc}") from exc
        # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).  It must be
        # in the process BEFORE libadn.so is mapped so that libadn's NEEDED libamdhip64.so.7 binds to that same
        # runtime instance (streams and allocations are shared with torch); loading libadn first would pull in
        # /opt/rocm's copy and leave two HIP runtimes in one process.
        import torch  # noqa: F401
        try:
            L = ctypes.CDLL(path)
        except OSError as exc:
            raise AdnError(f"cannot load {path}: {exc}") from exc
        vp, sz, ci, cl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_long
        L.adn_version.restype = ci
        L.adn_last_error.restype = ctypes.c_char_p
        L.adn_device_count.argtypes = [ctypes.POINTER(ci)]
        L.adn_prepare.argtypes = [ci, ci]
        L.adn_unet_create.argtypes = [ctypes.POINTER(vp), ci, ctypes.POINTER(c_float_p), ci]
        L.adn_unet_create_ex.argtypes = [ctypes.POINTER(vp), ci, ctypes.POINTER(c_float_p), ci, ci]
        L.adn_unet_create_general.argtypes = [ctypes.POINTER(vp), ci, ctypes.POINTER(c_float_p), ci, ci, ci, ci]
        L.adn_unet_channels.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.adn_unet_set_batch_invariant.argtypes = [vp, ci]
        L.adn_unet_destroy.argtypes = [vp]
        L.adn_unet_workspace_bytes.argtypes = [vp, ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_unet_forward.argtypes = [vp, vp, vp, ci, ci, ci, vp, sz, vp]
        L.adn_unet_forward_taps.argtypes = [vp, vp, vp, ci, ci, ci, vp, sz, ctypes.POINTER(vp), vp]
        L.adn_unet_set_timing.argtypes = [vp, ci]
        L.adn_unet_get_timing.argtypes = [vp, ci, c_float_p]
        L.adn_stft_n_frames.argtypes = [cl, ci, ci, ci, ctypes.POINTER(cl)]
        L.adn_stft_mag.argtypes = [vp, ci, cl, ci, ci, ci, vp, vp]
        L.adn_stft_mag_fit.argtypes = [vp, ci, cl, ci, ci, ci, vp, ci, ci, vp]
        L.adn_quantize_pad.argtypes = [vp, ci, ci, ci, vp, ci, ci, vp]
        L.adn_per_clip_l1.argtypes = [vp, vp, ci, cl, vp, vp]
        L.adn_perceptual_loss_workspace_bytes.argtypes = [ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_perceptual_loss.argtypes = [vp, vp, ci, ci, ci, vp, sz, vp, vp]
        L.adn_perceptual_loss_backward_workspace_bytes.argtypes = [ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_perceptual_loss_backward.argtypes = [vp, vp, ci, ci, ci, vp, vp, sz, vp, vp, vp]
        L.adn_resample_length.argtypes = [cl, ci, ci, ctypes.POINTER(cl)]
        L.adn_resample_prepare.argtypes = [ci, ci, ci]
        L.adn_resample.argtypes = [vp, ci, cl, ci, ci, vp, vp]
        L.adn_mix_snr_workspace_bytes.argtypes = [ci, cl, ctypes.POINTER(sz)]
        L.adn_mix_snr.argtypes = [vp, vp, ci, cl, ctypes.c_float, vp, sz, vp, vp]
        cf = ctypes.c_float
        L.adn_reverb.argtypes = [vp, ci, cl, ci, cf, cf, cf, cf, cf, ci, vp, vp]
        L.adn_istft_length.argtypes = [ci, ci, ctypes.POINTER(cl)]
        L.adn_griffin_lim_workspace_bytes.argtypes = [ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_griffin_lim.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, sz, vp, vp]
        L.adn_stft_complex.argtypes = [vp, ci, cl, ci, ci, vp, vp]
        L.adn_istft_workspace_bytes.argtypes = [ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_istft.argtypes = [vp, ci, ci, ci, ci, vp, sz, vp, vp]
        L.adn_denoise_plan.argtypes = [ci, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.adn_denoise_windows.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp]
        L.adn_denoise_stitch.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp]
        L.adn_denoise_resynth.argtypes = [vp, vp, ci, cl, ci, ci, ci, ci, vp, vp]
        L.adn_stream_plan.argtypes = [ci, ci, ci, ci, ci, cl, ctypes.POINTER(cl), ctypes.POINTER(cl), ctypes.POINTER(cl)]
        L.adn_stream_state_bytes.argtypes = [ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_stream_reset.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, ci, vp]
        L.adn_stream_analyze.argtypes = [vp, sz, vp, cl, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, vp, vp]
        L.adn_stream_emit.argtypes = [vp, sz, vp, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, vp, cl, vp]
        L.adn_stream_pool_state_bytes.argtypes = [ci, ci, ci, ci, ci, ci, cl, ctypes.POINTER(sz)]
        L.adn_stream_pool_reset.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, cl, ci, vp]
        L.adn_stream_pool_write.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, cl, ci, vp, cl, cl, vp]
        L.adn_stream_pool_analyze.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, cl, vp, ci, vp, vp]
        L.adn_stream_pool_emit.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, cl, vp, ci, vp, vp, cl, vp]
        L.adn_resample_stream_plan.argtypes = [ci, ci, cl, ci, ctypes.POINTER(cl), ctypes.POINTER(cl), ctypes.POINTER(cl)]
        L.adn_resample_stream_state_bytes.argtypes = [ci, ci, ci, ctypes.POINTER(sz)]
        L.adn_resample_stream.argtypes = [vp, sz, vp, cl, ci, cl, cl, cl, ci, ci, ci, vp, cl, vp]
        L.adn_stream_pool_rate_state_bytes.argtypes = [ci, ci, ctypes.POINTER(sz)]
        L.adn_stream_pool_push_rate.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, cl, vp, sz, ci, ci, vp, ci, vp, vp]
        L.adn_stream_pool_emit_rate.argtypes = [vp, sz, ci, ci, ci, vp, ci, vp, cl, vp, cl, vp]
        L.adn_quality_workspace_bytes.argtypes = [ci, cl, ctypes.POINTER(sz)]
        L.adn_quality.argtypes = [vp, vp, vp, ci, cl, ci, vp, sz, vp, vp]
        L.adn_stoi_workspace_bytes.argtypes = [ci, cl, ctypes.POINTER(sz)]
        L.adn_stoi.argtypes = [vp, vp, vp, ci, cl, vp, sz, vp, vp]
        L.adn_spectral_gain.argtypes = [vp, ci, ci, ci, ctypes.POINTER(SpectralParamsStruct), vp, vp, vp, ci, ci, vp]
        L.adn_spectral_gain_windows.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(SpectralParamsStruct), vp, ci, vp, vp]
        L.adn_wpe_workspace_bytes.argtypes = [ci, ci, ci, ctypes.POINTER(WpeParamsStruct), ctypes.POINTER(sz)]
        L.adn_wpe.argtypes = [vp, ci, ci, ci, ctypes.POINTER(WpeParamsStruct), vp, sz, vp, vp, ci, vp]
        L.adn_wpe_mc_workspace_bytes.argtypes = [ci, ci, ci, ci, ctypes.POINTER(WpeParamsStruct), ctypes.POINTER(sz)]
        L.adn_wpe_mc.argtypes = [vp, ci, ci, ci, ci, ctypes.POINTER(WpeParamsStruct), vp, sz, vp, vp, ci, vp]
        wsp = ctypes.POINTER(WpeStreamParamsStruct)
        L.adn_wpe_stream_state_bytes.argtypes = [ci, ci, wsp, ctypes.POINTER(sz)]
        L.adn_wpe_online.argtypes = [vp, ci, ci, ci, cl, wsp, vp, sz, ci, vp, vp, ci, ci, vp]
        L.adn_wpe_stream.argtypes = [vp, sz, vp, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, wsp, vp, sz, vp]
        L.adn_wpe_stream_pool.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, cl, vp, ci, vp, wsp, vp, sz, vp]
        L.adn_wpe_mc_stream_state_bytes.argtypes = [ci, ci, ci, wsp, ctypes.POINTER(sz)]
        L.adn_wpe_mc_online.argtypes = [vp, ci, ci, ci, ci, cl, wsp, vp, sz, ci, vp, vp, ci, ci, vp]
        L.adn_wpe_mc_stream.argtypes = [vp, sz, vp, ci, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, wsp, vp, sz, vp]
        L.adn_wpe_mc_stream_pool.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, ci, cl, vp, ci, vp, wsp, vp, sz, vp]
        L.adn_mvdr_workspace_bytes.argtypes = [ci, ci, ci, ci, ctypes.POINTER(MvdrParamsStruct), ctypes.POINTER(sz)]
        L.adn_mvdr.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(MvdrParamsStruct), vp, sz, vp, vp, ci, vp]
        msp = ctypes.POINTER(MvdrStreamParamsStruct)
        L.adn_mvdr_stream_state_bytes.argtypes = [ci, ci, ci, msp, ctypes.POINTER(sz)]
        L.adn_mvdr_online.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, cl, msp, vp, sz, ci, vp, vp, ci, ci, vp]
        L.adn_mvdr_stream.argtypes = [vp, sz, vp, ci, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, msp, vp, sz, vp]
        L.adn_mvdr_stream_pool.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, ci, cl, vp, ci, vp, msp, vp, sz, vp]
        for name in ("adn_device_count", "adn_prepare", "adn_unet_create", "adn_unet_create_ex", "adn_unet_create_general", "adn_unet_channels",
                     "adn_unet_set_batch_invariant", "adn_unet_destroy", "adn_unet_workspace_bytes", "adn_unet_forward", "adn_unet_forward_taps", "adn_unet_set_timing", "adn_unet_get_timing",
                     "adn_stft_n_frames", "adn_stft_mag", "adn_stft_mag_fit", "adn_quantize_pad", "adn_per_clip_l1",
                     "adn_perceptual_loss_workspace_bytes", "adn_perceptual_loss", "adn_perceptual_loss_backward_workspace_bytes",
                     "adn_perceptual_loss_backward", "adn_resample_length", "adn_resample_prepare", "adn_resample",
                     "adn_mix_snr_workspace_bytes", "adn_mix_snr", "adn_reverb", "adn_istft_length",
                     "adn_griffin_lim_workspace_bytes", "adn_griffin_lim", "adn_stft_complex",
                     "adn_istft_workspace_bytes", "adn_istft",
                     "adn_denoise_plan", "adn_denoise_windows", "adn_denoise_stitch", "adn_denoise_resynth",
                     "adn_stream_plan", "adn_stream_state_bytes", "adn_stream_reset", "adn_stream_analyze", "adn_stream_emit",
                     "adn_stream_pool_state_bytes", "adn_stream_pool_reset", "adn_stream_pool_write", "adn_stream_pool_analyze",
                     "adn_stream_pool_emit",
                     "adn_resample_stream_plan", "adn_resample_stream_state_bytes", "adn_resample_stream",
                     "adn_stream_pool_rate_state_bytes", "adn_stream_pool_push_rate", "adn_stream_pool_emit_rate",
                     "adn_quality_workspace_bytes", "adn_quality", "adn_stoi_workspace_bytes", "adn_stoi",
                     "adn_spectral_gain", "adn_spectral_gain_windows", "adn_wpe_workspace_bytes", "adn_wpe",
                     "adn_wpe_mc_workspace_bytes", "adn_wpe_mc",
                     "adn_wpe_stream_state_bytes", "adn_wpe_online", "adn_wpe_stream", "adn_wpe_stream_pool",
                     "adn_wpe_mc_stream_state_bytes", "adn_wpe_mc_online", "adn_wpe_mc_stream", "adn_wpe_mc_stream_pool",
                     "adn_mvdr_workspace_bytes", "adn_mvdr",
                     "adn_mvdr_stream_state_bytes", "adn_mvdr_online", "adn_mvdr_stream", "adn_mvdr_stream_pool"):
            getattr(L, name).restype = ci
        _lib = L
        return L


_echo = None


def load_echo() -> ctypes.CDLL:
    """Load libadn_echo.so (include/adn_echo.h; built with libadn.so, which is loaded first: the stream state the echo canceller
    works on is that library's).  Its failed calls leave their message in ``adn_aec_last_error``: ``check_echo``."""
    global _echo
    load()
    with _lock:
        if _echo is not None:
            return _echo
        path = _build.ECHO_LIB
        if not os.path.exists(path):
            raise AdnError(f"{path} is missing: python -m audiodenoiser_amd.build")
        try:
            L = ctypes.CDLL(path)
        except OSError as exc:
            raise AdnError(f"cannot load {path}: {exc}") from exc
        vp, sz, ci, cl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_long
        asp = ctypes.POINTER(AecParamsStruct)
        L.adn_aec_last_error.restype = ctypes.c_char_p
        L.adn_aec_stream_state_bytes.argtypes = [ci, ci, asp, ctypes.POINTER(sz)]
        L.adn_aec_online.argtypes = [vp, vp, ci, ci, ci, cl, asp, vp, sz, ci, vp, vp, ci, ci, vp]
        L.adn_aec_stream.argtypes = [vp, sz, vp, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, asp, vp, sz, vp]
        for name in ECHO_EXPORTED_SYMBOLS[1:]:
            getattr(L, name).restype = ci
        _echo = L
        return L


def check_echo(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_echo().adn_aec_last_error()
        raise AdnError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")


_call = None


def load_call() -> ctypes.CDLL:
    """Load libadn_call.so (include/adn_call.h; built with the other two, which are loaded first: the pool state and the echo state
    it works on are theirs).  Its failed calls leave their message in ``adn_call_last_error``: ``check_call``."""
    global _call
    load_echo()
    with _lock:
        if _call is not None:
            return _call
        path = _build.CALL_LIB
        if not os.path.exists(path):
            raise AdnError(f"{path} is missing: python -m audiodenoiser_amd.build")
        try:
            L = ctypes.CDLL(path)
        except OSError as exc:
            raise AdnError(f"cannot load {path}: {exc}") from exc
        vp, sz, ci, cl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_long
        L.adn_call_last_error.restype = ctypes.c_char_p
        asp = ctypes.POINTER(AecParamsStruct)
        L.adn_aec_stream_pool.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, ci, cl, vp, ci, vp, asp, vp, sz, vp]
        L.adn_aec_mr_state_bytes.argtypes = [ci, ci, ci, asp, ctypes.POINTER(sz)]
        L.adn_aec_mr_online.argtypes = [vp, vp, ci, ci, ci, ci, cl, asp, vp, sz, ci, vp, vp, ci, ci, vp]
        L.adn_aec_mr_stream.argtypes = [vp, sz, vp, ci, ci, cl, ci, cl, ci, ci, ci, ci, ci, ci, asp, vp, sz, vp]
        for name in CALL_EXPORTED_SYMBOLS[1:]:
            getattr(L, name).restype = ci
        _call = L
        return L


def check_call(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_call().adn_call_last_error()
        raise AdnError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")


class SpectralParamsStruct(ctypes.Structure):
    """``adn_spectral_params`` of include/adn.h (the Python face is ``audiodenoiser_amd.baseline.SpectralParams``)."""
    _fields_ = [(name, ctypes.c_float) for name in ("smooth", "beta", "gamma", "alpha", "gain_floor", "bias")]


class WpeParamsStruct(ctypes.Structure):
    """``adn_wpe_params`` of include/adn.h (the Python face is ``audiodenoiser_amd.dereverb.WpeParams``)."""
    _fields_ = [("taps", ctypes.c_int), ("delay", ctypes.c_int), ("iterations", ctypes.c_int), ("loading", ctypes.c_float),
                ("power_floor", ctypes.c_float)]


class WpeStreamParamsStruct(ctypes.Structure):
    """``adn_wpe_stream_params`` of include/adn.h (the Python face is ``audiodenoiser_amd.dereverb.WpeStreamParams``)."""
    _fields_ = [("taps", ctypes.c_int), ("delay", ctypes.c_int), ("forget", ctypes.c_float), ("loading", ctypes.c_float),
                ("power_floor", ctypes.c_float), ("smooth", ctypes.c_float)]


class MvdrParamsStruct(ctypes.Structure):
    """``adn_mvdr_params`` of include/adn.h (the Python face is ``audiodenoiser_amd.beamform.MvdrParams``)."""
    _fields_ = [("ref_channel", ctypes.c_int), ("loading", ctypes.c_float), ("mask_floor", ctypes.c_float)]


class MvdrStreamParamsStruct(ctypes.Structure):
    """``adn_mvdr_stream_params`` of include/adn.h (the Python face is ``audiodenoiser_amd.beamform.MvdrStreamParams``)."""
    _fields_ = [("ref_channel", ctypes.c_int), ("refresh", ctypes.c_int), ("forget", ctypes.c_float), ("loading", ctypes.c_float),
                ("mask_floor", ctypes.c_float)]


class AecParamsStruct(ctypes.Structure):
    """``adn_aec_params`` of include/adn_echo.h (the Python face is ``audiodenoiser_amd.echo.AecParams``)."""
    _fields_ = [("taps", ctypes.c_int), ("delay", ctypes.c_int), ("forget", ctypes.c_float), ("loading", ctypes.c_float),
                ("quiet", ctypes.c_float)]


class SpectralRow(ctypes.Structure):
    """``adn_spectral_row`` of include/adn.h: one row of an ``adn_spectral_gain_windows`` call."""
    _fields_ = [("slot", ctypes.c_int), ("fresh", ctypes.c_int)]


class StreamPoolRateRow(ctypes.Structure):
    """``adn_stream_pool_rate_row`` of include/adn.h: one row of a push_rate / emit_rate call."""
    _fields_ = [("slot", ctypes.c_int), ("rate", ctypes.c_int), ("call_index", ctypes.c_long), ("received_before", ctypes.c_long),
                ("n_new", ctypes.c_long), ("final", ctypes.c_int), ("audio_offset", ctypes.c_long)]


class StreamPoolRow(ctypes.Structure):
    """``adn_stream_pool_row`` of include/adn.h: one row of a pool call."""
    _fields_ = [("slot", ctypes.c_int), ("step", ctypes.c_int), ("final_length", ctypes.c_int)]


def staging_device():
    """The ROCm device host tensors are staged on when a caller hands CPU tensors to the mirror (the reference's
    ``test.py`` keeps model and data on the CPU, ``test.py:63-66,100,112-113``): torch's current device.  There is
    no CPU implementation, so without a device this raises."""
    import torch
    if not torch.cuda.is_available():
        raise AdnError("audiodenoiser_amd: no ROCm device is visible; the hot path has no CPU implementation "
                       "(CPU tensors are staged onto the current ROCm device, computed there by libadn.so and copied back)")
    return torch.device("cuda", torch.cuda.current_device())


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().adn_last_error()
        raise AdnError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")


EXPORTED_SYMBOLS = (
    "adn_version", "adn_last_error", "adn_device_count", "adn_prepare", "adn_unet_create", "adn_unet_create_ex", "adn_unet_create_general",
    "adn_unet_channels", "adn_unet_set_batch_invariant", "adn_unet_destroy", "adn_unet_workspace_bytes", "adn_unet_forward", "adn_unet_forward_taps", "adn_unet_set_timing",
    "adn_unet_get_timing", "adn_stft_n_frames", "adn_stft_mag", "adn_stft_mag_fit",
    "adn_quantize_pad", "adn_per_clip_l1", "adn_perceptual_loss_workspace_bytes", "adn_perceptual_loss",
    "adn_perceptual_loss_backward_workspace_bytes", "adn_perceptual_loss_backward", "adn_istft_length", "adn_griffin_lim_workspace_bytes", "adn_griffin_lim", "adn_stft_complex",
    "adn_istft_workspace_bytes", "adn_istft",
    "adn_resample_length", "adn_resample_prepare", "adn_resample", "adn_mix_snr_workspace_bytes", "adn_mix_snr", "adn_reverb",
    "adn_denoise_plan", "adn_denoise_windows", "adn_denoise_stitch", "adn_denoise_resynth",
    "adn_stream_plan", "adn_stream_state_bytes", "adn_stream_reset", "adn_stream_analyze", "adn_stream_emit",
    "adn_stream_pool_state_bytes", "adn_stream_pool_reset", "adn_stream_pool_write", "adn_stream_pool_analyze", "adn_stream_pool_emit",
    "adn_resample_stream_plan", "adn_resample_stream_state_bytes", "adn_resample_stream",
    "adn_stream_pool_rate_state_bytes", "adn_stream_pool_push_rate", "adn_stream_pool_emit_rate",
    "adn_quality_workspace_bytes", "adn_quality", "adn_stoi_workspace_bytes", "adn_stoi",
    "adn_spectral_gain", "adn_spectral_gain_windows", "adn_wpe_workspace_bytes", "adn_wpe",
    "adn_wpe_mc_workspace_bytes", "adn_wpe_mc",
    "adn_wpe_stream_state_bytes", "adn_wpe_online", "adn_wpe_stream", "adn_wpe_stream_pool",
    "adn_wpe_mc_stream_state_bytes", "adn_wpe_mc_online", "adn_wpe_mc_stream", "adn_wpe_mc_stream_pool",
    "adn_mvdr_workspace_bytes", "adn_mvdr",
    "adn_mvdr_stream_state_bytes", "adn_mvdr_online", "adn_mvdr_stream", "adn_mvdr_stream_pool",
)

# libadn_echo.so (include/adn_echo.h): a library of its own, so that the table above stays libadn.so's whole symbol table
ECHO_EXPORTED_SYMBOLS = ("adn_aec_last_error", "adn_aec_stream_state_bytes", "adn_aec_online", "adn_aec_stream")

# libadn_call.so (include/adn_call.h): operators of a two-way call that the two closed tables above cannot take.  This table is
# open: the next call operator is added here, in the header and in csrc/libadn_call.map
CALL_EXPORTED_SYMBOLS = ("adn_call_last_error", "adn_aec_stream_pool", "adn_aec_mr_state_bytes", "adn_aec_mr_online", "adn_aec_mr_stream")
