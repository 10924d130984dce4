"""MI355X-native (gfx950) implementation of the AudioDenoiser hot path: STFT magnitude + U-Net forward.

Importing the package does not touch the GPU; the HIP library is loaded (and built if missing) on first use
and every entry point raises if it is unavailable — there is no CPU or eager-PyTorch fallback.
"""
__version__ = "0.1.0"

__all__ = ["UNet", "SpectrogramDataset", "WavToSpecDataset", "audio_to_magnitude_spectrogram",
           "audio_to_spectrogram", "stft_magnitude", "per_clip_l1", "CombinedPerceptualLoss", "NoiseMixDataset",
           "resample_length", "mix_snr", "load_audio", "StreamResampler", "Denoiser", "StreamDenoiser", "StreamPool", "ReverbSettings",
           "snr", "si_sdr", "seg_snr", "stoi", "evaluate", "SpectralDenoiser", "SpectralParams",
           "StreamSpectralDenoiser", "SpectralStreamPool", "spectral_gain_windows", "Dereverberator", "WpeParams",
           "WpeStreamParams", "wpe_online", "StreamDereverberator", "DereverbStreamPool", "Beamformer", "MvdrParams", "mvdr",
           "MvdrStreamParams", "mvdr_online", "mvdr_stream_state_bytes", "StreamBeamformer",
           "BeamformStreamPool", "EchoCanceller", "AecParams", "aec_online", "aec_stream_state_bytes", "StreamEchoCanceller",
           "EchoStreamPool", "aec_pool_state_bytes", "aec_mr_online", "aec_mr_state_bytes"]
# (resample / reverb themselves: audiodenoiser_amd.resample.resample, audiodenoiser_amd.reverb.reverb -- the modules own the names)


def __getattr__(name):
    if name == "UNet":
        from .model import UNet
        return UNet
    if name in ("SpectrogramDataset", "WavToSpecDataset", "NoiseMixDataset"):
        from . import data_loader
        return getattr(data_loader, name)
    if name in ("audio_to_magnitude_spectrogram", "audio_to_spectrogram", "stft_magnitude"):
        from . import stft
        return getattr(stft, name)
    if name in ("resample_length", "mix_snr", "load_audio", "StreamResampler"):
        import importlib
        return getattr(importlib.import_module(".resample", __name__), name)
    if name == "ReverbSettings":
        import importlib
        return importlib.import_module(".reverb", __name__).ReverbSettings
    if name == "Denoiser":
        import importlib
        return importlib.import_module(".denoise", __name__).Denoiser
    if name in ("SpectralDenoiser", "SpectralParams", "StreamSpectralDenoiser", "SpectralStreamPool", "spectral_gain_windows"):
        import importlib
        return getattr(importlib.import_module(".baseline", __name__), name)
    if name in ("Dereverberator", "WpeParams", "WpeStreamParams", "wpe_online", "StreamDereverberator", "DereverbStreamPool"):
        import importlib
        return getattr(importlib.import_module(".dereverb", __name__), name)
    if name in ("Beamformer", "MvdrParams", "mvdr", "MvdrStreamParams", "mvdr_online", "mvdr_stream_state_bytes", "StreamBeamformer",
                "BeamformStreamPool"):
        import importlib
        return getattr(importlib.import_module(".beamform", __name__), name)
    if name in ("EchoCanceller", "AecParams", "aec_online", "aec_stream_state_bytes", "StreamEchoCanceller", "EchoStreamPool",
                "aec_pool_state_bytes", "aec_mr_online", "aec_mr_state_bytes"):
        import importlib
        return getattr(importlib.import_module(".echo", __name__), name)
    if name in ("StreamDenoiser", "StreamPool"):
        import importlib
        return getattr(importlib.import_module(".stream", __name__), name)
    if name in ("snr", "si_sdr", "seg_snr", "stoi", "evaluate"):
        import importlib
        return getattr(importlib.import_module(".metrics", __name__), name)
    if name in ("per_clip_l1", "CombinedPerceptualLoss"):
        from . import loss
        return getattr(loss, name)
    raise AttributeError(name)
