"""Drop-in for the reference's ``data_loader.py`` (``/root/reference/code/data_loader.py:1-72``).

``SpectrogramDataset(data_dir, target_size=(256, 64))`` keeps the reference contract: it pairs the sorted
``clean*.npy`` / ``noisy*.npy`` files of one folder, and ``__getitem__`` returns ``(noisy, clean)`` as
``(1, H, W)`` float32 tensors whose values went through float16 and were cropped / zero padded (bottom, right)
to ``target_size``.  That per-item host path is file I/O plus two numpy calls and stays on the host, as in the
reference (DataLoader worker processes cannot share a GPU context).

``load_batch_to_device`` is the MI355X ingest for the step right before the forward: raw fp32 spectrograms
are uploaded once and quantised + cropped/padded by one HIP kernel (``adn_quantize_pad``), producing the
``(B, 1, H, W)`` batch directly in HBM.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib
from .wav import read_wav, wav_info


def _list(data_dir: str, prefix: str, suffix: str = ".npy"):
    return sorted(os.path.join(data_dir, f) for f in os.listdir(data_dir)
                  if f.startswith(prefix) and f.endswith(suffix))


def fit_to(data: np.ndarray, target_size) -> np.ndarray:
    """Crop or zero-pad (bottom / right) a 2-D array to ``target_size`` (reference ``_pad_or_truncate``)."""
    th, tw = target_size
    out = np.zeros((th, tw), dtype=data.dtype)
    h, w = min(th, data.shape[0]), min(tw, data.shape[1])
    out[:h, :w] = data[:h, :w]
    return out


class SpectrogramDataset(Dataset):
    def __init__(self, data_dir, target_size=(256, 64)):
        self.target_size = tuple(target_size)
        clean = _list(data_dir, "clean")
        noisy = _list(data_dir, "noisy")
        print(f"Found {len(clean)} clean files and {len(noisy)} noisy files in {data_dir}")
        assert len(clean) == len(noisy), f"Mismatch in {data_dir}"
        self.pairs = list(zip(noisy, clean))
        print(f"Total pairs loaded: {len(self.pairs)}")

    def __len__(self):
        return len(self.pairs)

    def _load(self, path):
        with np.errstate(over="ignore"):
            spec = np.load(path).astype(np.float16)       # honours the header's fortran_order flag
        return torch.from_numpy(fit_to(spec, self.target_size).astype(np.float32)).unsqueeze(0)

    def __getitem__(self, idx):
        noisy_path, clean_path = self.pairs[idx]
        return self._load(noisy_path), self._load(clean_path)

    # ---- MI355X ingest -------------------------------------------------------------------------------
    def load_batch_to_device(self, indices, device="cuda"):
        """(noisy, clean) batches ``(B, 1, H, W)`` float32 on ``device`` for same-shaped source files."""
        noisy = np.stack([np.ascontiguousarray(np.load(self.pairs[i][0]), dtype=np.float32) for i in indices])
        clean = np.stack([np.ascontiguousarray(np.load(self.pairs[i][1]), dtype=np.float32) for i in indices])
        return (quantize_pad_on_device(torch.from_numpy(noisy).to(device), self.target_size),
                quantize_pad_on_device(torch.from_numpy(clean).to(device), self.target_size))


def quantize_pad_on_device(spec: torch.Tensor, target_size) -> torch.Tensor:
    """``spec`` (B, h, w) float32 on a ROCm device -> (B, 1, H, W) = fp32(fp16(spec)) cropped / zero padded."""
    if not spec.is_cuda or spec.dtype != torch.float32 or spec.dim() != 3:
        raise ValueError("quantize_pad_on_device: expected a (B, h, w) float32 tensor on a ROCm device")
    spec = spec.contiguous()
    b, h, w = spec.shape
    H, W = target_size
    out = torch.empty((b, 1, H, W), dtype=torch.float32, device=spec.device)
    stream = torch.cuda.current_stream(spec.device).cuda_stream
    with torch.cuda.device(spec.device):
        _lib.check(_lib.load().adn_quantize_pad(spec.data_ptr(), b, h, w, out.data_ptr(), H, W, stream),
                   "adn_quantize_pad")
    return out


class WavToSpecDataset(Dataset):
    """On-the-fly wav -> magnitude-spectrogram pairs: the dataset ``train.py`` imports
    (``/root/reference/code/train.py:16,106-109``: ``WavToSpecDataset(data_dir=..., subset_fraction=...)``) but whose
    module (``new_unet_data_loader``) is not part of the reference tree.  The contract is therefore assembled from
    the reference pieces on either side of it:

    * pairing as in ``SpectrogramDataset`` (``data_loader.py:17-31``): sorted ``clean*`` / ``noisy*`` files of one
      folder, equal counts asserted, here with the ``.wav`` suffix;
    * audio -> spectrogram as in ``audio_to_spectrogram`` (``create_test_dataset.py:35-41``): centred STFT,
      n_fft 512 / hop 128 by default, magnitude;
    * item format as in ``SpectrogramDataset.__getitem__`` (``data_loader.py:37-52``): fp32(fp16(.)), crop or
      bottom/right zero-pad to ``target_size``, ``(noisy, clean)`` each ``(1, H, W)`` float32.

    ``subset_fraction`` keeps the first ``max(1, int(n * fraction))`` pairs of the sorted list (deterministic).
    The STFT, the quantisation and the crop/pad run on the device (``adn_stft_mag`` + ``adn_quantize_pad``); there is
    no host STFT.  That fixes how the dataset is fed to a ``DataLoader`` (reference ``train.py:118-119`` uses
    ``num_workers=4, pin_memory=True``):

    * ``ds[i]`` (main process, ``num_workers=0``): device STFT, items come back as host tensors like the reference's
      datasets.  Inside a DataLoader worker that was FORKED from a parent that has already initialised HIP
      (``model.to(DEVICE)``, ``train.py:122``, then the default fork start method) it raises: such a child cannot use
      the GPU.  Workers started with ``multiprocessing_context="spawn"`` (or forked before anything touched the GPU)
      own a HIP context of their own and work -- at the price of one context per worker.
    * ``ds.loader(clip_samples, batch_size=16, num_workers=4, pin_memory=True, shuffle=True)``: a ``DataLoader`` over
      :meth:`audio_view` whose workers only decode wav files (host I/O) and collate fixed-length audio; the MAIN
      process then runs ONE batched device STFT per batch and yields ``(noisy, clean)`` batches ``(B, 1, H, W)``
      already resident in HBM -- the MI355X-shaped feed (a ``collate_fn`` cannot do this: it runs in the worker).
      ``subset=`` takes the ``Subset`` objects of ``random_split(ds, ...)`` (``train.py:111-114``) or a list of indices.
    * ``load_batch_to_device(indices)``: the same without a DataLoader.

    ``ds[i]`` transforms the WHOLE file and crops / zero-pads the spectrogram; the loader crops / zero-pads the AUDIO to
    ``clip_samples`` first.  Both give the same item when ``clip_samples >= min_clip_samples()`` =
    ``(W - 1) * hop + n_fft // 2``: then every frame inside ``target_size`` sees the same samples, and for a file SHORTER
    than ``clip_samples`` the frames that do not exist in its own STFT (index > L // hop; they would overlap the file's tail
    in the padded audio) are zeroed on the device from the true length the view hands along -- the loader rule's right
    zero-padding.  Below that bound a file longer than ``clip_samples`` loses samples the last frames would have seen;
    :meth:`audio_view` / :meth:`loader` refuse it unless ``allow_cut_frames=True``.

    ``sample_rate`` (if given) is checked against each file; by default a file at another rate raises.  With
    ``resample=True`` (needs a ``sample_rate``) such files are converted to ``sample_rate`` on the device before the STFT
    (``adn_resample``, :mod:`audiodenoiser_amd.resample`: this project's Kaiser polyphase filter, not librosa's soxr) -- in
    ``ds[i]`` and ``load_batch_to_device`` (clips of one call that share rate and length go through one launch).  The
    worker-fed form (:meth:`audio_view`, :meth:`to_device_batch`, :meth:`loader`) hands out audio without its rate and
    refuses ``resample=True``.
    """

    def __init__(self, data_dir, subset_fraction: float = 1.0, target_size=(256, 64), n_fft: int = 512,
                 hop_length: int = 128, sample_rate=None, device="cuda", resample: bool = False):
        if not 0.0 < subset_fraction <= 1.0:
            raise ValueError("subset_fraction must be in (0, 1]")
        if resample and sample_rate is None:
            raise ValueError("resample=True needs the sample_rate to convert to")
        self.resample = bool(resample)
        self.target_size = tuple(target_size)
        self.n_fft, self.hop_length, self.sample_rate, self.device = n_fft, hop_length, sample_rate, device
        clean = _list(data_dir, "clean", ".wav")
        noisy = _list(data_dir, "noisy", ".wav")
        print(f"Found {len(clean)} clean files and {len(noisy)} noisy files in {data_dir}")
        assert len(clean) == len(noisy), f"Mismatch in {data_dir}"
        pairs = list(zip(noisy, clean))
        keep = max(1, int(len(pairs) * subset_fraction)) if pairs else 0
        self.pairs = pairs[:keep]
        print(f"Total pairs loaded: {len(self.pairs)}")

    def __len__(self):
        return len(self.pairs)

    def _audio(self, path):
        audio, rate = read_wav(path, mono=True)
        if self.sample_rate is not None and rate != self.sample_rate:
            raise ValueError(f"{path}: sample rate {rate} != expected {self.sample_rate} (no resampler in this build)")
        return audio

    def _device_audio(self, paths):
        """``resample=True``: the files of ``paths`` as 1-D float32 device tensors at ``sample_rate``; files that share
        rate and length are resampled in one launch."""
        return _load_at_rate(paths, self.sample_rate, self.device)

    def _refuse_resample(self, what):
        if self.resample:
            raise ValueError(f"WavToSpecDataset.{what}: the worker-fed form hands out audio without its sample rate and does not "
                             "support resample=True; use ds[i] or load_batch_to_device(indices), which resample on the device")

    def _spec_batch(self, audios):
        """(B, L) float32 audio (array, list of equally long arrays or tensors, or tensor) -> (B, 1, H, W) float32 on the device."""
        from .stft import stft_magnitude_fit
        if isinstance(audios, torch.Tensor):
            a = audios
        elif isinstance(audios[0], torch.Tensor):
            a = torch.stack(list(audios))
        else:
            a = torch.from_numpy(np.stack(audios))
        a = a.to(self.device, non_blocking=True)
        # STFT + fp16 round trip + crop/pad in ONE kernel: only the frames inside target_size are computed
        return stft_magnitude_fit(a, self.target_size, self.n_fft, self.hop_length, True)

    def __getitem__(self, idx):
        if torch.utils.data.get_worker_info() is not None and _forked_from_gpu_parent():
            raise RuntimeError(
                "WavToSpecDataset computes its spectrograms on the GPU (there is no host STFT) and a DataLoader worker "
                "process forked from a GPU-initialised parent cannot use HIP.  Use num_workers=0, "
                "multiprocessing_context='spawn', or let the workers decode audio only and transform in the main "
                "process: ds.loader(clip_samples, batch_size=..., num_workers=4)")
        noisy_path, clean_path = self.pairs[idx]
        if self.resample:
            noisy, clean = self._device_audio([noisy_path, clean_path])
        else:
            noisy, clean = self._audio(noisy_path), self._audio(clean_path)
        if len(noisy) == len(clean):
            both = self._spec_batch([noisy, clean]).cpu()
            return both[0], both[1]
        return self._spec_batch([noisy]).cpu()[0], self._spec_batch([clean]).cpu()[0]

    def load_batch_to_device(self, indices):
        """(noisy, clean) batches ``(B, 1, H, W)`` on the device; clips of one call must have one length (with
        ``resample=True``: after the conversion)."""
        if self.resample:
            both = self._device_audio([self.pairs[i][0] for i in indices] + [self.pairs[i][1] for i in indices])
            return self._spec_batch(both[:len(indices)]), self._spec_batch(both[len(indices):])
        noisy = [self._audio(self.pairs[i][0]) for i in indices]
        clean = [self._audio(self.pairs[i][1]) for i in indices]
        return self._spec_batch(noisy), self._spec_batch(clean)

    # ---- DataLoader feed: host-only items in the workers, device transform in the main process ---------------
    def min_clip_samples(self) -> int:
        """Samples the frames inside ``target_size`` reach: the last one (index W - 1, centred STFT) ends at
        ``(W - 1) * hop + n_fft // 2``.  An audio crop at least this long leaves every item equal to ``ds[i]``."""
        return (self.target_size[1] - 1) * self.hop_length + self.n_fft // 2

    def audio_view(self, clip_samples: int, allow_cut_frames: bool = False):
        """Host-only ``Dataset`` of ``(noisy_audio, clean_audio)`` float32 tensors cropped / zero-padded at the end to
        ``clip_samples`` -- safe in DataLoader worker processes (wav decoding only, no GPU).  ``clip_samples`` below
        :meth:`min_clip_samples` would cut samples off frames inside ``target_size`` for longer files (items would
        differ from ``ds[i]``): refused unless ``allow_cut_frames=True``.  Not available with ``resample=True``."""
        self._refuse_resample("audio_view")
        clip_samples = int(clip_samples)
        if clip_samples < self.min_clip_samples() and not allow_cut_frames:
            raise ValueError(
                f"clip_samples={clip_samples} is shorter than the {self.min_clip_samples()} samples the {self.target_size[1]} frames "
                f"of target_size reach (n_fft {self.n_fft}, hop {self.hop_length}): files longer than clip_samples would give "
                "other items than ds[i].  Pass a longer clip or allow_cut_frames=True")
        return _WavAudioView(self, clip_samples)

    def to_device_batch(self, host_batch):
        """``(noisy_audio (B, L), clean_audio (B, L), noisy_len (B,), clean_len (B,))`` host tensors (what a DataLoader
        over :meth:`audio_view` yields; the lengths are the files' true sample counts) -> ``(noisy, clean)`` each
        ``(B, 1, H, W)`` float32 on the device: one batched STFT + quantise + crop/pad per side, then the frames a short
        file's own STFT does not have (index > len // hop) are zeroed.  Must run in the process that owns the GPU context
        (the DataLoader's consumer, not its workers).  Not available with ``resample=True``."""
        self._refuse_resample("to_device_batch")
        noisy, clean = host_batch[0], host_batch[1]
        out = [self._spec_batch(noisy), self._spec_batch(clean)]
        if len(host_batch) >= 4:
            frames = torch.arange(self.target_size[1], device=out[0].device)
            for k in range(2):
                nfr = 1 + torch.as_tensor(host_batch[2 + k]).to(out[k].device).clamp(max=noisy.shape[1]) // self.hop_length
                keep = frames[None, :] < nfr[:, None]                       # (B, W)
                out[k] = torch.where(keep[:, None, None, :], out[k], torch.zeros((), device=out[k].device))
        return out[0], out[1]

    def loader(self, clip_samples: int, subset=None, allow_cut_frames: bool = False, **dataloader_kwargs):
        """Iterable with the ``DataLoader`` call shape of ``train.py:118-119`` (``batch_size``, ``shuffle``,
        ``num_workers``, ``pin_memory``, ...) that yields device-resident spectrogram batches.  ``subset``: a
        ``torch.utils.data.Subset`` of this dataset (what ``random_split`` returns, ``train.py:111-114``) or a sequence of
        indices -- the feed then covers those items only.  Not available with ``resample=True``."""
        self._refuse_resample("loader")
        from torch.utils.data import DataLoader, Subset
        if "collate_fn" in dataloader_kwargs:
            raise ValueError("loader(): the collate function is fixed (stacked fixed-length audio)")
        view = self.audio_view(clip_samples, allow_cut_frames)
        if subset is not None:
            if isinstance(subset, Subset):
                if subset.dataset is not self:
                    raise ValueError("loader(subset=...): the Subset must be a split of this dataset")
                subset = subset.indices
            view = Subset(view, [int(i) for i in subset])
        return _DeviceSpecLoader(self, DataLoader(view, **dataloader_kwargs))


def _load_at_rate(paths, sample_rate, device):
    """Decode ``paths`` (mono) and return them as 1-D float32 tensors on ``device`` at ``sample_rate``: files at another rate
    go through the device resampler, one launch per (rate, length) group."""
    from .resample import resample
    decoded = [read_wav(p, mono=True) for p in paths]
    out, groups = [None] * len(paths), {}
    for k, (audio, rate) in enumerate(decoded):
        if rate == sample_rate or len(audio) == 0:
            out[k] = torch.from_numpy(audio).to(device)
        else:
            groups.setdefault((rate, len(audio)), []).append(k)
    for (rate, _), members in groups.items():
        y = resample(torch.from_numpy(np.stack([decoded[k][0] for k in members])).to(device), rate, sample_rate)
        for j, k in enumerate(members):
            out[k] = y[j]
    return out


def _forked_from_gpu_parent() -> bool:
    """True in a process forked from a parent that had already initialised the GPU through torch: HIP cannot be used
    there.  False in spawned workers and in workers forked before anything touched the GPU (both can open a context)."""
    probe = getattr(torch.cuda, "_is_in_bad_fork", None)
    return bool(probe()) if probe is not None else True


class _DeviceSpecLoader:
    def __init__(self, parent: "WavToSpecDataset", host_loader):
        self.parent, self.host_loader = parent, host_loader

    def __len__(self):
        return len(self.host_loader)

    def __iter__(self):
        for host_batch in self.host_loader:
            yield self.parent.to_device_batch(host_batch)


class _WavAudioView(Dataset):
    def __init__(self, parent: "WavToSpecDataset", clip_samples: int):
        if clip_samples < parent.n_fft // 2 + 1:
            raise ValueError("clip_samples too short for one centred STFT frame")
        self.parent, self.clip_samples = parent, clip_samples

    def __len__(self):
        return len(self.parent)

    def _fit(self, audio):
        out = np.zeros(self.clip_samples, dtype=np.float32)
        n = min(self.clip_samples, len(audio))
        out[:n] = audio[:n]
        return torch.from_numpy(out)

    def __getitem__(self, idx):
        noisy_path, clean_path = self.parent.pairs[idx]
        noisy, clean = self.parent._audio(noisy_path), self.parent._audio(clean_path)
        return self._fit(noisy), self._fit(clean), len(noisy), len(clean)


def _resampled_length(length: int, rate: int, sample_rate: int) -> int:
    """``ceil(length * up / down)``, the rule of ``adn_resample_length``, on the host (dataset sizes need no device)."""
    g = math.gcd(rate, sample_rate)
    up, down = sample_rate // g, rate // g
    return (length * up + down - 1) // down


class NoiseMixDataset(Dataset):
    """The reference's train-set builder (``/root/reference/code/create_train_dataset.py:181-254``) as an on-the-fly
    dataset: a folder of clean wavs and a folder of noise wavs in, device-resident ``(noisy, clean)`` spectrogram batches out.

    * Files: every ``.wav`` of each folder, sorted (``load_wav_list``, ``:43-49``).  A file is decoded once (mono), converted to
      ``sample_rate`` on the device (``adn_resample``) and kept there as float32; the noise file is not decoded again per chunk.
    * Items: each clean file is cut into non-overlapping chunks of ``int(sample_rate * chunk_seconds)`` samples, a shorter
      tail is dropped (``frame_audio``, ``:71-84``); item ``i`` is chunk ``i // len(noise_types)`` with noise type
      ``noise_types[i % len(noise_types)]``.  ``len(ds)`` comes from the wav headers alone.
    * Randomness: every random decision of item ``i`` is drawn from ``numpy.random.default_rng([seed, epoch, i])`` in a fixed
      order -- the noise file, the snippet position of ``match_audio_length`` (``:52-68``), the 0.8 coins of
      ``"noise_cancellation"`` (one per 16000-sample block, ``:124-135``) and the seed of the white noise, which is
      ``torch.randn`` of a ``torch.Generator`` on the device.  :meth:`item_plan` returns them; :meth:`set_epoch` changes the draw.
    * Noise types: ``"white"`` and ``"urban"`` are mixed at ``snr_db`` by ``adn_mix_snr``; ``"noise_cancellation"`` is
      elementwise on the device.  ``"reverb"`` is refused with ``ValueError`` by default: the reference renders it with the
      third-party Pedalboard ``Reverb`` effect, which is not reproduced.  ``reverb=True`` (default settings) or
      ``reverb=ReverbSettings(...)`` opts in to this project's own Freeverb (:mod:`audiodenoiser_amd.reverb`, ``adn_reverb``;
      defined in ``include/adn.h``, parity with Pedalboard unpinned): the item is ``reverb(clean_chunk, sample_rate, clip=True)``
      with zero state at the chunk's first sample (``pedalboard_reverb`` + ``np.clip``, ``:87-102,116-121``), one launch per
      batch.  It uses none of the item's random draws, and opting in changes no draw of any item.
    * ``ds[i]`` -> ``(noisy, clean)`` each ``(1, H, W)`` float32 host tensors (the reference's item format);
      ``ds.audio_batch(indices)`` -> ``(noisy_audio, clean_audio)`` each ``(B, chunk)`` on the device;
      ``ds.load_batch_to_device(indices)`` -> ``(noisy, clean)`` each ``(B, 1, H, W)`` on the device, the
      ``stft_magnitude_fit`` of exactly those audio batches (``center=False`` as in ``audio_to_magnitude_spectrogram``,
      ``:162-174``).  Per batch: one resample launch per (rate, length) group of files not yet cached, one mix launch per
      noise type, two STFT launches.

    ``NOISE_TYPES`` lists the types that need no opt-in.
    """

    NOISE_TYPES = ("white", "urban", "noise_cancellation")
    _NC_BLOCK, _NC_HALF = 16000, 8000          # the reference's block constants are samples, whatever the rate (:128-130)

    def __init__(self, clean_dir, noise_dir, noise_types=("white", "urban"), sample_rate: int = 8000, chunk_seconds: float = 2.0,
                 snr_db: float = 8.0, target_size=(256, 64), n_fft: int = 512, hop_length: int = 128, center: bool = False,
                 seed: int = 0, device="cuda", reverb=None):
        noise_types = tuple(noise_types)
        if reverb is None or reverb is False:
            self.reverb = None
        else:
            from .reverb import MAX_SAMPLE_RATE, MIN_SAMPLE_RATE, ReverbSettings
            if reverb is not True and not isinstance(reverb, ReverbSettings):
                raise TypeError("reverb must be None, True (default settings) or a ReverbSettings")
            if not MIN_SAMPLE_RATE <= int(sample_rate) <= MAX_SAMPLE_RATE:
                raise ValueError(f"reverb needs a sample_rate in [{MIN_SAMPLE_RATE}, {MAX_SAMPLE_RATE}], got {sample_rate}")
            self.reverb = ReverbSettings() if reverb is True else reverb
        if "reverb" in noise_types and self.reverb is None:
            raise ValueError('noise type "reverb" is not available: the reference renders it with the third-party Pedalboard '
                             "Reverb effect (create_train_dataset.py:87-102), which this project does not reimplement; pass "
                             "reverb=True or reverb=ReverbSettings(...) to opt in to this project's own Freeverb "
                             "(audiodenoiser_amd.reverb), whose parity with Pedalboard is unpinned")
        legal = self.NOISE_TYPES + (("reverb",) if self.reverb is not None else ())
        bad = [t for t in noise_types if t not in legal]
        if bad or not noise_types:
            raise ValueError(f"noise_types must be a non-empty selection of {legal}, got {noise_types}")
        self.noise_types, self.sample_rate, self.snr_db = noise_types, int(sample_rate), float(snr_db)
        self.chunk_samples = int(self.sample_rate * chunk_seconds)
        if self.chunk_samples < 1:
            raise ValueError("chunk_seconds * sample_rate must be at least one sample")
        self.target_size = tuple(target_size)
        self.n_fft, self.hop_length, self.center = int(n_fft), int(hop_length), bool(center)
        self.seed, self.epoch, self.device = int(seed), 0, device
        self.clean_files = self._wavs(clean_dir)
        self.noise_files = self._wavs(noise_dir)
        # lengths at sample_rate from the headers: nothing is decoded here
        self.clean_lengths = [self._length_of(p) for p in self.clean_files]
        self.noise_lengths = [self._length_of(p) for p in self.noise_files]
        self.chunks = [(f, c) for f, n in enumerate(self.clean_lengths) for c in range(n // self.chunk_samples)]
        self._cache = {}

    @staticmethod
    def _wavs(dirname):
        return sorted(os.path.join(dirname, f) for f in os.listdir(dirname) if f.lower().endswith(".wav"))

    def _length_of(self, path):
        rate, _, frames = wav_info(path)
        return _resampled_length(frames, rate, self.sample_rate) if frames else 0

    def __len__(self):
        return len(self.chunks) * len(self.noise_types)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def item_plan(self, idx: int) -> dict:
        """Everything that decides item ``idx``: clean file and chunk, noise type and the item's random draws (host only)."""
        idx = int(idx)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        chunk, kind = divmod(idx, len(self.noise_types))
        f, c = self.chunks[chunk]
        rng = np.random.default_rng([self.seed, self.epoch, idx])
        noise_file = int(rng.integers(len(self.noise_files))) if self.noise_files else None
        u = float(rng.random())
        blocks = -(-self.chunk_samples // self._NC_BLOCK)
        coins = [bool(v < 0.8) for v in rng.random(blocks)]
        white_seed = int(rng.integers(1 << 62))
        start = None
        if noise_file is not None and self.noise_lengths[noise_file] > self.chunk_samples:
            start = int(u * (self.noise_lengths[noise_file] - self.chunk_samples))       # randint(0, len - target): high excluded
        return {"index": idx, "clean_file": f, "chunk": c, "noise_type": self.noise_types[kind], "noise_file": noise_file,
                "noise_start": start, "coins": coins, "white_seed": white_seed}

    def white_noise(self, idx: int) -> torch.Tensor:
        """The ``(chunk,)`` standard-normal samples item ``idx`` mixes in when its type is ``"white"`` (on the device)."""
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self.item_plan(idx)["white_seed"])
        return torch.randn(self.chunk_samples, generator=gen, device=self.device, dtype=torch.float32)

    def _audio_of(self, paths):
        """Cached device audio at ``sample_rate`` of ``paths``; the missing ones are decoded and resampled together."""
        missing = [p for p in dict.fromkeys(paths) if p not in self._cache]
        if missing:
            for p, a in zip(missing, _load_at_rate(missing, self.sample_rate, self.device)):
                self._cache[p] = a
        return [self._cache[p] for p in paths]

    def _match_length(self, noise: torch.Tensor, start) -> torch.Tensor:
        n = self.chunk_samples
        if len(noise) == n:
            return noise
        if len(noise) < n:
            return noise.repeat(-(-n // len(noise)))[:n] if len(noise) else torch.zeros(n, device=noise.device)
        return noise[start:start + n]

    def audio_batch(self, indices):
        """``(noisy_audio, clean_audio)`` each ``(B, chunk)`` float32 on the device for the items ``indices``."""
        from .resample import mix_snr
        from .reverb import reverb
        plans = [self.item_plan(i) for i in indices]
        if not plans:
            raise ValueError("audio_batch: no indices")
        n = self.chunk_samples
        files = self._audio_of([self.clean_files[p["clean_file"]] for p in plans])
        clean = torch.stack([a[p["chunk"] * n:(p["chunk"] + 1) * n] for a, p in zip(files, plans)])
        noisy = torch.empty_like(clean)
        for kind in self.noise_types:
            rows = [k for k, p in enumerate(plans) if p["noise_type"] == kind]
            if not rows:
                continue
            sel = torch.as_tensor(rows, device=clean.device)
            if kind == "reverb":
                r = self.reverb
                noisy[sel] = reverb(clean[sel], self.sample_rate, r.room_size, r.damping, r.wet_level, r.dry_level, r.width, clip=True)
                continue
            if kind == "noise_cancellation":
                out = clean[sel]
                for j, k in enumerate(rows):
                    for b, coin in enumerate(plans[k]["coins"]):
                        if coin:
                            lo, hi = b * self._NC_BLOCK, min(b * self._NC_BLOCK + self._NC_HALF, n)
                            out[j, lo:hi] = out[j, lo:hi] + (-0.8) * out[j, lo:hi]
                noisy[sel] = out.clamp_(-1.0, 1.0)
                continue
            if kind == "white":
                noise = torch.stack([self.white_noise(plans[k]["index"]) for k in rows])
            else:
                used = [plans[k]["noise_file"] for k in rows]
                if self.noise_files:
                    audio = self._audio_of([self.noise_files[f] for f in used])
                    noise = torch.stack([self._match_length(a, plans[k]["noise_start"]) for a, k in zip(audio, rows)])
                else:
                    noise = torch.zeros((len(rows), n), dtype=torch.float32, device=clean.device)
            noisy[sel] = mix_snr(clean[sel], noise, self.snr_db)
        return noisy, clean

    def load_batch_to_device(self, indices):
        """``(noisy, clean)`` each ``(B, 1, H, W)`` float32 on the device: ``stft_magnitude_fit`` of :meth:`audio_batch`."""
        from .stft import stft_magnitude_fit
        noisy, clean = self.audio_batch(indices)
        return (stft_magnitude_fit(noisy, self.target_size, self.n_fft, self.hop_length, self.center),
                stft_magnitude_fit(clean, self.target_size, self.n_fft, self.hop_length, self.center))

    def __getitem__(self, idx):
        noisy, clean = self.load_batch_to_device([idx])
        return noisy[0].cpu(), clean[0].cpu()
