"""Streaming denoiser: audio that is still arriving, in blocks, with the state carried on the device.

    from audiodenoiser_amd import StreamDenoiser
    sd = StreamDenoiser(model, n_streams=1)           # an audiodenoiser_amd.model.UNet(1, 1) on a ROCm device, .eval()
    for block in feed:                                # (m,) or (n_streams, m) float32 at sample_rate, any m >= 0
        out = sd.push(block)                          # (n_streams, newly final samples), possibly zero columns
    out = sd.flush()                                  # the rest: exactly as many samples out as went in
    sd = StreamDenoiser(model, input_rate=48000)      # the same for a feed at 48 kHz: samples at 48 kHz in, samples at 48 kHz out

    python -m audiodenoiser_amd.stream --model CKPT.pth IN.wav OUT.wav [--chunk 1024] [--window 192] [--block 16]
                                       [--lookahead 0] [--dtype f32|f16] [--live]

``Denoiser`` handles a finished recording.  This class handles a call, a capture device, a long file read block by block, or many
concurrent feeds served from one card (definition: ``include/adn.h``, "stream"; float64 restatement: ``tests/stream_ref.py``;
kernels: ``csrc/stream_kernels.hip``).  Step ``k`` runs as soon as frame ``k B + B + A - 1`` of the centred STFT is complete,
feeds the network the last ``W = window_frames`` frames of ``|X|`` -- past context instead of an overlap with a neighbour -- and
keeps the ``B = block_frames`` frames that end ``A = lookahead_frames`` frames before the newest one.  Those are clamped at zero,
given the noisy input's phase and overlap-added onto the tail carried from the step before; what no later frame can change is
returned.  The result does not depend on how the audio was cut into ``push`` calls (bit for bit with
``model.set_batch_invariant(True)``, within the network's per-batch-size bound otherwise), and at worst ``latency_samples`` =
``(B + A - 1) hop + n_fft`` samples lie between a sample's arrival and its return.

All streams of one object advance in lockstep (one ``push`` brings the same number of samples for each); feeds with independent
timing use separate objects.  A ``push`` that completes several steps sends them through the network as one batch,
``batch_windows`` windows at a time.

``sample_rate`` is the network's working rate.  A feed at another rate names it as ``input_rate``: ``push`` then takes and returns
samples at ``input_rate``, and inside a ``StreamResampler`` (``adn_resample_stream``, the filter's history carried on the device)
brings them to the working rate, the steps above run, and a second one takes the result back -- all on the current stream.  The
result is, bit for bit with ``set_batch_invariant(True)``, ``resample`` of the whole input -> this class at the working rate ->
``resample`` back, cut to the input's length, whatever the pushes were; ``latency_input_samples`` bounds the delay at the input
rate (14 976 samples, 0.312 s, at 48 kHz with the default plan).  The command line's ``--live`` feeds the file that way, ``--chunk``
samples at its own rate at a time; without it the file is converted as a whole before and after the stream, as before.

What is NOT claimed: parity of the STFT with librosa stays unpinned, as everywhere in this package; ``window_frames=192``,
``block_frames=16`` and ``lookahead_frames=0`` are design values whose audible quality has not been judged; the result differs
from ``Denoiser``'s by design (other windows).  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

__all__ = ["StreamDenoiser", "stream_plan", "stream_rate_plan"]


def stream_plan(received: int, n_fft: int = 512, hop_length: int = 128, window_frames: int = 192, block_frames: int = 16,
                lookahead_frames: int = 0):
    """``(steps_done, emitted, latency_samples)`` after ``received`` samples (``adn_stream_plan``, host only)."""
    s, e, lat = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.load().adn_stream_plan(int(n_fft), int(hop_length), int(window_frames), int(block_frames), int(lookahead_frames),
                                           int(received), ctypes.byref(s), ctypes.byref(e), ctypes.byref(lat)), "adn_stream_plan")
    return int(s.value), int(e.value), int(lat.value)


def _rate_latency(input_rate: int, sample_rate: int, latency_samples: int) -> int:
    """``ceil((2 half + latency_samples down) / up)`` with up / down of input -> working rate: both filters' reach plus the steps'."""
    g = math.gcd(input_rate, sample_rate)
    up, down = sample_rate // g, input_rate // g
    half = 0 if up == down else 32 * max(up, down)
    return -(-(2 * half + latency_samples * down) // up)


def stream_rate_plan(received: int, input_rate: int, n_fft: int = 512, hop_length: int = 128, window_frames: int = 192,
                     block_frames: int = 16, lookahead_frames: int = 0, sample_rate: int = 8000):
    """``(emitted, latency_input_samples)``, both at ``input_rate``, of a ``StreamDenoiser(..., input_rate=input_rate)`` that has
    received ``received`` samples: the three plans composed (resampler in, steps, resampler out; host only)."""
    from .resample import resample_stream_plan
    plan = (n_fft, hop_length, window_frames, block_frames, lookahead_frames)
    at_work = resample_stream_plan(received, input_rate, sample_rate)[0]
    _, at_work_out, lat = stream_plan(at_work, *plan)
    return resample_stream_plan(at_work_out, sample_rate, input_rate)[0], _rate_latency(int(input_rate), int(sample_rate), lat)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class StreamDenoiser:
    def __init__(self, model, n_streams: int = 1, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128,
                 window_frames: int = 192, block_frames: int = 16, lookahead_frames: int = 0, batch_windows: int = 64,
                 input_rate=None):
        if not (isinstance(n_streams, int) and n_streams >= 1):
            raise ValueError("StreamDenoiser: n_streams must be >= 1")
        if not (isinstance(n_fft, int) and 64 <= n_fft <= 4096 and n_fft & (n_fft - 1) == 0):
            raise ValueError("StreamDenoiser: n_fft must be a power of two in [64, 4096]")
        if not (isinstance(hop_length, int) and 1 <= hop_length <= n_fft // 4):
            raise ValueError("StreamDenoiser: need 1 <= hop_length <= n_fft / 4 (the inverse transform of the whole input length "
                             "divides by a window sum-of-squares that falls to 2e-8 at n_fft / 2)")
        if not (isinstance(window_frames, int) and window_frames >= 16):
            raise ValueError("StreamDenoiser: window_frames must be >= 16 (the network pools four times)")
        if not (isinstance(block_frames, int) and block_frames >= 1):
            raise ValueError("StreamDenoiser: block_frames must be >= 1")
        if not (isinstance(lookahead_frames, int) and lookahead_frames >= 0):
            raise ValueError("StreamDenoiser: lookahead_frames must be >= 0")
        if block_frames + lookahead_frames > window_frames:
            raise ValueError("StreamDenoiser: need block_frames + lookahead_frames <= window_frames")
        if not (isinstance(batch_windows, int) and batch_windows >= 1):
            raise ValueError("StreamDenoiser: batch_windows must be >= 1")
        if not (isinstance(sample_rate, int) and sample_rate >= 1):
            raise ValueError("StreamDenoiser: sample_rate must be >= 1")
        if input_rate is not None and not (isinstance(input_rate, int) and input_rate >= 1):
            raise ValueError("StreamDenoiser: input_rate must be None (the feed is at sample_rate) or an integer >= 1")
        from .model import UNet
        if not isinstance(model, UNet) or model.in_channels != 1 or model.num_classes != 1:
            raise ValueError("StreamDenoiser: model must be an audiodenoiser_amd.model.UNet(1, 1)")
        if model.training:
            raise RuntimeError("StreamDenoiser: the model is in train mode; call .eval() (the HIP forward is the eval forward)")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("StreamDenoiser: the model must live on a ROCm device (model.to('cuda')); there is no CPU path")
        self.model, self.device = model, dev
        self.n_streams, self.sample_rate, self.n_fft, self.hop_length = n_streams, sample_rate, n_fft, hop_length
        self.window_frames, self.block_frames, self.lookahead_frames = window_frames, block_frames, lookahead_frames
        self.batch_windows = batch_windows
        self.n_bins = n_fft // 2 + 1
        # one analysis / emit call covers up to max_steps steps: about one network batch of windows over all streams
        self.max_steps = max(1, batch_windows // n_streams)
        self._plan = (n_fft, hop_length, window_frames, block_frames, lookahead_frames)
        need = ctypes.c_size_t()
        _lib.check(_lib.load().adn_stream_state_bytes(n_streams, *self._plan, self.max_steps, ctypes.byref(need)),
                   "adn_stream_state_bytes")
        self._state = torch.empty(need.value, dtype=torch.uint8, device=dev)
        # samples that do not complete a step yet wait here; room for the first step plus max_steps blocks
        self._cap = self._end_of(0) + self.max_steps * block_frames * hop_length
        self._pend = torch.zeros((n_streams, self._cap), dtype=torch.float32, device=dev)
        self._numpy = True
        # a feed at another rate: one resampler into the working rate, one back (none otherwise)
        self.input_rate = sample_rate if input_rate is None else input_rate
        self._rs_in = self._rs_out = None
        if self.input_rate != sample_rate:
            from .resample import StreamResampler
            self._rs_in = StreamResampler(self.input_rate, sample_rate, n_streams, dev)
            self._rs_out = StreamResampler(sample_rate, self.input_rate, n_streams, dev)
        self.reset()

    # ------------------------------------------------------------------ the plan
    def _end_of(self, step: int) -> int:
        """Samples that must have arrived for ``step`` to run (``e(k)`` of adn.h; 0 for step -1)."""
        if step < 0:
            return 0
        b, a = self.block_frames, self.lookahead_frames
        return (step * b + b + a - 1) * self.hop_length + self.n_fft // 2

    @property
    def latency_samples(self) -> int:
        return stream_plan(0, *self._plan)[2]

    @property
    def latency_input_samples(self) -> int:
        """``latency_samples`` at ``input_rate``, the reach of the two resampling filters included."""
        return _rate_latency(self.input_rate, self.sample_rate, self.latency_samples)

    @property
    def received(self) -> int:
        """Samples pushed so far, at ``input_rate``."""
        return self._received if self._rs_in is None else self._rs_in.received

    @property
    def emitted(self) -> int:
        """Samples returned so far, at ``input_rate``."""
        return self._emitted if self._rs_out is None else self._rs_out.emitted

    def reset(self):
        """Forget the running stream: the object is ready for a new one."""
        if self._rs_in is not None:
            self._rs_in.reset()
            self._rs_out.reset()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_stream_reset(self._state.data_ptr(), self._state.numel(), self.n_streams, *self._plan,
                                                    self.max_steps, _stream(self.device)), "adn_stream_reset")
        self._received = self._emitted = 0
        self._done = 0                 # steps run so far
        self._base = 0                 # index in the stream of the first pending sample
        self._fill = 0                 # pending samples per stream

    # ------------------------------------------------------------------ building blocks (device tensors)
    def analyze(self, audio: torch.Tensor, audio_stride: int, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        """``adn_stream_analyze``: the samples steps ``first_step ..`` bring -> network input ``(n_streams * n_steps, 1, F, W)``."""
        out = torch.empty((self.n_streams * n_steps, 1, self.n_bins, self.window_frames), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_stream_analyze(self._state.data_ptr(), self._state.numel(), audio.data_ptr(), audio_stride,
                                                      self.n_streams, first_step, n_steps, final_length, *self._plan, self.max_steps,
                                                      out.data_ptr(), _stream(self.device)), "adn_stream_analyze")
        return out

    def network(self, x: torch.Tensor) -> torch.Tensor:
        """The U-Net over ``batch_windows`` windows at a time, into slices of one output buffer (as ``Denoiser.network``)."""
        nw, _, f, w = x.shape
        dev = x.device
        y = torch.empty_like(x)
        m = self.model
        if m.training:
            raise RuntimeError("StreamDenoiser: the model is in train mode; call .eval()")
        L = _lib.load()
        handle = m._ensure_handle(dev)
        step, per = self.batch_windows, f * w * 4
        with torch.cuda.device(dev):
            for i in range(0, nw, step):
                n = min(step, nw - i)
                ws = m._workspace_for(n, f, w, dev)
                _lib.check(L.adn_unet_forward(handle, x.data_ptr() + i * per, y.data_ptr() + i * per, n, f, w, ws.data_ptr(),
                                              ws.numel(), _stream(dev)), "adn_unet_forward")
        return y

    def emit_count(self, first_step: int, n_steps: int, final_length: int = -1) -> int:
        """Samples per stream that ``emit`` returns for these steps."""
        half, per = self.n_fft // 2, self.block_frames * self.hop_length
        lo = max(0, first_step * per - half)
        hi = max(0, (first_step + n_steps) * per - half)
        if final_length >= 0:
            n_frames = 1 + final_length // self.hop_length
            if first_step + n_steps == -(-n_frames // self.block_frames):
                hi = final_length
        return max(0, hi - lo)

    def emit(self, y: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        """``adn_stream_emit``: the network's output for the windows of ``analyze`` -> ``(n_streams, emit_count)`` samples."""
        y = y.contiguous()
        n = self.emit_count(first_step, n_steps, final_length)
        out = torch.empty((self.n_streams, n), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_stream_emit(self._state.data_ptr(), self._state.numel(), y.data_ptr(), self.n_streams,
                                                   first_step, n_steps, final_length, *self._plan, self.max_steps,
                                                   out.data_ptr() if n else None, n, _stream(self.device)), "adn_stream_emit")
        return out

    def _run(self, n_steps: int, final_length: int = -1) -> torch.Tensor:
        """Steps ``_done .. _done + n_steps - 1`` on the pending samples; what they bring leaves the pending buffer."""
        first = self._done
        x = self.analyze(self._pend, self._cap, first, n_steps, final_length)
        out = self.emit(self.network(x), first, n_steps, final_length)
        end = self._end_of(first + n_steps - 1)
        used = min(max(end - self._base, 0), self._fill)
        rest = self._fill - used
        if rest:
            self._pend[:, :rest] = self._pend[:, used:self._fill].clone()
        self._fill, self._base, self._done = rest, end, first + n_steps
        return out

    # ------------------------------------------------------------------ public surface
    def _to_device(self, block) -> torch.Tensor:
        self._numpy = not isinstance(block, torch.Tensor)
        if self._numpy:
            x = torch.from_numpy(np.ascontiguousarray(block, dtype=np.float32)).to(self.device)
        else:
            x = block
            if not x.is_cuda:
                raise RuntimeError("StreamDenoiser.push: a tensor must live on a ROCm device (no CPU path); pass numpy to have it staged")
            if x.dtype != torch.float32:
                raise TypeError("StreamDenoiser.push: expected float32 audio")
            x = x.to(self.device)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[0] != self.n_streams:
            raise ValueError(f"StreamDenoiser.push: audio must be (m,) for one stream or (n_streams, m) = ({self.n_streams}, m)")
        return x

    def _cat(self, outs) -> torch.Tensor:
        return torch.cat(outs, dim=1) if outs else torch.empty((self.n_streams, 0), dtype=torch.float32, device=self.device)

    def _result(self, outs):
        out = self._cat(outs)
        return out.cpu().numpy() if self._numpy else out

    def push(self, block):
        """``block``: the next ``m >= 0`` samples of every stream at ``input_rate`` (``sample_rate`` unless given), ``(m,)`` for
        one stream or ``(n_streams, m)``, float32.  Returns the samples that have become final, at the same rate, ``(n_streams,
        emitted(received) - emitted(before))`` (``stream_plan``; ``stream_rate_plan`` with an ``input_rate``) -- zero columns while no
        step completes; numpy in -> numpy out, a tensor on the ROCm device in -> a tensor there out.  Everything between the input copy and the output copy runs on the device on the current stream."""
        x = self._to_device(block)
        if self._rs_in is None:
            return self._result(self._push_steps(x))
        return self._result([self._rs_out.push(self._cat(self._push_steps(self._rs_in.push(x))))])

    def _push_steps(self, x: torch.Tensor):
        """``x`` (n_streams, m) at the working rate on the device -> the list of tensors the completed steps returned."""
        m, pos, outs = x.shape[1], 0, []
        if self._received + m >= 1 << 30:
            raise ValueError("StreamDenoiser.push: a stream holds fewer than 2^30 samples; flush() it before")
        while True:
            take = min(m - pos, self._cap - self._fill)
            if take:
                self._pend[:, self._fill:self._fill + take] = x[:, pos:pos + take]
                self._fill += take
                pos += take
            n = min(stream_plan(self._base + self._fill, *self._plan)[0] - self._done, self.max_steps)
            if n > 0:
                outs.append(self._run(n))
            elif pos >= m:
                break
        self._received += m
        self._emitted = stream_plan(self._received, *self._plan)[1]
        return outs

    def flush(self):
        """The stream has ended: runs the remaining steps (frames that reach past the end zero padded) and returns the rest, so that
        the stream has produced exactly ``received`` samples, in the kind (numpy / tensor) of the last ``push``.  The object is then
        ready for a new stream.  With an ``input_rate`` the three stages end in order -- the resampler in, the steps, the resampler
        out -- and the result is cut to the input's length (``ceil(ceil(L up / down) down / up) >= L``)."""
        if self._rs_in is None or self._rs_in.received == 0:
            out = self._result(self._flush_steps())
            self.reset()
            return out
        length, before = self._rs_in.received, self._rs_out.emitted
        outs = self._push_steps(self._rs_in.flush())
        out = self._cat([self._rs_out.push(self._cat(outs + self._flush_steps())), self._rs_out.flush()])
        assert before <= length <= before + out.shape[1], (before, out.shape, length)
        out = self._result([out[:, :length - before]])
        self.reset()
        return out

    def _flush_steps(self):
        """The remaining steps of the stream at the working rate -> the list of tensors they returned."""
        length, outs = self._received, []
        if length:
            n_frames = 1 + length // self.hop_length
            k = -(-n_frames // self.block_frames)
            while self._done < k:
                outs.append(self._run(min(self.max_steps, k - self._done), length))
        assert self._emitted + sum(o.shape[1] for o in outs) == length, (self._emitted, length)
        return outs


def main(argv=None) -> int:
    import argparse

    from .denoise import _load_model
    from .resample import _resample_device
    from .wav import read_wav, write_wav
    ap = argparse.ArgumentParser(prog="python -m audiodenoiser_amd.stream",
                                 description="Denoise a wav file by feeding it to the streaming denoiser chunk by chunk.")
    ap.add_argument("--model", required=True, help="checkpoint: the state_dict of UNet(1, 1) (reference train.py:142)")
    ap.add_argument("src", metavar="IN", help="the wav file to read")
    ap.add_argument("dst", metavar="OUT", help="the wav file to write")
    ap.add_argument("--chunk", type=int, default=1024, help="samples per push at the working rate (with --live: at the file's rate)")
    ap.add_argument("--live", action="store_true",
                    help="push the file at its own rate, as a live feed arrives: the rate is converted inside the stream")
    ap.add_argument("--window", type=int, default=192)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--lookahead", type=int, default=0)
    ap.add_argument("--dtype", choices=("f32", "f16"), default="f32")
    args = ap.parse_args(argv)
    if args.chunk < 1:
        ap.error("--chunk must be >= 1")
    dev = _lib.staging_device()
    audio, rate = read_wav(args.src, mono=False)             # (L, channels): every channel is a stream
    x = torch.from_numpy(np.ascontiguousarray(audio.T, dtype=np.float32)).to(dev)
    sd = StreamDenoiser(_load_model(args.model, args.dtype, dev), n_streams=x.shape[0], window_frames=args.window,
                        block_frames=args.block, lookahead_frames=args.lookahead, input_rate=rate if args.live else None)
    length = x.shape[1]
    if rate != sd.input_rate:                                # not --live: the file is converted as a whole, before and after
        x = _resample_device(x, rate, sd.sample_rate)
    outs = [sd.push(x[:, i:i + args.chunk]) for i in range(0, x.shape[1], args.chunk)]
    outs.append(sd.flush())
    out = torch.cat(outs, dim=1)
    if rate != sd.input_rate:
        up = _resample_device(out, sd.sample_rate, rate)
        out = torch.zeros((x.shape[0], length), dtype=torch.float32, device=dev)
        n = min(length, up.shape[1])
        out[:, :n] = up[:, :n]
    write_wav(args.dst, np.ascontiguousarray(out.cpu().numpy().T), rate)
    print(f"{args.src} -> {args.dst}: {length} samples at {rate} Hz in pushes of {args.chunk}"
          f"{' at its own rate' if args.live else ''}, latency {sd.latency_input_samples if args.live else sd.latency_samples} samples")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
