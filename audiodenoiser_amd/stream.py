"""Streaming denoiser: audio that is still arriving, in blocks, with the state carried on the device.

    from audiodenoiser_amd import StreamDenoiser
    sd = StreamDenoiser(model, n_streams=1)           # an audiodenoiser_amd.model.UNet(1, 1) on a ROCm device, .eval()
    for block in feed:                                # (m,) or (n_streams, m) float32 at sample_rate, any m >= 0
        out = sd.push(block)                          # (n_streams, newly final samples), possibly zero columns
    out = sd.flush()                                  # the rest: exactly as many samples out as went in
    sd = StreamDenoiser(model, input_rate=48000)      # the same for a feed at 48 kHz: samples at 48 kHz in, samples at 48 kHz out
    pool = StreamPool(model, max_streams=64)          # feeds that start, stop and arrive independently, at their own rates: see StreamPool

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
timing go into one ``StreamPool``, which batches their ready steps.  A ``push`` that completes several steps sends them through the network as one batch,
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
from ._host import check_stft_plan, model_device, run_live, stage, unet_windows
from ._host import current_stream as _stream          # the name this module's methods have always called it by
from .resample import prepare_resample, resample_stream_plan

__all__ = ["StreamDenoiser", "StreamPool", "PoolBook", "RecordingBook", "stream_plan", "stream_rate_plan"]


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


def end_of(plan, step: int) -> int:
    """Samples that must have arrived for ``step`` of a running stream with ``plan`` = ``(n_fft, hop, W, B, A)`` to run (``e(k)`` of
    adn.h; 0 for step -1)."""
    n_fft, hop, _, b, a = plan
    return (step * b + b + a - 1) * hop + n_fft // 2 if step >= 0 else 0


def n_steps(plan, length: int) -> int:
    """``K``: the steps of a finished stream of ``length`` samples (0 for an empty one)."""
    return -(-(1 + length // plan[1]) // plan[3]) if length > 0 else 0


def causal_carrier(block_frames):
    """``(window_frames, lookahead_frames, batch_windows)`` of a lockstep class whose operator is causal and reads only the
    ``block_frames`` columns a step keeps: no look-ahead, the window only the carrier the stream geometry needs (the narrowest
    one the library takes), 64 rows a call.  A ``block_frames`` that is no integer is left for the argument check to name."""
    return (max(16, block_frames) if isinstance(block_frames, int) else 16), 0, 64


def _emit_count(n_fft: int, hop: int, block: int, first_step: int, n_steps: int, final_length: int = -1) -> int:
    """Samples ``adn_stream_emit`` returns per stream for steps ``first_step .. first_step + n_steps - 1``."""
    half, per = n_fft // 2, block * hop
    lo = max(0, first_step * per - half)
    hi = max(0, (first_step + n_steps) * per - half)
    if final_length >= 0:
        n_frames = 1 + final_length // hop
        if first_step + n_steps == -(-n_frames // block):
            hi = final_length
    return max(0, hi - lo)


def _check_step_plan(who, sample_rate, n_fft, hop_length, window_frames, block_frames, lookahead_frames):
    """The plan of a stream's steps, lockstep or pooled: the transform, then window, block and look-ahead."""
    check_stft_plan(who, n_fft, hop_length, sample_rate)
    if not (isinstance(window_frames, int) and window_frames >= 16):
        raise ValueError(f"{who}: window_frames must be >= 16 (the network pools four times)")
    if not (isinstance(block_frames, int) and block_frames >= 1):
        raise ValueError(f"{who}: block_frames must be >= 1")
    if not (isinstance(lookahead_frames, int) and lookahead_frames >= 0):
        raise ValueError(f"{who}: lookahead_frames must be >= 0")
    if block_frames + lookahead_frames > window_frames:
        raise ValueError(f"{who}: need block_frames + lookahead_frames <= window_frames")


def _check_stream_args(who, n_streams, sample_rate, n_fft, hop_length, window_frames, block_frames, lookahead_frames, batch_windows,
                       input_rate):
    """The model-free argument checks of ``StreamDenoiser`` (``who``: the class the messages name)."""
    if not (isinstance(n_streams, int) and n_streams >= 1):
        raise ValueError(f"{who}: n_streams must be >= 1")
    _check_step_plan(who, sample_rate, n_fft, hop_length, window_frames, block_frames, lookahead_frames)
    if not (isinstance(batch_windows, int) and batch_windows >= 1):
        raise ValueError(f"{who}: batch_windows must be >= 1")
    if input_rate is not None and not (isinstance(input_rate, int) and input_rate >= 1):
        raise ValueError(f"{who}: input_rate must be None (the feed is at sample_rate) or an integer >= 1")


class StreamDenoiser:
    def __init__(self, model, n_streams: int = 1, sample_rate: int = 8000, n_fft: int = 512, hop_length: int = 128,
                 window_frames: int = 192, block_frames: int = 16, lookahead_frames: int = 0, batch_windows: int = 64,
                 input_rate=None):
        _check_stream_args("StreamDenoiser", n_streams, sample_rate, n_fft, hop_length, window_frames, block_frames, lookahead_frames,
                           batch_windows, input_rate)
        self.model = model
        self._setup(model_device("StreamDenoiser", model), n_streams, sample_rate, n_fft, hop_length, window_frames, block_frames,
                    lookahead_frames, batch_windows, input_rate)

    def _setup(self, dev, n_streams, sample_rate, n_fft, hop_length, window_frames, block_frames, lookahead_frames, batch_windows,
               input_rate):
        """Everything of the constructor that needs no model: the plan, the device state, the pending buffer, the resamplers."""
        self.device = dev
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
        self._cap = end_of(self._plan, 0) + self.max_steps * block_frames * hop_length
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
        return unet_windows("StreamDenoiser", self.model, x, self.batch_windows)

    def _net(self, x: torch.Tensor, first_step: int, n_steps: int, final_length: int = -1) -> torch.Tensor:
        """What stands between ``analyze`` and ``emit`` for steps ``first_step ..`` of a stream that runs (``final_length`` -1) or has
        ended at that length (``x``: a stream's ``n_steps`` steps consecutive): here the network, which needs none of the numbers."""
        return self.network(x)

    def emit_count(self, first_step: int, n_steps: int, final_length: int = -1) -> int:
        """Samples per stream that ``emit`` returns for these steps."""
        return _emit_count(self.n_fft, self.hop_length, self.block_frames, first_step, n_steps, final_length)

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
        out = self.emit(self._net(x, first, n_steps, final_length), first, n_steps, final_length)
        end = end_of(self._plan, first + n_steps - 1)
        used = min(max(end - self._base, 0), self._fill)
        rest = self._fill - used
        if rest:
            self._pend[:, :rest] = self._pend[:, used:self._fill].clone()
        self._fill, self._base, self._done = rest, end, first + n_steps
        return out

    # ------------------------------------------------------------------ public surface
    def _to_device(self, block) -> torch.Tensor:
        x, self._numpy = stage("StreamDenoiser.push", block, self.device)
        if not self._numpy:
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
        k = n_steps(self._plan, length)
        while self._done < k:
            outs.append(self._run(min(self.max_steps, k - self._done), length))
        assert self._emitted + sum(o.shape[1] for o in outs) == length, (self._emitted, length)
        return outs


POOL_MAX_ROWS = 256          # ADN_STREAM_POOL_MAX_ROWS of include/adn.h: the rows of one analyze / emit call
POOL_RATE_MAX_ROWS = 64      # ADN_STREAM_POOL_RATE_MAX_ROWS: the rows of one push_rate / emit_rate call


def _rs_emitted(received: int, src: int, dst: int, final: bool = False) -> int:
    return resample_stream_plan(received, src, dst, final)[0]


class PoolBook:
    """The host side of a ``StreamPool``, no device needed: per slot ``received`` (samples pushed) and ``done`` (steps run), and
    what follows from them -- which step is ready, how many samples it returns, how much room the slot's ring has left.

    ``ring_samples`` = ``n_fft - hop`` (the history a step's first frame shares with the step before) + ``e(0)`` (what the first
    step reads) + ``backlog_steps`` blocks of ``B hop`` samples that may wait while their step has not run.

    ``input_rates``: the rates streams may be opened at (None: the working rate only, and nothing below applies).  A stream at
    another rate than ``sample_rate`` has, per slot, ``rate``, the calls made so far to its two resamplers (``calls_in``,
    ``calls_out``), ``received_in`` (samples pushed, at its rate), ``work_out`` (working-rate samples its steps have returned, all
    handed to the resampler out) and ``emitted_in`` (samples returned, at its rate); ``received`` stays what the ring has received,
    at the working rate.  All of it follows from ``adn_resample_stream_plan``.  The ring grows by ``reserve`` samples, the most the
    resampler in still releases when a stream ends, and ``room`` keeps them free."""
    FREE, RUNNING, CLOSED = 0, 1, 2

    def __init__(self, max_streams: int = 64, backlog_steps: int = 4, n_fft: int = 512, hop_length: int = 128,
                 window_frames: int = 192, block_frames: int = 16, lookahead_frames: int = 0, input_rates=None,
                 sample_rate: int = 8000):
        _check_step_plan("StreamPool", sample_rate, n_fft, hop_length, window_frames, block_frames, lookahead_frames)
        rates = () if input_rates is None else tuple(input_rates)
        if not all(isinstance(r, int) and r >= 1 for r in rates):
            raise ValueError("StreamPool: input_rates must be None or integers >= 1")
        if not (isinstance(max_streams, int) and 1 <= max_streams <= 1 << 20):
            raise ValueError("StreamPool: max_streams must be in [1, 2^20]")
        if not (isinstance(backlog_steps, int) and backlog_steps >= 1):
            raise ValueError("StreamPool: backlog_steps must be >= 1")
        self.max_streams, self.backlog_steps = max_streams, backlog_steps
        self.n_fft, self.hop_length, self.window_frames = n_fft, hop_length, window_frames
        self.block_frames, self.lookahead_frames = block_frames, lookahead_frames
        self.plan = (n_fft, hop_length, window_frames, block_frames, lookahead_frames)
        self.keep = n_fft - hop_length
        self.out_stride = block_frames * hop_length + n_fft // 2          # the most a step returns (the last one of a stream)
        # the rates: history both ways, what the resampler in releases at a stream's end, the most a step returns at a stream's rate
        self.sample_rate, self.input_rates = sample_rate, tuple(sorted(set(rates) - {sample_rate}))
        self.max_history = self.reserve = self.rate_out_stride = 0
        for r in self.input_rates:
            g = math.gcd(r, sample_rate)
            up, down = sample_rate // g, r // g                           # rate -> working rate
            half = 32 * max(up, down)                                     # adn.h, "resample": half = ZEROS max(up, down)
            if resample_stream_plan(0, r, sample_rate)[2] != -(-half // up) or resample_stream_plan(0, sample_rate, r)[2] != -(-half // down):
                raise RuntimeError("StreamPool: the library's resampling filter is not the one the ring reserve is sized for")
            self.max_history = max(self.max_history, resample_stream_plan(0, r, sample_rate)[1], resample_stream_plan(0, sample_rate, r)[1])
            # ceil(n up / down) - emitted(n) <= (half + 1) / down + 2 for every n;  back out: up and down change places
            self.reserve = max(self.reserve, (half + 1) // down + 2)
            self.rate_out_stride = max(self.rate_out_stride, (self.out_stride * down + half + 1) // up + 2)
        self.ring_samples = self.keep + self.end_of(0) + backlog_steps * block_frames * hop_length + self.reserve
        if self.ring_samples > 1 << 28:
            raise ValueError("StreamPool: backlog_steps asks for a ring of more than 2^28 samples per stream")
        self.status = [self.FREE] * max_streams
        self.received = [0] * max_streams
        self.done = [0] * max_streams
        self.rate = [None] * max_streams                                  # None: the stream is at the working rate
        self.calls_in, self.calls_out = [0] * max_streams, [0] * max_streams
        self.received_in, self.work_out, self.emitted_in = [0] * max_streams, [0] * max_streams, [0] * max_streams

    def end_of(self, step: int) -> int:
        """Samples that must have arrived for ``step`` of a running stream (``e(k)`` of adn.h; 0 for step -1)."""
        return end_of(self.plan, step)

    def n_steps(self, length: int) -> int:
        """``K``: the steps of a finished stream of ``length`` samples (0 for an empty one)."""
        return n_steps(self.plan, length)

    def _live(self, slot, what):
        if not (isinstance(slot, int) and 0 <= slot < self.max_streams) or self.status[slot] == self.FREE:
            raise ValueError(f"StreamPool.{what}: {slot!r} is not an open stream")

    def open(self, input_rate=None) -> int:
        if input_rate is not None and input_rate != self.sample_rate and input_rate not in self.input_rates:
            raise ValueError(f"StreamPool.open: input_rate {input_rate!r} is not among the pool's input_rates {self.input_rates}")
        for slot, st in enumerate(self.status):
            if st == self.FREE:
                self.status[slot], self.received[slot], self.done[slot] = self.RUNNING, 0, 0
                self.rate[slot] = None if input_rate == self.sample_rate else input_rate
                self.calls_in[slot] = self.calls_out[slot] = 0
                self.received_in[slot] = self.work_out[slot] = self.emitted_in[slot] = 0
                return slot
        raise RuntimeError(f"StreamPool.open: all {self.max_streams} streams are taken")

    def room(self, slot: int) -> int:
        """Samples that fit before a push would overwrite one that the stream's next step still reads: the ring holds the last
        ``ring_samples`` samples, the next step reads from ``e(done - 1) - (n_fft - hop)`` on.  For a stream at a rate of its own,
        in samples at that rate: the largest ``m`` after which the stream could still END inside the ring --
        ``ceil((received_in + m) up / down)`` working-rate samples, what the resampler in releases at the end included."""
        self._live(slot, "room")
        oldest = max(0, self.end_of(self.done[slot] - 1) - self.keep)
        if self.rate[slot] is None:
            return oldest + self.ring_samples - self.received[slot]
        if self.status[slot] == self.CLOSED:
            return 0
        g = math.gcd(self.rate[slot], self.sample_rate)
        up, down = self.sample_rate // g, self.rate[slot] // g
        return max(0, (oldest + self.ring_samples) * down // up - self.received_in[slot])

    def take(self, slot: int, m: int) -> int:
        """Book a push of ``m`` samples; returns the position they start at.  Changes nothing when it raises."""
        self.check(slot, m)
        at = self.received[slot]
        self.received[slot] = at + m
        return at

    def check(self, slot: int, m: int) -> None:
        """What ``take`` raises, without booking anything."""
        self._live(slot, "push")
        if self.status[slot] == self.CLOSED:
            raise RuntimeError("StreamPool.push: the stream has been closed")
        if m > self.room(slot):
            raise RuntimeError(f"StreamPool.push: {m} samples do not fit, the stream has room for {self.room(slot)} before samples "
                               "that no step has used yet would be overwritten; call step()")
        if self.received[slot] + m >= 1 << 30:
            raise ValueError("StreamPool.push: a stream holds fewer than 2^30 samples; close() it before")

    def check_rate(self, slot: int, m: int) -> None:
        """What ``take_rate`` raises, without booking anything."""
        self._live(slot, "push")
        if self.status[slot] == self.CLOSED:
            raise RuntimeError("StreamPool.push: the stream has been closed")
        if m > self.room(slot):
            raise RuntimeError(f"StreamPool.push: {m} samples do not fit, the stream has room for {self.room(slot)} at its rate before "
                               "samples that no step has used yet would be overwritten; call step()")
        if self.received_in[slot] + m >= 1 << 31 or _rs_emitted(self.received_in[slot] + m, self.rate[slot], self.sample_rate, True) >= 1 << 30:
            raise ValueError("StreamPool.push: a stream holds fewer than 2^30 samples at the working rate; close() it before")

    def take_rate(self, slot: int, m: int):
        """Book a push of ``m >= 1`` samples at the stream's own rate -> ``(call_index, received_before)`` of the call to the
        resampler in; ``received`` becomes what the ring holds after it.  Changes nothing when it raises."""
        self.check_rate(slot, m)
        call = self.calls_in[slot], self.received_in[slot]
        self.calls_in[slot] += 1
        self.received_in[slot] += m
        self.received[slot] = _rs_emitted(self.received_in[slot], self.rate[slot], self.sample_rate)
        return call

    def close_rate(self, slot: int):
        """The end of a stream at a rate of its own with ``received_in > 0``: -> ``(call_index, received_before)`` of the resampler
        in's final call (``n_new = 0``), which the caller has to enqueue; ``received`` becomes the stream's working-rate length."""
        call = self.calls_in[slot], self.received_in[slot]
        self.calls_in[slot] += 1
        self.received[slot] = _rs_emitted(self.received_in[slot], self.rate[slot], self.sample_rate, True)
        return call

    def count_rate(self, slot: int, n: int, last: bool) -> int:
        """Samples at the stream's rate that the resampler out returns for the ``n`` working-rate samples of the stream's next
        step; ``last``: it is the stream's last step, and the result is cut to the samples the stream received."""
        total = _rs_emitted(self.work_out[slot] + n, self.sample_rate, self.rate[slot], last)
        if last:                                                          # ceil(ceil(L up / down) down / up) >= L
            total = self.received_in[slot]
        return total - self.emitted_in[slot]

    def ran_rate(self, slot: int, n: int, last: bool):
        """Book the call to the resampler out for a step that returned ``n`` working-rate samples -> ``(call_index,
        received_before, samples returned at the stream's rate)``, or None when there is no call (nothing new, not the end)."""
        if n == 0 and not last:
            return None
        call = self.calls_out[slot], self.work_out[slot], self.count_rate(slot, n, last)
        self.calls_out[slot] += 1
        self.work_out[slot] += n
        self.emitted_in[slot] += call[2]
        return call

    def rate_calls(self, rows):
        """Book the resampler out's calls of a tick's ``rows`` (``self.rows()``) -> ``(calls, where)``: ``calls`` = ``(row, rate row)``
        per row that makes one, in row order, the rate row ``(slot, rate, call_index, received_before, n_new, final, 0)``;
        ``where[row]`` = ``(index into calls or None, samples returned at the stream's rate)`` for every row of a stream at a rate
        of its own.  Rows of working-rate streams and rows that returned nothing yet make no call."""
        calls, where = [], {}
        for i, (slot, k, final) in enumerate(rows):
            if self.rate[slot] is None:
                continue
            n = self.count(k, final)
            last = final >= 0 and k == self.n_steps(final) - 1
            call = self.ran_rate(slot, n, last)
            if call is None:
                where[i] = (None, 0)
            else:
                where[i] = (len(calls), call[2])
                calls.append((i, (slot, self.rate[slot], call[0], call[1], n, 1 if last else 0, 0)))
        return calls, where

    def close(self, slot: int) -> bool:
        """The stream has ended.  True when nothing is left to run (a stream of no samples): the slot is free again."""
        self._live(slot, "close")
        self.status[slot] = self.CLOSED
        if self.done[slot] >= self.n_steps(self.received[slot]):
            self.status[slot] = self.FREE
            return True
        return False

    def ready(self, slot: int):
        """``(step, final_length)`` of the step the stream in ``slot`` can run now, or None."""
        st, k = self.status[slot], self.done[slot]
        if st == self.RUNNING and self.received[slot] >= self.end_of(k):
            return k, -1
        if st == self.CLOSED and k < self.n_steps(self.received[slot]):
            return k, self.received[slot]
        return None

    def rows(self):
        """The ready rows ``(slot, step, final_length)`` of one tick, in ascending slot order."""
        out = []
        for slot in range(self.max_streams):
            r = self.ready(slot)
            if r is not None:
                out.append((slot,) + r)
        return out

    def count(self, step: int, final_length: int) -> int:
        """Samples the step returns (``adn_stream_emit``'s count for one step)."""
        return _emit_count(self.n_fft, self.hop_length, self.block_frames, step, 1, final_length)

    def ran(self, slot: int) -> bool:
        """Book the step that ``ready`` named as run; True when it was the last one of a closed stream (the slot is free again)."""
        self.done[slot] += 1
        if self.status[slot] == self.CLOSED and self.done[slot] >= self.n_steps(self.received[slot]):
            self.status[slot] = self.FREE
            return True
        return False


class RecordingBook(PoolBook):
    """A ``PoolBook`` over RECORDINGS of ``channels`` microphones (``include/adn.h``, ``adn_wpe_mc_stream_pool``): everything the
    parent keeps -- ``received``, ``done``, ``room``, the rates -- exists once per recording, because the channels of a recording
    start, advance and end together.  Recording ``r`` owns the stream slots ``r C ... r C + C - 1`` of the device state, so a row
    ``(rid, step, final_length)`` of a tick expands to ``C`` stream rows in channel order (``stream_rows``), and a tick is cut into
    calls of ``256 // C`` recordings (``calls``): a recording never straddles two calls.  One channel count per pool."""

    def __init__(self, max_recordings: int = 16, channels: int = 2, backlog_steps: int = 4, n_fft: int = 512, hop_length: int = 128,
                 window_frames: int = 192, block_frames: int = 16, lookahead_frames: int = 0, input_rates=None,
                 sample_rate: int = 8000):
        if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= 8:
            raise ValueError("StreamPool: channels must be an integer in [1, 8]")
        if not (isinstance(max_recordings, int) and 1 <= max_recordings and max_recordings * channels <= 1 << 20):
            raise ValueError("StreamPool: max_recordings * channels must be in [1, 2^20]")
        super().__init__(max_recordings, backlog_steps, n_fft, hop_length, window_frames, block_frames, lookahead_frames, input_rates,
                         sample_rate)
        self.channels, self.max_recordings = channels, max_recordings
        self.n_slots = max_recordings * channels                          # stream slots of the device state
        self.recordings_per_call = POOL_MAX_ROWS // channels

    def slots(self, rid: int):
        """The stream slots of recording ``rid``, in channel order."""
        return range(rid * self.channels, (rid + 1) * self.channels)

    def stream_rows(self, rows):
        """``rows`` ``(rid, step, final_length)`` -> the stream rows ``(slot, step, final_length)``, ``C`` per recording."""
        return [(slot, k, final) for rid, k, final in rows for slot in self.slots(rid)]

    def calls(self, rows):
        """``rows`` of recordings cut into the lists one library call takes: ``256 // C`` recordings each."""
        n = self.recordings_per_call
        return [rows[i:i + n] for i in range(0, len(rows), n)]


class StreamPool:
    """Live streams that start, stop and arrive independently, served from one card: every ``step()`` runs ONE step of every
    stream that has one ready, all of them through the network as one batch.

        pool = StreamPool(model, max_streams=64)      # an audiodenoiser_amd.model.UNet(1, 1) on a ROCm device, .eval()
        sid = pool.open()                             # a free slot; RuntimeError when all are taken
        pool.push(sid, block)                         # the next m >= 0 samples of THAT stream, (m,) float32, numpy or device tensor
        pool.close(sid)                               # the stream has ended; its remaining steps run in the following ticks
        for sid, samples, finished in pool.step():    # the newly final samples of every stream that ran a step
            ...

    Definition: ``include/adn.h``, "stream pool" -- ``max_streams`` independent instances of the "stream" definition; kernels:
    ``csrc/stream_kernels.hip``, the lockstep kernels' bodies with one (slot, step, final_length) row per stream in the kernel
    arguments.  A stream's samples wait in a ring on the device (``backlog_steps`` blocks beyond what one step reads); the frames
    still to be emitted, the magnitudes of the last ``window_frames`` frames and the overlap-add tail live there too.  The host
    keeps two numbers per stream, ``received`` and ``done`` (``PoolBook``).  Step ``k`` of a running stream is ready once
    ``(k B + B + A - 1) hop + n_fft / 2`` samples have arrived; every remaining step of a closed stream is ready.  A tick gathers
    the ready rows in ascending slot order, analyses them (``adn_stream_pool_analyze``, at most 256 rows a call), sends the
    windows through the U-Net ``batch_windows`` at a time, and takes the result back to audio (``adn_stream_pool_emit``).

    What is claimed: a stream's output is a function of its own samples and its own step index only -- bit for bit, with
    ``model.set_batch_invariant(True)``, what a ``StreamDenoiser(n_streams=1)`` returns for the same samples, whatever the other
    slots carry, whenever they were opened and however the pushes and ticks interleave (within the network's per-batch-size
    bound otherwise); each stream returns exactly as many samples as it received; a slot is free again, and reusable without a
    reset, once the tick that reports ``finished=True`` has run.  ``push`` beyond ``room`` raises and changes nothing.
    What is NOT claimed: anything ``StreamDenoiser`` does not claim; fairness, priorities or deadlines between streams; more than
    one step per stream and tick (a stream that is several steps behind catches up one tick at a time); graph capture of a tick.
    There is no CPU path.  Samples come back in the kind (numpy / device tensor) of the stream's last ``push``.

    Feeds at their own rates (``include/adn.h``, "stream pool at a rate"; kernel: ``csrc/stream_resample_kernels.hip``, the
    lockstep resampler's body over a by-value table of rows that each carry their own stream):

        pool = StreamPool(model, input_rates=(48000, 44100, 16000))      # the rates streams may be opened at
        sid = pool.open(input_rate=48000)                                # push, room and the samples of step(): at 48 kHz
        pool.push_many({sid: block, other: block2})                      # all blocks: one staging copy, one launch per 64 streams

    ``input_rates`` sizes the resamplers' history (``max_history``), the row of a step's samples at the fastest rate and the
    ring's reserve; None gives exactly the pool above.  A push goes through ``adn_stream_pool_push_rate`` straight into the ring,
    the rows of a tick that ran go back through ``adn_stream_pool_emit_rate``; ``close`` enqueues the resampler in's last call,
    for whose samples ``room`` has kept the ring free, and the stream's last step is cut so that it has returned exactly as many
    samples as it received.  Claimed: a stream's output is, bit for bit with ``set_batch_invariant(True)``, that of
    ``StreamDenoiser(n_streams=1, input_rate=rate)`` for the same samples, whatever rates and timing its neighbours have.  Not
    claimed: rates outside ``adn_resample``'s limits; anything ``StreamDenoiser(input_rate=...)`` does not claim.

    Recordings.  A subclass whose ``book`` is a ``RecordingBook`` (``DereverbStreamPool(channels=C)``, ``BeamformStreamPool``) serves
    RECORDINGS of ``C`` microphones: ``open`` returns a recording id, ``push`` takes ``(C, m)``, recording ``r`` lives in the device
    slots ``r C ... r C + C - 1``, a tick's rows are its recordings' ``C`` stream rows in channel order, ``256 // C`` recordings a
    call, and ``step`` returns ``(C, k)`` per recording -- or ``(E, k)`` where ``_emit_rows`` keeps ``E`` rows of each, ``(k,)`` for
    ``E = 1``.  This class
    itself, and every pool with ``channels = 1``, is the pool of single streams above."""

    def __init__(self, model, max_streams: int = 64, backlog_steps: int = 4, n_fft: int = 512, hop_length: int = 128,
                 window_frames: int = 192, block_frames: int = 16, lookahead_frames: int = 0, batch_windows: int = 64,
                 input_rates=None, sample_rate: int = 8000):
        self.book = PoolBook(max_streams, backlog_steps, n_fft, hop_length, window_frames, block_frames, lookahead_frames,
                             input_rates, sample_rate)
        if not (isinstance(batch_windows, int) and batch_windows >= 1):
            raise ValueError("StreamPool: batch_windows must be >= 1")
        dev = model_device("StreamPool", model)
        self.model, self.batch_windows = model, batch_windows
        self._setup(dev)

    def _setup(self, dev):
        """Everything of the constructor that needs no model, ``self.book`` given: the device state and the rates' histories.
        With a ``RecordingBook`` a stream of the pool is a recording of ``channels`` device slots; ``max_streams`` counts recordings."""
        max_streams = self.book.max_streams
        self.device = dev
        self.max_streams, self.n_bins = max_streams, self.book.n_fft // 2 + 1
        self.channels = getattr(self.book, "channels", 1)
        n_slots = max_streams * self.channels
        self._args = (n_slots,) + self.book.plan + (self.book.ring_samples,)
        need = ctypes.c_size_t()
        _lib.check(_lib.load().adn_stream_pool_state_bytes(*self._args, ctypes.byref(need)), "adn_stream_pool_state_bytes")
        self._state = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self._numpy = [True] * max_streams
        # streams at a rate of their own: the histories of their resamplers, two directions per slot (none without input_rates)
        self._rate_state = None
        if self.book.input_rates:
            _lib.check(_lib.load().adn_stream_pool_rate_state_bytes(n_slots, self.book.max_history, ctypes.byref(need)),
                       "adn_stream_pool_rate_state_bytes")
            self._rate_state = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
            self._rate_args = (self._rate_state.data_ptr(), need.value, n_slots, self.book.max_history, self.book.sample_rate)
            for r in self.book.input_rates:                  # the coefficient tables, so that no push builds one
                prepare_resample(r, self.book.sample_rate, dev)
                prepare_resample(self.book.sample_rate, r, dev)
        self.reset()

    @property
    def latency_samples(self) -> int:
        return stream_plan(0, *self.book.plan)[2]

    def reset(self):
        """Forget every stream: all slots are free."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_stream_pool_reset(self._state.data_ptr(), self._state.numel(), *self._args, -1,
                                                         _stream(self.device)), "adn_stream_pool_reset")
        b = self.book
        b.status, b.received, b.done = [b.FREE] * self.max_streams, [0] * self.max_streams, [0] * self.max_streams

    # ------------------------------------------------------------------ streams
    def open(self, input_rate=None) -> int:
        """A free slot for a new stream (the lowest one); ``RuntimeError`` when all ``max_streams`` are taken.  ``input_rate``: the
        rate of the stream's samples, in and out, one of the pool's ``input_rates`` (None: the working rate)."""
        return self.book.open(input_rate)

    def room(self, sid: int) -> int:
        """Samples, at the stream's rate, that still fit before a ``push`` would overwrite samples no step has used yet."""
        return self.book.room(sid)

    def received(self, sid: int) -> int:
        """Samples pushed so far, at the stream's rate."""
        self.book._live(sid, "received")
        return self.book.received[sid] if self.book.rate[sid] is None else self.book.received_in[sid]

    def push(self, sid: int, block) -> None:
        """The next ``m >= 0`` samples of stream ``sid``: ``(m,)`` float32, numpy or a tensor on the ROCm device.  More than
        ``room(sid)`` raises ``RuntimeError`` and changes nothing: call ``step()`` first."""
        self.book._live(sid, "push")
        if self.book.rate[sid] is not None:
            return self.push_many({sid: block})
        x, as_numpy = self._block(block)
        m = x.shape[-1]
        at = self.book.take(sid, m)
        self._numpy[sid] = as_numpy
        if m == 0:
            return
        x = x.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            for c in range(self.channels):                   # a recording: channel c into slot sid C + c, one write each
                _lib.check(_lib.load().adn_stream_pool_write(self._state.data_ptr(), self._state.numel(), *self._args,
                                                             sid * self.channels + c, x.data_ptr() + 4 * c * m, m, at,
                                                             _stream(self.device)), "adn_stream_pool_write")

    def _block(self, block):
        """``block`` as a float32 tensor of one dimension (on the host for numpy) and whether it was numpy; ``(channels, m)`` in a
        pool of recordings."""
        x, as_numpy = stage("StreamPool.push", block, None)
        if self.channels == 1:
            if x.dim() != 1:
                raise ValueError("StreamPool.push: audio must be (m,), the samples of one stream")
        elif x.dim() != 2 or x.shape[0] != self.channels:
            raise ValueError(f"StreamPool.push: audio must be (channels, m) = ({self.channels}, m), the samples of one recording")
        return x, as_numpy

    def _rate_rows(self, rows):
        return (_lib.StreamPoolRateRow * len(rows))(*[_lib.StreamPoolRateRow(*r) for r in rows])

    def _push_rate(self, rows, audio) -> None:
        """``adn_stream_pool_push_rate``: rows ``(slot, rate, call_index, received_before, n_new, final, audio_offset)`` -> rings."""
        L = _lib.load()
        with torch.cuda.device(self.device):
            for i in range(0, len(rows), POOL_RATE_MAX_ROWS):
                g = rows[i:i + POOL_RATE_MAX_ROWS]
                _lib.check(L.adn_stream_pool_push_rate(self._state.data_ptr(), self._state.numel(), *self._args, *self._rate_args[:2],
                                                       *self._rate_args[3:], self._rate_rows(g), len(g),
                                                       audio.data_ptr() if audio is not None else None, _stream(self.device)),
                           "adn_stream_pool_push_rate")

    def push_many(self, blocks) -> None:
        """``{sid: block}``: the next samples of several streams, each at its stream's rate.  The blocks of the streams at a rate of
        their own are staged with one host-to-device copy when all of them are numpy (device tensors: one concatenation; mixed: a
        copy per numpy block) and resampled into their rings by one ``adn_stream_pool_push_rate`` call per 64 of them (a pool
        with ``input_rates`` takes its working-rate streams along as copy rows; without, they go the way of ``push``).  When one
        block does not fit its stream's ``room``, ``RuntimeError`` is raised and NO stream has changed; the same holds when
        the library refuses the call."""
        book = self.book
        items = []
        for sid, block in blocks.items():
            book._live(sid, "push")
            x, as_numpy = self._block(block)
            (book.check if book.rate[sid] is None else book.check_rate)(sid, x.shape[-1])
            items.append((sid, x, as_numpy))
        rows, parts, offset, undo, C = [], [], 0, [], self.channels
        for sid, x, as_numpy in items:
            m = x.shape[-1]
            if book.rate[sid] is None and self._rate_state is None:
                self.push(sid, x if not as_numpy else x.numpy())
                continue
            if m == 0:
                self._numpy[sid] = as_numpy
                continue
            undo.append((sid, book.received[sid], book.received_in[sid], book.calls_in[sid], self._numpy[sid]))
            self._numpy[sid] = as_numpy
            if book.rate[sid] is None:                       # at the working rate among others: a copy row of the same call
                before = book.take(sid, m)
                rate, call = book.sample_rate, min(before, 1)
            else:
                call, before = book.take_rate(sid, m)
                rate = book.rate[sid]
            for c in range(C):                               # a row per channel: slot sid C + c, its samples c m further on
                rows.append((sid * C + c, rate, call, before, m, 0, offset + c * m))
            parts.append((x.reshape(-1), as_numpy))
            offset += C * m
        if not rows:
            return
        host = [x for x, as_numpy in parts if as_numpy]
        if len(host) == len(parts):                          # all numpy: one staging buffer, one copy
            audio = (torch.cat(host) if len(host) > 1 else host[0]).to(self.device)
        else:
            audio = torch.cat([x.to(self.device) for x, _ in parts]) if len(parts) > 1 else parts[0][0].to(self.device).contiguous()
        try:
            self._push_rate(rows, audio)
        except Exception:                                    # refused by the library: the book does not run ahead of the device
            for sid, received, received_in, calls_in, as_numpy in undo:
                book.received[sid], book.received_in[sid], book.calls_in[sid], self._numpy[sid] = received, received_in, calls_in, as_numpy
            raise

    def close(self, sid: int) -> bool:
        """The stream has ended; its remaining steps run in the following ticks, the last of which reports ``finished=True``.
        Returns True when there is nothing left to run -- a stream of no samples -- and the slot is free already.  For a stream at
        a rate of its own the resampler in's last call goes into the ring here (``room`` has kept its samples free)."""
        book = self.book
        book._live(sid, "close")
        if book.rate[sid] is not None and book.status[sid] == book.RUNNING and book.received_in[sid] > 0:
            call, before = book.close_rate(sid)
            self._push_rate([(slot, book.rate[sid], call, before, 0, 1, 0) for slot in self._slots(sid)], None)
        return book.close(sid)

    # ------------------------------------------------------------------ building blocks (device tensors)
    def _slots(self, sid: int):
        """The device slots of stream ``sid``: itself, or the ``channels`` slots of a recording in channel order."""
        return range(sid * self.channels, (sid + 1) * self.channels)

    def _rows(self, rows):
        return (_lib.StreamPoolRow * len(rows))(*[_lib.StreamPoolRow(*r) for r in rows])

    def _emit_rows(self, rows):
        """The stream rows of a tick that ``emit`` takes back to audio, ``_net``'s result holding one window for each: all of them
        here; a class whose operator leaves a recording's result in its first row keeps that one (``BeamformStreamPool``), and one
        whose recordings carry rows that are only read keeps the others (``EchoStreamPool``: the microphones, not the far end).
        Any rows of each recording may be kept, the same channels of every one, in channel order: ``step`` reads the channels off
        the first recording's kept rows."""
        return rows

    def analyze(self, rows) -> torch.Tensor:
        """``adn_stream_pool_analyze``: rows ``(slot, step, final_length)``, at most 256 -> network input ``(n_rows, 1, F, W)``."""
        out = torch.empty((len(rows), 1, self.n_bins, self.book.window_frames), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_stream_pool_analyze(self._state.data_ptr(), self._state.numel(), *self._args, self._rows(rows),
                                                           len(rows), out.data_ptr(), _stream(self.device)), "adn_stream_pool_analyze")
        return out

    def network(self, x: torch.Tensor) -> torch.Tensor:
        return unet_windows("StreamPool", self.model, x, self.batch_windows)

    def _net(self, x: torch.Tensor, rows) -> torch.Tensor:
        """What stands between ``analyze`` and ``emit`` for a tick's ``rows`` (``(slot, step, final_length)``, window i from row i):
        here the network, which needs none of them."""
        return self.network(x)

    def emit(self, y: torch.Tensor, rows) -> torch.Tensor:
        """``adn_stream_pool_emit``: the network's output for the windows of ``analyze`` -> ``(n_rows, B hop + n_fft / 2)``, row i
        holding ``book.count(step, final_length)`` samples."""
        y = y.contiguous()
        out = torch.empty((len(rows), self.book.out_stride), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().adn_stream_pool_emit(self._state.data_ptr(), self._state.numel(), *self._args, self._rows(rows),
                                                        len(rows), y.data_ptr(), out.data_ptr(), self.book.out_stride,
                                                        _stream(self.device)), "adn_stream_pool_emit")
        return out

    # ------------------------------------------------------------------ ticks
    def step(self):
        """ONE step of every stream that has one ready -> a list of ``(sid, samples, finished)`` in ascending ``sid``; ``samples``
        are the stream's newly final ones (possibly none, while ``B hop < n_fft / 2`` in a stream's first steps)."""
        rows = self.book.rows()
        if not rows:
            return []
        book, C = self.book, self.channels
        # the device's rows: a stream's own, or the C of a recording in channel order, 256 // C recordings a call
        srows = rows if C == 1 else book.stream_rows(rows)
        group = POOL_MAX_ROWS // C * C
        groups = [srows[i:i + group] for i in range(0, len(srows), group)]
        x = torch.cat([self.analyze(g) for g in groups]) if len(groups) > 1 else self.analyze(srows)
        y = self._net(x, srows)
        erows = self._emit_rows(srows)
        E = len(erows) // len(rows)                      # rows of `out` per row of the tick: 1, or a recording's channels
        groups = [erows[i:i + POOL_MAX_ROWS] for i in range(0, len(erows), POOL_MAX_ROWS)]
        outs = [self.emit(y[i * POOL_MAX_ROWS:i * POOL_MAX_ROWS + len(g)], g) for i, g in enumerate(groups)]
        out = torch.cat(outs) if len(outs) > 1 else outs[0]
        calls, rated = book.rate_calls(rows)             # the rows of streams at a rate of their own go back to it
        if C > 1:                                        # a call per emitted channel: slot sid C + its channel, row i E + e of `out`
            kept = [r[0] - rows[0][0] * C for r in erows[:E]]            # the channels `_emit_rows` keeps of a recording
            calls = [(i * E + e, (c[0] * C + kept[e],) + c[1:]) for i, c in calls for e in range(E)]
            rated = {i: (None if j is None else j * E, n) for i, (j, n) in rated.items()}
        rout = self.emit_rate(out, calls) if calls else None
        plain = any(self._numpy[r[0]] and i not in rated for i, r in enumerate(rows))
        host = out.cpu().numpy() if plain else None
        rhost = rout.cpu().numpy() if rout is not None and any(self._numpy[rows[i // E][0]] for i, _ in calls) else None
        if C == 1 or E == 1:
            def pick(a, i, n):
                return a[i, :n]
        else:                                            # a recording that keeps its channels: (C, n)
            def pick(a, i, n):
                return a[i:i + E, :n]
        result = []
        for i, (slot, k, final) in enumerate(rows):
            if i in rated:
                j, n = rated[i]
                if j is None:
                    samples = np.empty(0, dtype=np.float32) if self._numpy[slot] else out.new_empty(0)
                    if C > 1 and E > 1:
                        samples = samples.reshape(E, 0)
                else:
                    samples = pick(rhost, j, n).copy() if self._numpy[slot] else pick(rout, j, n).clone()
            else:
                n = book.count(k, final)
                samples = pick(host, i * E, n).copy() if self._numpy[slot] else pick(out, i * E, n).clone()
            result.append((slot, samples, book.ran(slot)))
        return result

    def emit_rate(self, out: torch.Tensor, calls) -> torch.Tensor:
        """``adn_stream_pool_emit_rate``: ``calls`` as ``PoolBook.rate_calls`` returns them, ``out`` what ``emit`` wrote for the
        tick; -> ``(len(calls), book.rate_out_stride)``, row j holding call j's samples at its stream's rate.  One call per 64
        of them, whichever rows of ``out`` they are: a row names the rows left out before it in its ``audio_offset``."""
        stride, in_stride = self.book.rate_out_stride, out.stride(0)
        rout = torch.empty((len(calls), stride), dtype=torch.float32, device=self.device)
        L = _lib.load()
        with torch.cuda.device(self.device):
            for j in range(0, len(calls), POOL_RATE_MAX_ROWS):
                g = [c[:6] + ((row - i) * in_stride,) for i, (row, c) in enumerate(calls[j:j + POOL_RATE_MAX_ROWS])]
                _lib.check(L.adn_stream_pool_emit_rate(*self._rate_args, self._rate_rows(g), len(g), out.data_ptr(), in_stride,
                                                       rout[j].data_ptr(), stride, _stream(self.device)), "adn_stream_pool_emit_rate")
        return rout

    def drain(self):
        """``step()`` until nothing is ready -> ``(sid, samples, finished)`` per stream that ran, its samples concatenated."""
        order, parts, fin = [], {}, {}
        while True:
            tick = self.step()
            if not tick:
                break
            for sid, samples, finished in tick:
                if sid not in parts:
                    order.append(sid)
                    parts[sid] = []
                parts[sid].append(samples)
                fin[sid] = finished
        return [(sid, np.concatenate(parts[sid], axis=-1) if isinstance(parts[sid][0], np.ndarray) else torch.cat(parts[sid], dim=-1), fin[sid])
                for sid in sorted(order)]


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
    def make(dev, n_streams, input_rate):
        return StreamDenoiser(_load_model(args.model, args.dtype, dev), n_streams=n_streams, window_frames=args.window,
                              block_frames=args.block, lookahead_frames=args.lookahead, input_rate=input_rate)
    if args.live:
        return run_live(make, args.src, args.dst, args.chunk, None)
    dev = _lib.staging_device()
    audio, rate = read_wav(args.src, mono=False)             # (L, channels): every channel is a stream
    x = torch.from_numpy(np.ascontiguousarray(audio.T, dtype=np.float32)).to(dev)
    sd = make(dev, x.shape[0], None)
    length = x.shape[1]
    if rate != sd.input_rate:                                # the file is converted as a whole, before and after
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
    print(f"{args.src} -> {args.dst}: {length} samples at {rate} Hz in pushes of {args.chunk}, latency {sd.latency_samples} samples")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
