"""SHA-256 digests of the spectral entry points (STFT, fitted STFT, complex STFT, inverse STFT, Griffin-Lim, the denoiser's
windows / stitch / resynth, StreamDenoiser, StreamPool) at every n_fft the library supports: one line per call.

A change that must not move a bit of their output (a refactoring of csrc/{stft,gl,denoise,stream}_kernels.hip or spectral.h) is
checked by running this script against both libraries on the same machine and comparing the two outputs as text:

    python -m audiodenoiser_amd.build --variant parent        # in a worktree of the other commit; copy the .so over
    ADN_LIBADN_PATH=.../libadn_parent.so python tools/spectral_digest.py > before.txt
    python tools/spectral_digest.py > after.txt ; diff before.txt after.txt

Fixed seeds.  The network is replaced by a fixed elementwise map of its input (a random gain and offset, negative values
included so that the clamp works): the digests then depend on the spectral kernels alone.  Shapes are small -- 3 clips of
4 n_fft + 37 and 2 hop - 1 samples (both odd), windows of 32 frames overlapping by 16, the stream plan W = 32, B = 8, A = 4 --
with three additions: clips of 20 n_fft + 37 samples where the denoiser needs more frames than one window to cross-fade at
all; the fitted STFT of those clips into 96 frames, three 32-frame groups per clip, so that the persistent kernel steps from
group to group inside a clip; and, for the fitted STFT at n_fft 512 and 1024, 2100 one-group clips.  The persistent kernel
launches min(items, workgroups the card holds) workgroups; the library does not report that grid, so the line gives the items
and the CUs, and `more_items_than_8_per_cu` says whether the items exceed even 8 workgroups on every CU (the kernel's
registers allow 3): then some workgroup must walk from one clip into the next.  Not covered here: fitted windows wider than
96 frames and the reference's 513 x 256 at scale -- tests/test_gpu_parity.py has those.  A digest only says that a value has
not moved: whether resynth and the stream kernels are RIGHT at n_fft 2048 and 4096, and at every other size, is checked against
float64 by tests/test_gpu_spectral_grid.py.

At n_fft 64 and 512 the classes with an operator in the network's place follow (`operators`): SpectralDenoiser, Dereverberator,
their lockstep stream forms at the working rate and at 48 kHz, and their pools with streams at 8, 48 and 16 kHz driven through
push_many / step / close -- block_frames 8, pushes of 1, 3, 8, 2 hops in turn.  Those lines use public names only, so the script
also compares two versions of the PYTHON layer over one library: import the other commit's package first and run this file in
that process (`runpy.run_path`; a package already imported wins over the path added below), ADN_LIBADN_PATH naming the one
built library.

Last comes the WPE family on random complex spectrograms (`wpe_family`; no STFT in front): 33 bins -- no multiple of the 4, 8 or 16
bins of a workgroup -- and 3 clips or groups.  Offline: taps 4, 20, 24, 32 (the 16-, 16-, 32- and 64-lane kernels) and the joint
form at (channels, taps) = (2, 8), (2, 5), (3, 7), (4, 8), (8, 4), (8, 1), (1, 5) (both block layouts, every lane count, the lane
doubling at 8 channels, the forward to the single-channel kernel), each at 70 frames (two staged chunks, 70 % 4 != 0) and at 3
(fewer than delay + taps).  Online: taps 1, 20, 32 and the joint form at (2, 16), (3, 7), (8, 4), (8, 1), (1, 20), two calls of 5
then 9 frames with the state carried; d, the magnitudes and the state bytes are hashed.  `python tools/spectral_digest.py --wpe`
prints the `operators` lines and that section alone."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from audiodenoiser_amd.denoise import Denoiser  # noqa: E402
from audiodenoiser_amd.griffin_lim import griffin_lim_reconstruction, istft, stft_complex  # noqa: E402
from audiodenoiser_amd.model import UNet  # noqa: E402
from audiodenoiser_amd.stft import stft_magnitude, stft_magnitude_fit  # noqa: E402
from audiodenoiser_amd.stream import StreamDenoiser, StreamPool  # noqa: E402

N_FFTS = (64, 128, 256, 512, 1024, 2048, 4096)
DEV = torch.device("cuda", 0)
W, V, B, A = 32, 16, 8, 4
_GAIN = {}


def rand(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def audio(seed, n, length):
    return (rand(seed, n, length) * 2 - 1).to(DEV)


def say(what, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        t = torch.view_as_real(t) if t.is_complex() else t
        h.update(str(tuple(t.shape)).encode())
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    print(f"{what} {h.hexdigest()}", flush=True)


def fake_network(x):
    """In place of the U-Net: y = x * gain + offset with a fixed random gain in [-0.25, 1.25) and offset in [-0.1, 0.1)."""
    key = tuple(x.shape)
    if key not in _GAIN:
        _GAIN[key] = (rand(11, *key).to(x.device) * 1.5 - 0.25, rand(12, *key).to(x.device) * 0.2 - 0.1)
    g, o = _GAIN[key]
    return x * g + o


def transforms(n_fft):
    hop = n_fft // 4
    for length in (4 * n_fft + 37, 2 * hop - 1):
        a = audio(length, 3, length)
        tag = f"n_fft={n_fft} hop={hop} L={length}"
        for center in (True, False):
            if not center and length < n_fft:
                continue
            say(f"stft {tag} center={int(center)}", stft_magnitude(a, n_fft, hop, center))
            for h, w in ((n_fft // 2 + 1, W), (n_fft // 2 - 3, 12)):
                say(f"stft_fit {tag} center={int(center)} {h}x{w}", stft_magnitude_fit(a, (h, w), n_fft, hop, center))
        spec = stft_complex(a, n_fft, hop)
        say(f"stft_complex {tag}", spec)
        say(f"istft {tag}", istft(spec, hop))
        say(f"griffin_lim {tag} iterations=10",
            griffin_lim_reconstruction(spec.abs().transpose(1, 2).contiguous(), n_fft, hop, 10, rand=rand(5, *spec.shape)))
    if n_fft >= 256:                               # the sizes stft_fit_kernel serves (and, above 1024, stft_mag_kernel's fitted form)
        length = 20 * n_fft + 37
        a = audio(length, 3, length)
        for center in (True, False):
            say(f"stft_fit n_fft={n_fft} hop={hop} L={length} center={int(center)} {n_fft // 2 + 1}x96 groups_per_clip=3",
                stft_magnitude_fit(a, (n_fft // 2 + 1, 96), n_fft, hop, center))
    if n_fft in (512, 1024):
        n, length = 2100, 4 * n_fft + 37
        a = audio(77, n, length)
        cus = torch.cuda.get_device_properties(DEV).multi_processor_count
        for center in (True, False):
            say(f"stft_fit n_fft={n_fft} hop={hop} L={length} center={int(center)} 65x{W} items={n} cus={cus} more_items_than_8_per_cu={int(n > 8 * cus)}",
                stft_magnitude_fit(a, (65, W), n_fft, hop, center))


def denoiser(model, n_fft):
    hop = n_fft // 4
    dn = Denoiser(model, n_fft=n_fft, hop_length=hop, window_frames=W, overlap_frames=V)
    for length in (4 * n_fft + 37, 2 * hop - 1, 20 * n_fft + 37):
        a = audio(1000 + length, 3, length)
        spec = stft_complex(a, n_fft, hop)
        x = dn.windows(spec)
        y = fake_network(x)
        tag = f"n_fft={n_fft} hop={hop} L={length} W={W} V={V}"
        say(f"denoise.windows {tag}", x)
        for clamp in (False, True):
            say(f"denoise.stitch {tag} clamp={int(clamp)}", dn.stitch(y, 3, spec.shape[1], clamp))
        say(f"denoise.resynth {tag}", dn.resynth(y, spec, length))


def stream(model, n_fft):
    hop = n_fft // 4
    length = 20 * n_fft + 37
    a = audio(2000 + n_fft, 3, length)
    sd = StreamDenoiser(model, n_streams=3, n_fft=n_fft, hop_length=hop, window_frames=W, block_frames=B, lookahead_frames=A,
                        batch_windows=9)
    sd.network = fake_network
    outs, pos = [], 0
    for m in (1, n_fft // 2 + 3, 7 * n_fft + 1, 0, 5 * hop, length):          # uneven pushes; the last takes the rest
        outs.append(sd.push(a[:, pos:pos + m]))
        pos = min(pos + m, length)
    outs.append(sd.flush())
    say(f"stream n_fft={n_fft} hop={hop} L={length} W={W} B={B} A={A} streams=3", torch.cat(outs, dim=1))

    pool = StreamPool(model, max_streams=3, n_fft=n_fft, hop_length=hop, window_frames=W, block_frames=B, lookahead_frames=A)
    pool.network = fake_network
    lengths = (length, 9 * n_fft + 2, 2 * hop - 1)                            # slot 2 opens late and ends first
    got = {s: [] for s in range(3)}
    sent = [0, 0, 0]
    open_at = (0, 0, 3)
    sids = {}
    for tick in range(400):
        for s in range(3):
            if tick == open_at[s]:
                sids[s] = pool.open()
            if s in sids and sent[s] < lengths[s]:
                m = min((s + 1) * hop + 5 * (tick % 3), lengths[s] - sent[s], pool.room(sids[s]))
                pool.push(sids[s], a[s, sent[s]:sent[s] + m])
                sent[s] += m
                if sent[s] == lengths[s]:
                    pool.close(sids[s])
        ran = pool.step()
        for sid, samples, _ in ran:
            got[sid].append(samples)
        if not ran and all(sent[s] == lengths[s] for s in range(3)):
            break
    outs = [torch.cat(got[sids[s]]) if got[sids[s]] else torch.empty(0, device=DEV) for s in range(3)]
    assert [o.shape[0] for o in outs] == list(lengths), ([o.shape[0] for o in outs], lengths)
    say(f"stream_pool n_fft={n_fft} hop={hop} lengths={lengths} W={W} B={B} A={A} slots=3", *outs)


def pieces(total, unit):
    """Cuts of ``total`` samples into pushes of 1, 3, 8, 2, 1, 3, ... ``unit``s; the last takes what is left."""
    pos, k = 0, 0
    while pos < total:
        m = min((1, 3, 8, 2)[k % 4] * unit, total - pos)
        yield pos, m
        pos, k = pos + m, k + 1


def lockstep(cls, tag, a, hop, rate, **kw):
    """A lockstep stream class without a network: every channel of ``a`` a stream, fed at ``rate`` (None: the working rate)."""
    sd = cls(DEV, n_streams=a.shape[0], n_fft=4 * hop, hop_length=hop, block_frames=B, input_rate=rate, **kw)
    outs = [sd.push(a[:, pos:pos + m]) for pos, m in pieces(a.shape[1], hop * (rate or 8000) // 8000)]
    outs.append(sd.flush())
    out = torch.cat(outs, dim=1)
    assert out.shape == a.shape, (out.shape, a.shape)
    say(f"{tag} streams={a.shape[0]} L={a.shape[1]} B={B} input_rate={rate}", out)


def pooled(cls, tag, feeds, hop, **kw):
    """A pool class without a network: ``feeds`` = ``(rate, samples)`` per stream, all opened at once, each pushed in its own
    pieces through ``push_many`` as far as its room allows, closed when it has sent everything; one ``step`` per round."""
    rates = [r for r, _ in feeds]
    pool = cls(DEV, max_streams=len(feeds), n_fft=4 * hop, hop_length=hop, block_frames=B, input_rates=rates, **kw)
    sids = [pool.open(input_rate=r) for r in rates]
    cuts = [pieces(x.shape[0], hop * r // 8000) for r, x in feeds]
    sent, got, waiting = [0] * len(feeds), {s: [] for s in sids}, {}
    for _ in range(1000):
        blocks = {}
        for i, (r, x) in enumerate(feeds):
            if i not in waiting and sent[i] < x.shape[0]:
                waiting[i] = next(cuts[i])[1]
            if i in waiting and waiting[i] <= pool.room(sids[i]):
                blocks[sids[i]] = x[sent[i]:sent[i] + waiting[i]]
                sent[i] += waiting.pop(i)
        pool.push_many(blocks)
        for i, (r, x) in enumerate(feeds):
            if sids[i] in blocks and sent[i] == x.shape[0]:
                pool.close(sids[i])
        ran = pool.step()
        for sid, samples, _ in ran:
            got[sid].append(samples)
        if not ran and not blocks:
            break
    outs = [torch.cat(got[s]) if got[s] else torch.empty(0, device=DEV) for s in sids]
    assert [o.shape[0] for o in outs] == [x.shape[0] for _, x in feeds], [o.shape[0] for o in outs]
    say(f"{tag} rates={tuple(rates)} lengths={tuple(x.shape[0] for _, x in feeds)} B={B}", *outs)


def operators(n_fft):
    """The classes with an operator in the network's place, through their public surface alone: offline, lockstep at the working
    rate and at 48 kHz, pooled with streams at 8, 48 and 16 kHz.  3 channels of 4 n_fft + 37 samples at the working rate; a feed
    at another rate is that many times longer, so that it brings as many steps."""
    from audiodenoiser_amd.baseline import SpectralDenoiser, SpectralStreamPool, StreamSpectralDenoiser
    from audiodenoiser_amd.dereverb import DereverbStreamPool, Dereverberator, StreamDereverberator
    hop, length = n_fft // 4, 4 * n_fft + 37
    tag = f"n_fft={n_fft} hop={hop}"
    a = audio(3000 + n_fft, 3, 6 * length)
    say(f"SpectralDenoiser {tag} L={length}", SpectralDenoiser(DEV, n_fft=n_fft, hop_length=hop).denoise(a[:, :length]))
    for rate in (None, 48000):
        lockstep(StreamSpectralDenoiser, f"StreamSpectralDenoiser {tag}", a[:, :length * (rate or 8000) // 8000], hop, rate)
    feeds = [(r, a[i, :length * r // 8000].contiguous()) for i, r in enumerate((8000, 48000, 16000))]
    pooled(SpectralStreamPool, f"SpectralStreamPool {tag}", feeds, hop)
    for gain in (False, True):
        say(f"Dereverberator {tag} L={length} gain={int(gain)}",
            Dereverberator(DEV, n_fft=n_fft, hop_length=hop, gain=gain).denoise(a[:, :length]))
        for rate in (None, 48000):
            lockstep(StreamDereverberator, f"StreamDereverberator {tag} gain={int(gain)}", a[:, :length * (rate or 8000) // 8000], hop,
                     rate, gain=gain)
        pooled(DereverbStreamPool, f"DereverbStreamPool {tag} gain={int(gain)}", feeds, hop, gain=gain)
    # the three channels as ONE recording: the joint forms
    say(f"Dereverberator joint {tag} L={length}",
        Dereverberator(DEV, n_fft=n_fft, hop_length=hop, channels="joint").denoise(a[:, :length]))
    for gain in (False, True):
        for rate in (None, 48000):
            lockstep(StreamDereverberator, f"StreamDereverberator channels=3 {tag} gain={int(gain)}",
                     a[:, :length * (rate or 8000) // 8000], hop, rate, gain=gain, channels=3)


def wpe_family():
    """The four WPE operators on random complex spectrograms: see the module text."""
    from audiodenoiser_amd.dereverb import WpeParams, WpeStreamParams, wpe, wpe_joint, wpe_online, wpe_online_joint
    f, n = 33, 3

    def spec(seed, rows, t):
        return torch.view_as_complex((rand(seed, rows, t, f, 2) * 2 - 1).to(DEV))

    for t in (70, 3):
        for taps in (4, 20, 24, 32):
            say(f"wpe F={f} clips={n} T={t} taps={taps}", *wpe(spec(4000 + t, n, t), WpeParams(taps=taps)))
        for c, k in ((2, 8), (2, 5), (3, 7), (4, 8), (8, 4), (8, 1), (1, 5)):
            say(f"wpe_joint F={f} groups={n} T={t} channels={c} taps={k}", *wpe_joint(spec(4100 + 10 * c + t, n * c, t), c, WpeParams(taps=k)))

    def two_calls(what, run, x, p):                 # frames 0 .. 4, then 5 .. 13 on the state the first call left
        d1, m1, state = run(x[:, :5].contiguous(), None, 0, p)
        d2, m2, state = run(x[:, 5:].contiguous(), state, 5, p)
        say(what, d1, m1, d2, m2, state)

    for taps in (1, 20, 32):
        two_calls(f"wpe_online F={f} rows={n} T=5+9 taps={taps}", wpe_online, spec(4200 + taps, n, 14), WpeStreamParams(taps=taps))
    for c, k in ((2, 16), (3, 7), (8, 4), (8, 1), (1, 20)):
        two_calls(f"wpe_online_joint F={f} groups={n} T=5+9 channels={c} taps={k}",
                  lambda x, state, first, p, c=c: wpe_online_joint(x, c, state, first, p), spec(4300 + 10 * c + k, n * c, 14),
                  WpeStreamParams(taps=k))


def main():
    if "--wpe" in sys.argv[1:]:
        with torch.no_grad():
            for n_fft in (64, 512):
                operators(n_fft)
            return wpe_family()
    model = UNet(1, 1).eval().to(DEV)              # the classes ask for one; fake_network runs in its place
    with torch.no_grad():
        for n_fft in N_FFTS:
            transforms(n_fft)
            denoiser(model, n_fft)
            stream(model, n_fft)
            if n_fft in (64, 512):
                operators(n_fft)
        wpe_family()


if __name__ == "__main__":
    main()
