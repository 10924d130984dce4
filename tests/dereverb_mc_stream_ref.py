"""numpy restatement of the streaming multichannel dereverberator of include/adn.h ("dereverb stream multichannel") -- TEST
INFRASTRUCTURE, written from the header text.  float64 is the reference; dtype=np.float32 carries every statement out in float32
(every sum term by term in the header's order), which is how the float32 host floors FLOOR and FLOOR_AUDIO below were measured
(python tests/dereverb_mc_stream_cases.py); arithmetic="fma" is the other float32 form, the header's fmaf pairing and order, as in
tests/dereverb_stream_ref.py.  Vectorised over bins; a group's spectrograms are (C, T, F), frame-major like the
device's; the end-to-end form is built on tests/dereverb_stream_ref.py's transforms and on tests/baseline_ref.py's gain.  With
C = 1 every float64 statement is evaluated by the very expression tests/dereverb_stream_ref.py uses, so the two agree exactly."""
import numpy as np

import baseline_ref
import denoise_ref
import dereverb_stream_ref as ds

FIELDS = ds.FIELDS

# The float32 host floors: the worst max|d32 - d64| / max|d64| per group over the GPU parity cases of
# tests/dereverb_mc_stream_cases.py (FLOOR: the spectrum d of wpe_mc_online; FLOOR_AUDIO: the audio of the end-to-end stream form),
# measured on the host from this restatement (never from the device) and written here by `python tests/dereverb_mc_stream_cases.py`.
FLOOR = 3.7e-06
FLOOR_AUDIO = 2.0e-06


def defaults(channels):
    """The parent's defaults with taps = 32 / C."""
    return dict(ds.DEFAULTS, taps=32 // channels)


def lowest_forget(n):
    """The lowest fp32 forget the rule 2 N (1 - forget) <= 1 admits at stacked size N (in double on the fp32 value)."""
    f = np.float32(1.0 - 1.0 / (2.0 * n))
    while not 2.0 * n * (1.0 - float(f)) <= 1.0:
        f = np.nextafter(f, np.float32(2.0))
    return float(f)


def check_params(p, channels):
    """The legal ranges of the header; ValueError (naming the field) outside them."""
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= 8:
        raise ValueError("channels")
    ds.check_params(p)
    n = channels * int(p["taps"])
    if n > 32:
        raise ValueError("channels * taps")
    if channels >= 2 and not 2.0 * n * (1.0 - float(np.float32(p["forget"]))) <= 1.0:
        raise ValueError("forget")


def wpe_mc_online(specs, params=None, dtype=np.float64, state=None, first_frame=0, with_state=False, with_lam=False,
                  arithmetic="plain"):
    """specs (C, T, F) complex, the frames first_frame ... first_frame + T - 1 of the C channels of ONE group -> d (C, T, F) complex
    in `dtype`'s precision.  `state` is what an earlier call returned (with_state=True); first_frame = 0 starts fresh whatever it
    holds.  with_state: also the state after the last frame, a dict G (F, C, N) (G[:, c, r] = G_rc), P (F, N, N), s (F,), past
    (F, C, D + K - 1) = the last raw frames of every channel, oldest first.  with_lam: also lam (T, F).
    arithmetic (float32 only): "plain" or "fma", as in dereverb_stream_ref.wpe_online: "fma" is the header's pairing and order of
    every complex multiply-add and its componentwise divisions; "plain" is what FLOOR was measured with."""
    X = np.asarray(specs)
    C, T, F = X.shape
    p = defaults(C)
    p.update(params or {})
    check_params(p, C)
    dt = np.dtype(dtype).type
    assert arithmetic in ds.ARITHMETICS and (arithmetic == "plain" or dt is np.float32)
    fused = arithmetic == "fma"
    ct = np.complex64 if dt is np.float32 else np.complex128
    K, D = int(p["taps"]), int(p["delay"])
    N = C * K
    alpha, delta, rho, beta = (dt(np.float32(p[name])) for name in ("forget", "loading", "power_floor", "smooth"))
    # the two derived constants are computed once, in fp32, as the header says
    one_minus_beta = dt(np.float32(1.0) - np.float32(p["smooth"]))
    p0 = dt(np.float32(1.0) / np.float32(p["loading"]))
    tiny, fC = dt(1e-30), dt(C)
    X = X.astype(ct)
    H = D + K - 1
    if first_frame == 0:
        G = np.zeros((F, C, N), ct)
        P = np.zeros((F, N, N), ct)
        P[:, np.arange(N), np.arange(N)] = p0
        s = np.zeros(F, dt)
        past = np.zeros((F, C, H), ct)
    else:
        G, P, s, past = (np.array(state[name]) for name in ("G", "P", "s", "past"))
        assert G.dtype == ct and past.shape == (F, C, H)
    full = np.concatenate([past, np.transpose(X, (2, 0, 1))], axis=2)      # (F, C, H + T): frame t of the call at column H + t
    d = np.empty((C, T, F), ct)
    lams = np.empty((T, F), dt)
    low = np.tril(np.ones((N, N), bool))
    idx = np.arange(N)
    with np.errstate(all="ignore"):
        for t in range(T):
            x = full[:, :, H + t]                                          # (F, C)
            # x~[r] = X_{t-D-j, c} at r = c K + j: channel-major, the lag ascending inside a channel
            xt = full[:, :, H + t - D - K + 1:H + t - D + 1][:, :, ::-1].reshape(F, N)
            pw = np.zeros(F, dt)
            for c in range(C):                                             # c ascending, then one division
                pw = (pw + ds._power(x[:, c], dt)).astype(dt)
            pw = (pw / fC).astype(dt)
            s = pw if first_frame + t == 0 else (beta * s + one_minus_beta * pw).astype(dt)
            phi = ds._max(rho * s, tiny)
            e = np.empty((F, C), ct)
            if fused:                                                      # term by term, in the header's order and pairing
                pred = np.zeros((F, C), ct)
                for r in range(N):
                    pred = ds.cfma_conj(xt[:, r, None], G[:, :, r], pred)
                e[:] = ds.cx(x.real - pred.real, x.imag - pred.imag)
                u = np.zeros((F, N), ct)
                for k in range(N):
                    u = ds.cfma(P[:, :, k], xt[:, k, None], u)
                q = np.zeros(F, dt)
                for r in range(N):
                    q = ds.fma(xt[:, r].imag, u[:, r].imag, ds.fma(xt[:, r].real, u[:, r].real, q))
            elif dt is np.float32:                                         # term by term, in the header's order
                pred = np.zeros((F, C), ct)                                # every channel's sum in r order, the channels side by side
                for r in range(N):
                    pred = pred + np.conj(G[:, :, r]) * xt[:, r, None]
                e[:] = x - pred
                u = np.zeros((F, N), ct)
                for k in range(N):
                    u = u + P[:, :, k] * xt[:, k, None]
                q = np.zeros(F, dt)
                for r in range(N):
                    q = q + (np.conj(xt[:, r]) * u[:, r]).real
            else:
                for c in range(C):
                    e[:, c] = x[:, c] - np.einsum("fj,fj->f", np.conj(G[:, c]), xt)
                u = np.einsum("fjk,fk->fj", P, xt)
                q = np.einsum("fj,fj->f", np.conj(xt), u).real
            ee = np.zeros(F, dt)
            for c in range(C):
                ee = (ee + ds._power(e[:, c], dt)).astype(dt)
            lam = ds._max((ee / fC).astype(dt), phi)
            den = (alpha * lam + q).astype(dt)
            if fused:
                kk = ds.cx(u.real / den[:, None], u.imag / den[:, None])
                Pn = ds.cfma_conj(-kk[:, :, None], u[:, None, :], P)
                Pn = ds.cx(Pn.real / alpha, Pn.imag / alpha)
            else:
                kk = (u / den[:, None]).astype(ct)
                Pn = ((P - kk[:, :, None] * np.conj(u)[:, None, :]) / alpha).astype(ct)
            Pn = np.where(low, Pn, np.conj(np.swapaxes(Pn, 1, 2)))          # the upper triangle is the lower one's conjugate
            Pn[:, idx, idx] = Pn[:, idx, idx].real
            P = Pn
            Gn = np.empty_like(G)
            for c in range(C):
                Gn[:, c] = ds.cfma_conj(kk, e[:, c, None], G[:, c]) if fused else (G[:, c] + kk * np.conj(e[:, c])[:, None]).astype(ct)
            G = Gn
            d[:, t] = e.T
            lams[t] = lam
    out = [d]
    if with_state:
        out.append(dict(G=G, P=P, s=np.asarray(s, dt), past=np.ascontiguousarray(full[:, :, T:])))
    if with_lam:
        out.append(lams)
    return out[0] if len(out) == 1 else tuple(out)


def _resynth(d, hop, length, gain, gain_params, dtype):
    """One channel's d (T, F) -> audio: M = |d| (with gain=True the spectral gain on it), M with the phase of d, the inverse STFT:
    the tail of dereverb_stream_ref.stream_dereverb, statement for statement."""
    f32 = np.dtype(dtype) == np.float32
    mag = ds.magnitude(d, dtype)
    if gain:
        mag, _ = baseline_ref.spectral_gain(mag.T.astype(d.dtype), gain_params, dtype=dtype)
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(mag), mag, np.maximum(mag, 0)).astype(dtype)       # adn_stream_emit clamps what it reads
        if not f32:
            return denoise_ref.istft(denoise_ref.rephase(m, d), hop, length)
        size = ds.magnitude(d, dtype).T
        scale = (m.T / np.where(size > 0, size, np.float32(1.0))).astype(np.float32)
        s = np.where(size > 0, (d * scale).astype(np.complex64), (m.T + 0j).astype(np.complex64))
        return ds.istft32(s, hop, length)


def stream_dereverb_mc(x, n_fft=512, hop=128, params=None, gain=False, gain_params=None, dtype=np.float64):
    """End to end, what StreamDereverberator(channels=C) returns for the finished recording x (C, L): the STFT of every channel,
    the joint recursion, then per channel M = |d| (with gain=True the spectral gain on it), M with the phase of d and the inverse
    STFT of the input's length.  dtype=np.float32 carries EVERY statement out in float32, the two transforms included."""
    f32 = np.dtype(dtype) == np.float32
    x = np.asarray(x)
    specs = np.stack([ds.stft32(row, n_fft, hop) if f32 else denoise_ref.stft(row, n_fft, hop) for row in x])
    d = wpe_mc_online(specs, params, dtype=dtype)
    return np.stack([_resynth(d[c], hop, x.shape[1], gain, gain_params, dtype) for c in range(x.shape[0])])


si_sdr = baseline_ref.si_sdr
