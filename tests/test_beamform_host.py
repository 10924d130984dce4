"""The beamformer without a device: the restatement's own properties (tests/beamform_ref.py) against an independent float64
evaluation, the gain over the single-microphone forms that the feature exists for, the Python face
(audiodenoiser_amd/beamform.py) and the argument checks of adn_mvdr / adn_mvdr_workspace_bytes, which refuse before anything is
launched.
Measured on the host (float64 restatements, the 8 dB recording of tests/beamform_cases.py, SI-SDR after the inverse STFT): spectral
gain on microphone 0 5.65 dB; MVDR at C = 4 7.77 (margin 2.1, condition 1); MVDR + gain at C = 2 8.83 (margin 3.2, condition 2).
The restatement against np.linalg.solve on the dense matrices: at most 8e-16 of the maximum (bound 1e-9)."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_ref as bf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)).astype(np.complex64)


def _mags(x, seed):
    """A magnitude estimate that keeps the mask inside the clip: uniform [0.2, 0.9) x |X|, (C, F, T)."""
    rng = np.random.default_rng(seed)
    a = np.abs(x).transpose(0, 2, 1)
    return ((0.2 + 0.7 * rng.random(a.shape)) * a).astype(np.float32)


def _dense(x, mags, ref=0, loading=1e-3, rho=1e-3):
    """The definition evaluated independently in float64: dense matrices by einsum, np.linalg.solve, no Cholesky."""
    X = x.astype(np.complex128)                                                    # (C, T, F)
    C = X.shape[0]
    M = mags.astype(np.float64).transpose(0, 2, 1)[:, :X.shape[1]]                # (C, T, F)
    q = (np.abs(X) ** 2).sum(0)
    top = float(np.float32(1.0) - np.float32(rho))
    with np.errstate(all="ignore"):
        m = np.where(q > 0, np.clip((M ** 2).sum(0) / q, float(np.float32(rho)), top), float(np.float32(rho)))
    phi_s = np.einsum("tf,rtf,ktf->frk", m, X, np.conj(X))
    phi_n = np.einsum("tf,rtf,ktf->frk", 1.0 - m, X, np.conj(X))
    eye = np.eye(C)[None]
    A = phi_n + (float(np.float32(loading)) * np.trace(phi_n, axis1=1, axis2=2).real / C + 1e-30)[:, None, None] * eye
    G = np.linalg.solve(A, phi_s)
    tau = np.maximum(np.trace(G, axis1=1, axis2=2).real, 1e-30)
    w = G[:, :, ref] / tau[:, None]
    return np.einsum("fc,ctf->tf", np.conj(w), X)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,ref,loading", ((1, 0, 1e-3), (2, 1, 1e-3), (3, 0, 1e-2), (5, 4, 1e-3), (8, 0, 1e-3), (8, 7, 1e-6)))
def test_restatement_against_an_independent_dense_evaluation(channels, ref, loading):
    x = _noise((channels, 60, 7), 10 + channels)
    mags = _mags(x, channels)
    want = _dense(x, mags, ref, loading)
    got = bf.mvdr(x, mags, dict(ref_channel=ref, loading=loading))
    assert got.shape == (60, 7) and got.dtype == np.complex128
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"C {channels} ref {ref} loading {loading:g}: {err:.3g} of the maximum (bound 1e-9)")
    assert err <= 1e-9


def test_the_gain_s_mask_and_a_wider_pitch():
    """With the mask magnitudes of the spectral gain (what mask="spectral" feeds it), and columns past T ignored."""
    specs = bc.group_specs(64, 23, 3, 1)
    mags = bc.magnitudes_of(specs, dict())
    want = _dense(specs, mags, 2)
    got = bf.mvdr(specs, mags, dict(ref_channel=2))
    assert float(np.abs(got - want).max() / np.abs(want).max()) <= 1e-9
    wide = np.concatenate([mags, np.full(mags.shape[:2] + (9,), np.nan, np.float32)], axis=2)
    assert np.array_equal(bf.mvdr(specs, wide, dict(ref_channel=2)), got)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_one_channel_zero_groups_isolation_and_the_clip(dtype):
    ct = np.complex64 if dtype is np.float32 else np.complex128
    x = _noise((1, 40, 6), 3)
    y, w = bf.mvdr(x, _mags(x, 3), dtype=dtype, with_filter=True)
    assert np.all(w == 1) and np.array_equal(y, x[0].astype(ct))                  # C = 1: w = G / G = 1
    assert np.all(bf.mvdr(np.zeros((3, 30, 4), np.complex64), np.zeros((3, 4, 30), np.float32), dtype=dtype) == 0)
    x = _noise((3, 40, 6), 4)
    mags = _mags(x, 4)
    whole = bf.mvdr(x, mags, dtype=dtype)
    assert np.array_equal(bf.mvdr(x[:, :, 2:5], mags[:, 2:5], dtype=dtype), whole[:, 2:5])     # a bin does not see its neighbours
    bad = x.copy()
    bad[1, 20, 3] = np.nan
    keep = np.arange(6) != 3
    assert np.array_equal(bf.mvdr(bad, mags, dtype=dtype)[:, keep], whole[:, keep])
    zero_bin = x.copy()
    zero_bin[:, :, 1] = 0
    assert np.all(bf.mvdr(zero_bin, mags, dtype=dtype)[:, 1] == 0)
    # the clip: a magnitude estimate of zero, or far above |X|, is the mask rho or 1 - rho, and both give a finite filter
    rho = np.float32(1e-3)
    assert np.all(bf.mask(x, np.zeros_like(mags), rho, dtype) == dtype(rho))
    assert np.all(bf.mask(x, 100 * mags, rho, dtype) == dtype(np.float32(1) - rho))
    assert np.all(bf.mask(np.zeros_like(x), mags, rho, dtype) == dtype(rho))      # q = 0
    m = bf.mask(x, 1.4 * mags, 0.25, dtype)                                       # s / q in [0.08, 1.6): both ends are reached
    assert m.min() == dtype(np.float32(0.25)) and m.max() == dtype(np.float32(0.75))
    for scale in (0.0, 100.0):
        assert np.all(np.isfinite(bf.mvdr(x, scale * mags, dtype=dtype)))


def test_a_common_scale_of_the_magnitudes_is_not_an_invariance():
    """n_t = 1 - m_t does not scale with m_t: the header says so instead of claiming the invariance."""
    x = _noise((2, 50, 4), 6)
    mags = (0.25 * _mags(x, 6)).astype(np.float32)
    a, b = bf.mvdr(x, mags), bf.mvdr(x, 2 * mags)
    assert np.abs(bf.mask(x, 2 * mags, 1e-3)).max() < 1 - 1e-3                    # both masks are inside the clip
    assert float(np.abs(a - b).max() / np.abs(a).max()) > 1e-3
    header = open(os.path.join(ROOT, "include", "adn.h")).read()
    section = header[header.index("beamform: mask-driven MVDR"):header.index("environment switches")]
    for phrase in ("UNPINNED", "not tuned by ear", "NOT a consequence", "1 <= C <= 8", "0 <= ref_channel < channels",
                   "1e-6 <= mask_floor <= 0.25", "Not here: streaming or recursive beamforming", "no atomics"):
        assert phrase in section, phrase


def test_defaults_and_legal_ranges():
    assert bf.DEFAULTS == dict(ref_channel=0, loading=1e-3, mask_floor=1e-3)
    for channels, kw in ((0, {}), (9, {}), (2, dict(ref_channel=2)), (2, dict(ref_channel=-1)), (2, dict(loading=0.0)),
                         (2, dict(loading=2.0)), (2, dict(mask_floor=0.3)), (2, dict(mask_floor=1e-7)), (2, dict(loading=float("nan")))):
        with pytest.raises(ValueError):
            bf.check_params(dict(bf.DEFAULTS, **kw), channels)
    bf.check_params(dict(bf.DEFAULTS, ref_channel=7, loading=1e-6, mask_floor=0.25), 8)


def test_float32_is_carried_out_in_float32_and_the_floors_are_recorded():
    """The floors are what `python tests/beamform_cases.py` measured; here three of its cases stay under theirs."""
    assert 0 < bf.FLOOR_FULL_RANK <= bf.FLOOR < 1e-2
    x = _noise((2, 40, 5), 9)
    y32 = bf.mvdr(x, _mags(x, 9), dtype=np.float32)
    assert y32.dtype == np.complex64 and not np.array_equal(y32, bf.mvdr(x, _mags(x, 9)).astype(np.complex64))
    for n_fft, n_frames, channels, extra in ((64, 23, 3, dict()), (64, 1, 8, dict()), bc.LOADING_CASE):
        specs = bc.group_specs(n_fft, n_frames, channels, 1)
        f = bc.floor_of(specs, bc.magnitudes_of(specs, extra), bc.params_of(extra, channels - 1))
        print(f"n_fft {n_fft} T {n_frames} C {channels} {extra}: {f:.3g} (its floor {bc.floor_for(n_frames, channels, extra):.3g})")
        assert f <= bc.floor_for(n_frames, channels, extra) * 1.05                # the floors are written with two digits
    assert sum(1 for _ in bc.parity_cases()) == 5 * 5 + 4


def test_the_beamformer_beats_the_single_microphone_forms():
    """The two conditions of the table: MVDR at C = 4 beats the spectral gain on microphone 0 by at least 1 dB, MVDR + gain at
    C = 2 by at least 2 dB."""
    alone = bc.restatement_si_sdr("spectral gain on microphone 0", 2)
    four = bc.restatement_si_sdr("MVDR, mask from the spectral gain", 4)
    two = bc.restatement_si_sdr("MVDR, then the spectral gain", 2)
    print(f"input {bc.restatement_si_sdr('microphone 0 as recorded', 2):.2f} dB, spectral gain on microphone 0 {alone:.2f}, "
          f"MVDR at C = 4 {four:.2f}, MVDR + gain at C = 2 {two:.2f}")
    noisy, dry = bc.recording(4)
    assert noisy.shape == (4, 32000) and dry.shape == (32000,)
    assert four >= alone + 1.0 and two >= alone + 2.0


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.beamform import MvdrParams
    L = _lib.load()
    buf = ctypes.create_string_buffer(32768)                 # never dereferenced: every call below is refused before a launch
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    m, q, qm = p + 8192, p + 16384, p + 24576                # spec 2 x 4 x 8 x 8 = 512 bytes, mag 2 x 8 x 4 x 4 = 256

    def call(params=None, spec=p, mag=m, mag_width=4, n=1, c=2, t=4, f=8, ws=None, ws_bytes=0, out=q, mag_out=qm, width=4):
        return L.adn_mvdr(spec, mag, mag_width, n, c, t, f, params, ws, ws_bytes, out, mag_out, width, None)

    def size(params=None, n=1, c=2, t=4, f=8, bytes_=True):
        need = ctypes.c_size_t(12345)
        return L.adn_mvdr_workspace_bytes(n, c, t, f, params, ctypes.byref(need) if bytes_ else None), need.value

    def both(word, params=None, **kw):
        assert call(params, **kw) == 1, (word, kw)
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_mvdr:") and word in msg, (kw, msg)
        rc, need = size(params, **kw)
        msg = L.adn_last_error()
        assert rc == 1 and need == 12345 and msg.startswith(b"adn_mvdr_workspace_bytes:") and word in msg, (kw, msg)

    for c in (0, 9, -1):
        both(b"channels", c=c)
    for name, value, channels in (("ref_channel", 2, 2), ("ref_channel", -1, 2), ("ref_channel", 1, 1), ("ref_channel", 8, 8),
                                  ("loading", float("nan"), 2), ("loading", 0.0, 2), ("loading", 1.5, 2),
                                  ("mask_floor", float("nan"), 2), ("mask_floor", 0.0, 2), ("mask_floor", 0.3, 2)):
        s = MvdrParams().to_struct()
        setattr(s, name, value)
        both(name.encode(), ctypes.byref(s), c=channels)
    for kw, word in ((dict(n=0), b"n_groups"), (dict(t=0), b"n_frames"), (dict(f=0), b"n_bins"), (dict(n=1 << 30, c=2), b"2^31"),
                     (dict(n=1 << 30, c=1, f=129), b"grid")):
        both(word, **kw)
    for kw, word in ((dict(spec=None), b"null"), (dict(mag=None), b"null"), (dict(out=None), b"null"), (dict(width=3), b"width"),
                     (dict(mag_width=3), b"mag_width"), (dict(spec=p + 4), b"aligned"), (dict(out=q + 4), b"aligned"),
                     (dict(mag=m + 2), b"aligned"), (dict(mag_out=qm + 2), b"aligned"), (dict(out=p), b"overlap"),
                     (dict(out=p + 512 - 8), b"overlap"), (dict(spec=q + 8, out=q), b"overlap"), (dict(out=m), b"overlap"),
                     (dict(mag_out=m), b"overlap"), (dict(mag_out=m + 256 - 4), b"overlap"), (dict(mag_out=p + 8), b"overlap"),
                     (dict(mag_out=q + 8), b"overlap")):
        assert call(**kw) == 1, kw
        msg = L.adn_last_error()
        assert msg.startswith(b"adn_mvdr:") and word in msg, (kw, msg)
    assert size(bytes_=False)[0] == 1 and b"null" in L.adn_last_error()
    # the defaults are legal for every channel count, and so is every reference channel of the parity cases
    for channels in range(1, 9):
        assert size(c=channels)[0] == 0, channels
        assert size(ctypes.byref(MvdrParams(ref_channel=channels - 1, loading=1e-6, mask_floor=0.25).to_struct()), c=channels)[0] == 0
    # a workspace below adn_mvdr_workspace_bytes: the size function may report 0 (everything on chip), and then no size is too small
    rc, need = size(n=3, c=2, t=188, f=257)
    assert rc == 0
    if need > 0:
        assert call(n=3, c=2, t=188, f=257, width=188, mag_width=188, ws=p, ws_bytes=need - 1) == 3
        assert L.adn_last_error().startswith(b"adn_mvdr:") and b"workspace" in L.adn_last_error()


# ---- the Python face ---------------------------------------------------------------------------------------------------------------
def test_mvdr_params_ranges():
    from audiodenoiser_amd import _lib
    from audiodenoiser_amd.beamform import MvdrParams
    assert dataclasses.asdict(MvdrParams()) == bf.DEFAULTS and tuple(f.name for f in dataclasses.fields(MvdrParams)) == bf.FIELDS
    assert ctypes.sizeof(_lib.MvdrParamsStruct) == 12
    for kw in (dict(ref_channel=-1), dict(ref_channel=8), dict(ref_channel=1.0), dict(ref_channel=True), dict(loading=0.0),
               dict(loading=1.5), dict(loading=float("nan")), dict(mask_floor=0.0), dict(mask_floor=0.26), dict(mask_floor=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            MvdrParams(**kw)
    MvdrParams(ref_channel=7, loading=1e-6, mask_floor=0.25)
    with pytest.raises(dataclasses.FrozenInstanceError):
        MvdrParams().loading = 0.5
    for name in ("adn_mvdr_workspace_bytes", "adn_mvdr"):
        assert name in _lib.EXPORTED_SYMBOLS


def test_python_face_refuses_before_it_looks_at_a_device():
    import torch
    import audiodenoiser_amd as pkg
    from audiodenoiser_amd import beamform
    from audiodenoiser_amd.beamform import Beamformer, MvdrParams, mvdr
    for name in beamform.__all__:
        assert getattr(pkg, name) is getattr(beamform, name) and name in pkg.__all__
    spec = torch.zeros((6, 5, 9), dtype=torch.complex64)
    mag = torch.zeros((6, 1, 9, 5))
    for channels in (0, 9, -2, 2.0, True, "2"):
        with pytest.raises(ValueError, match="channels"):
            mvdr(spec, mag, channels)
    with pytest.raises(ValueError, match="multiple of channels"):
        mvdr(spec, mag, 4)
    with pytest.raises(ValueError, match="ref_channel"):
        mvdr(spec, mag, 2, MvdrParams(ref_channel=2))
    with pytest.raises(TypeError):
        mvdr(spec, mag, 2, dict(ref_channel=0))
    with pytest.raises(ValueError, match="ROCm device"):                        # legal arguments: only the device is missing
        mvdr(spec, mag, 3)
    with pytest.raises(ValueError, match="ROCm device"):
        mvdr(spec.real, mag, 3)                                                 # and a dtype that is not complex64
    for bad in ("gain", None, 1):
        with pytest.raises(ValueError, match="mask must be 'spectral' or 'model'"):
            Beamformer(mask=bad)
    with pytest.raises(ValueError, match="needs a model"):
        Beamformer(mask="model")
    with pytest.raises(ValueError, match="needs a model"):
        Beamformer(model=object())
    with pytest.raises(TypeError, match="MvdrParams"):
        Beamformer(params=dict())
    with pytest.raises(TypeError, match="WpeParams"):
        Beamformer(wpe_params=dict())
    with pytest.raises(TypeError, match="SpectralParams"):
        Beamformer(gain_params=dict())
    with pytest.raises(ValueError, match="n_fft"):
        Beamformer(n_fft=500)
    with pytest.raises(ValueError, match="hop_length"):
        Beamformer(hop_length=512)
