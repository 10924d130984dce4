"""Every layout the WPE and MVDR kernels can be asked for has a device parity case (no GPU): tests/variant_cover.py enumerates the
legal parameter sets under the key of the host-side choices, and the case tables of the device tests are read for what runs
against float64.  A table that loses a layout fails here.

* adn_wpe_mc: the enumeration gives 24 keys (LPB, WINDOW, cq, partial last row block, partial last P block, doubled), written out
  below with their members; each has a case in dereverb_mc_cases.PARITY_CK or VARIANT_CK.
* adn_wpe: three lane groupings x {K % 4 == 0, != 0}: six keys, all legal (K = 32 is the only member of 64 lanes with a whole last
  block row); K = 1, 19 | 20 | 21 | 28 | 29 | 32 run on the device.
* adn_mvdr, adn_mvdr_online: one instantiation per C = 1 .. 8; all eight run.  adn_wpe_mc_online: C = 2 .. 8 all run.
* The variant tables are exactly the lists they were chosen as: a case taken out of one fails here even where another member of
  its key remains.
* No variant case has a float32 floor above its cap (5e-4 for the solvers and adn_mvdr_online, recursive_bounds.CAP for
  adn_wpe_mc_online): a case over the cap bounds nothing and is replaced by another member of its key, never loosened.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_stream_cases as bsc  # noqa: E402
import dereverb_cases as dc  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_stream_cases as msc  # noqa: E402
import recursive_bounds as rb  # noqa: E402
import solver_bounds as sb  # noqa: E402
import variant_cover as vc  # noqa: E402

T, F = True, False
# (LPB, WINDOW, cq, partial last row block, partial last P block, doubled) -> its legal (C, K); the first seven are the keys of
# PARITY_CK, the other seventeen had no device case before VARIANT_CK
WPE_MC_KEYS = {
    (16, F, 1, T, T, F): ((2, 1), (2, 3), (2, 5), (2, 7)),
    (32, F, 1, F, T, F): ((2, 10),),
    (32, F, 1, T, T, F): ((2, 9), (2, 11), (3, 6), (3, 7)),
    (32, T, 1, F, T, F): ((2, 12), (3, 8)),
    (64, T, 1, F, T, F): ((2, 16),),
    (64, T, 1, F, F, F): ((4, 8),),
    (64, T, 2, F, F, F): ((8, 4),),
    (16, F, 1, F, T, F): ((2, 2), (2, 6)),
    (16, T, 1, F, T, F): ((2, 4), (2, 8)),
    (32, F, 1, F, F, F): ((4, 5), (4, 6)),
    (32, F, 1, F, F, T): ((4, 1), (4, 2), (4, 3)),
    (32, F, 1, T, T, T): ((3, 1), (3, 2), (3, 3), (3, 5)),
    (32, T, 1, F, F, T): ((4, 4),),
    (32, T, 1, F, T, T): ((3, 4),),
    (64, F, 1, F, F, F): ((4, 7),),
    (64, F, 1, F, T, F): ((2, 14),),
    (64, F, 1, T, T, F): ((2, 13), (2, 15), (3, 9), (3, 10)),
    (64, F, 2, F, F, F): ((8, 3),),
    (64, F, 2, F, F, T): ((8, 1), (8, 2)),
    (64, F, 2, F, T, T): ((6, 2),),
    (64, F, 2, T, T, F): ((5, 5), (5, 6), (6, 5), (7, 3)),
    (64, F, 2, T, T, T): ((5, 1), (5, 2), (5, 3), (6, 1), (6, 3), (7, 1), (7, 2)),
    (64, T, 2, F, T, F): ((6, 4), (7, 4)),
    (64, T, 2, F, T, T): ((5, 4),),
}
WPE_KEYS = {(16, F): tuple(k for k in range(1, 21) if k % 4), (16, T): (4, 8, 12, 16, 20), (32, F): (21, 22, 23, 25, 26, 27),
            (32, T): (24, 28), (64, F): (29, 30, 31), (64, T): (32,)}
MVDR_KEYS = {(1, 4, 1): (1,), (2, 4, 1): (2,), (3, 4, 2): (3,), (4, 4, 3): (4,), (5, 8, 2): (5,), (6, 8, 3): (6,), (7, 8, 4): (7,),
             (8, 8, 5): (8,)}


def _as_tuples(variants):
    return {k: tuple(v) for k, v in variants.items()}


def test_the_enumeration_gives_the_written_keys():
    assert len(WPE_MC_KEYS) == 24 and _as_tuples(vc.wpe_mc_variants()) == WPE_MC_KEYS
    assert sum(len(v) for v in WPE_MC_KEYS.values()) == len(vc.wpe_mc_legal()) == sum(32 // c for c in range(2, 9))
    assert _as_tuples(vc.wpe_variants()) == WPE_KEYS and sum(len(v) for v in WPE_KEYS.values()) == 32
    assert _as_tuples(vc.mvdr_variants()) == MVDR_KEYS
    # the doubling loop is what the written rule of csrc/dereverb_mc_kernels.hip says: at most 32 cells per staged frame row
    for c, k in vc.wpe_mc_legal():
        lanes = vc.wpe_mc_lanes_per_bin(c, k)
        assert lanes in (16, 32, 64) and (256 // lanes) * c <= 32 and vc.wpe_mc_blocks(c, k) <= lanes
    # params = NULL: taps = 32 / C, the rule the Python classes restate
    from audiodenoiser_amd.dereverb import WpeParams, WpeStreamParams, _joint_params, _joint_stream_params
    for c in range(1, 9):
        assert vc.joint_default_taps(c) == 32 // c == _joint_params("test", None, c).taps == _joint_stream_params("test", None, c).taps
        assert _joint_params("test", None, c) == WpeParams(taps=32 // c)
        assert _joint_stream_params("test", None, c) == WpeStreamParams(taps=32 // c)


def test_every_key_has_a_device_parity_case():
    assert vc.uncovered(vc.wpe_mc_variants(), vc.wpe_mc_device_pairs()) == []
    assert vc.uncovered(vc.wpe_variants(), vc.wpe_device_taps()) == []
    assert vc.uncovered(vc.mvdr_variants(), vc.mvdr_device_channels()) == [] and vc.mvdr_device_channels() == tuple(range(1, 9))
    assert vc.uncovered(vc.mvdr_variants(), vc.mvdr_online_device_channels()) == []
    assert vc.mvdr_online_device_channels() == tuple(range(1, 9))
    assert sorted({c for c, _ in vc.wpe_mc_online_device_pairs()}) == list(range(2, 9))
    # every device case is a legal parameter set
    assert set(vc.wpe_mc_device_pairs()) <= set(vc.wpe_mc_legal()) and set(vc.wpe_mc_online_device_pairs()) <= set(vc.wpe_mc_legal())
    assert set(vc.wpe_device_taps()) <= set(vc.wpe_legal())
    # the documented defaults of a 3-, 5-, 6- and 7-microphone recording run, offline and streaming
    for c in (3, 5, 6, 7):
        assert (c, vc.joint_default_taps(c)) in vc.wpe_mc_device_pairs()
    for c in (5, 6, 7):
        assert (c, vc.joint_default_taps(c)) in vc.wpe_mc_online_device_pairs()
    # before the variant tables: 7 of the 24 keys, 3 of the 6, C = 4, 6, 7 missing
    parity = {tuple(ck) for _, _, ck, _ in mc.parity_cases()}
    assert len(vc.uncovered(vc.wpe_mc_variants(), parity)) == 17
    assert vc.uncovered(vc.wpe_variants(), (1, 20, 32)) == [(32, F), (32, T), (64, F)]


def test_the_variant_tables_are_the_lists_they_were_chosen_as():
    assert dc.VARIANT_TAPS == (19, 21, 28, 29) and dc.VARIANT_FRAMES == (23, 97)
    assert mc.VARIANT_CK == ((2, 6), (2, 8), (4, 5), (4, 2), (3, 2), (4, 4), (3, 4), (4, 7), (2, 14), (3, 10), (8, 3), (8, 1), (6, 2),
                             (5, 6), (5, 2), (7, 4), (5, 4), (6, 5), (7, 1)) and mc.VARIANT_FRAMES == (23, 97)
    assert msc.VARIANT_CK == ((5, 6), (6, 5), (7, 4), (5, 2), (7, 1)) and msc.VARIANT_FRAMES == (4, 23, 97)
    assert bc.VARIANT_CHANNELS == (4, 6, 7) and bc.VARIANT_REF_CASE == (64, 65, 6, (3,))
    assert bsc.VARIANT_CHANNELS == (4, 6, 7)
    assert bsc.VARIANT_ADDED == ((65, 4, dict(refresh=4, forget=0.9), dict()), (23, 7, dict(ref_channel=6), dict()))
    assert len(list(dc.variant_cases())) == 8 and len(list(mc.variant_cases())) == 38 and len(list(msc.variant_cases())) == 15
    assert len(list(bc.variant_cases())) == 3 * len(bc.PARITY_FRAMES) + 1 and bc.PARITY_FRAMES == (1, 2, 23, 65, 97)
    assert len(list(bsc.variant_cases())) == 3 * len(bsc.PARITY_FRAMES) + 2 and bsc.PARITY_FRAMES == (1, 2, 23, 65)
    # all at n_fft 64: F = 33 ends in a partial tile for every tile width (16, 8, 4 bins)
    assert all(case[0] == 64 for cases in (dc.variant_cases(), mc.variant_cases(), msc.variant_cases(), bc.variant_cases())
               for case in cases) and bsc.N_FFT == 64
    # one pair per key that had none, and the two added beside them
    keys = [vc.wpe_mc_key(*ck) for ck in mc.VARIANT_CK[:17]]
    parity = {vc.wpe_mc_key(*ck) for ck in mc.PARITY_CK}
    assert len(set(keys)) == 17 and not set(keys) & parity and set(keys) | parity == set(WPE_MC_KEYS)
    # the host tables hold a row for every one of them
    labels = [label for label, _ in sb.host_cases()] + [label for label, _ in rb.host_cases()]
    assert len(set(labels)) == len(labels)
    assert sum(" variant " in label for label in labels) == 8 + 38 + 16 + 15


def test_no_variant_case_has_a_floor_above_its_cap():
    assert sb.VARIANT_CAP == bsc.VARIANT_CAP == 5e-4 and rb.CAP == 1e-4
    worst = {}
    for label, thunk in sb.variant_cases():
        b = thunk()
        assert sb.EPS <= b.floor <= sb.VARIANT_CAP, (label, b.floor)
        op = label.split()[0]
        worst[op] = max(worst.get(op, (0.0, "")), (b.floor, label))
    for case in bsc.variant_cases():
        n_frames, channels, params, extra = case
        b = bsc.bounds(*bsc.host_inputs(n_frames, channels), channels, params)
        assert sb.EPS <= b.floor <= bsc.VARIANT_CAP, (case, b.floor)
        worst["mvdr_stream"] = max(worst.get("mvdr_stream", (0.0, "")), (b.floor, bsc.label(*case, kind="variant")))
    for label, thunk in rb.variant_cases():
        b = thunk()
        rb.assert_cap(label, b)
        worst["wpe_mc_online"] = max(worst.get("wpe_mc_online", (0.0, "")), (b.floor, label))
    for op, (floor, label) in worst.items():
        print(f"largest host floor of the variant cases of {op}: {floor:.3g} ({label})")
