"""What the WPE and MVDR kernels can be asked to be, and which device parity case asks for it -- TEST INFRASTRUCTURE.

The layout of a kernel of the WPE / MVDR family is fixed on the host from its parameters.  This module restates those choices in
Python, each beside the name of the C++ function it mirrors, enumerates every legal parameter set with its key, and reads the
case tables of the device tests (tests/*_cases.py) for the parameter sets that run against float64.  tests/test_variant_cover_host.py
asserts that every key has a case: a case table that drops a layout, or a host function that gains one, fails there.

Nothing here is exported by the library and nothing looks at a compiled kernel: the restatements are held to the keys and members
written out in the host test, so a change to either side shows there.

    python tests/variant_cover.py           prints every key with its legal parameter sets and the ones that run on the device
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beamform_cases as bc  # noqa: E402
import beamform_stream_cases as bsc  # noqa: E402
import dereverb_cases as dc  # noqa: E402
import dereverb_mc_cases as mc  # noqa: E402
import dereverb_mc_stream_cases as msc  # noqa: E402

MAX_STACKED = 32                                       # K <= 32 (adn_wpe), C K <= 32 (adn_wpe_mc): the ranges of include/adn.h
MAX_CHANNELS = 8
DEFAULT_TAPS = 20                                      # adn_wpe_params.taps


# ---- adn_wpe (csrc/dereverb_kernels.hip) -----------------------------------------------------------------------------------------
def wpe_lanes_per_bin(taps):
    """wpe_lanes_per_bin: the smallest of 16, 32, 64 lanes that holds the nb (nb + 1) / 2 blocks of the lower triangle."""
    return 16 if taps <= 20 else 32 if taps <= 28 else 64


def wpe_key(taps):
    """(lanes per bin, whether the last block row is whole: K % 4 == 0)."""
    return wpe_lanes_per_bin(taps), taps % 4 == 0


def wpe_legal():
    return tuple(range(1, MAX_STACKED + 1))


# ---- adn_wpe_mc (csrc/dereverb_mc_kernels.hip) -----------------------------------------------------------------------------------
WPE_MC_THREADS = 256
WPE_MC_CELLS = 32                                      # most (channel, bin) cells of a staged frame row


def wpe_mc_blocks(channels, taps):
    """wpe_mc_blocks: nb (nb + 1) / 2 blocks of R's lower triangle and nb ceil(C / 4) of P, nb = ceil(C K / 4)."""
    nb = (channels * taps + 3) // 4
    return nb * (nb + 1) // 2 + nb * ((channels + 3) // 4)


def wpe_mc_lanes_for_blocks(channels, taps):
    """The first statement of wpe_mc_lanes_per_bin: the smallest of 16, 32, 64 lanes that holds the blocks."""
    blocks = wpe_mc_blocks(channels, taps)
    return 16 if blocks <= 16 else 32 if blocks <= 32 else 64


def wpe_mc_lanes_per_bin(channels, taps):
    """wpe_mc_lanes_per_bin: ... doubled until the tile's 256 / lanes bins times C channels are at most 32 cells."""
    lanes = wpe_mc_lanes_for_blocks(channels, taps)
    while (WPE_MC_THREADS // lanes) * channels > WPE_MC_CELLS:
        lanes *= 2
    return lanes


def joint_default_taps(channels):
    """joint_default_taps (csrc/adn_api.hip), and `_joint_rules` of audiodenoiser_amd: params = NULL is taps = 32 / C."""
    return MAX_STACKED // max(channels, 1)


def wpe_mc_key(channels, taps):
    """(LPB, WINDOW, cq, partial last row block, partial last P block, doubled), as launch_wpe_mc and wpe_mc_kernel take them:
    WINDOW is the template argument K % 4 == 0; cq = ceil(C / 4) the P block columns; N % 4 != 0 makes `min(4 rb + a, N - 1)` walk
    the last row again, C % 4 != 0 makes `min(4 cb + a, C - 1)` walk the last channel again; doubled: the `while` loop ran."""
    n = channels * taps
    lanes = wpe_mc_lanes_per_bin(channels, taps)
    return lanes, taps % 4 == 0, (channels + 3) // 4, n % 4 != 0, channels % 4 != 0, lanes > wpe_mc_lanes_for_blocks(channels, taps)


def wpe_mc_legal():
    """Every (C, K) adn_wpe_mc runs its own kernel for: 2 <= C <= 8, K >= 1, C K <= 32 (C = 1 is adn_wpe's kernel)."""
    return tuple((c, k) for c in range(2, MAX_CHANNELS + 1) for k in range(1, MAX_STACKED // c + 1))


# ---- adn_mvdr, adn_mvdr_online (csrc/beamform_kernels.hip, csrc/beamform_stream_kernels.hip) ----------------------------------------
def mvdr_lanes_per_bin(channels):
    """mvdr_lanes_per_bin: 4 lanes per bin up to C = 4, 8 beyond; the streaming kernel takes the same."""
    return 4 if channels <= 4 else 8


def mvdr_entries_per_lane(channels):
    """EPL = ceil(E / LPB), E = C (C + 1) / 2 entries of a covariance's lower triangle."""
    lanes = mvdr_lanes_per_bin(channels)
    return (channels * (channels + 1) // 2 + lanes - 1) // lanes


def mvdr_key(channels):
    """(C, lanes per bin, entries per lane): every channel count is its own instantiation of mvdr_kernel / mvdr_stream_kernel."""
    return channels, mvdr_lanes_per_bin(channels), mvdr_entries_per_lane(channels)


def mvdr_legal():
    return tuple(range(1, MAX_CHANNELS + 1))


# ---- every legal parameter set under its key ---------------------------------------------------------------------------------------
def _by_key(legal, key):
    out = {}
    for p in legal:
        out.setdefault(key(*p) if isinstance(p, tuple) else key(p), []).append(p)
    return out


def wpe_variants():
    """{key: [K, ...]} of adn_wpe."""
    return _by_key(wpe_legal(), wpe_key)


def wpe_mc_variants():
    """{key: [(C, K), ...]} of adn_wpe_mc."""
    return _by_key(wpe_mc_legal(), wpe_mc_key)


def mvdr_variants():
    """{key: [C]} of adn_mvdr and of adn_mvdr_online."""
    return _by_key(mvdr_legal(), mvdr_key)


# ---- what the case tables run on the device against float64 -----------------------------------------------------------------------
def wpe_device_taps():
    """The K of every adn_wpe case of tests/test_gpu_dereverb.py that is compared with the float64 restatement."""
    cases = list(dc.parity_cases()) + list(dc.variant_cases())
    return tuple(sorted({(kw or {}).get("taps", DEFAULT_TAPS) for _, _, kw in cases}))


def wpe_mc_device_pairs():
    """The (C, K) of every adn_wpe_mc case of tests/test_gpu_dereverb_mc.py that is compared with the float64 restatement."""
    cases = list(mc.parity_cases()) + list(mc.variant_cases())
    return tuple(sorted({tuple(ck) for _, _, ck, _ in cases}))


def wpe_mc_online_device_pairs():
    """The (C, K) of every adn_wpe_mc_online case of tests/test_gpu_dereverb_mc_stream.py compared with float64."""
    cases = list(msc.parity_cases()) + list(msc.variant_cases())
    return tuple(sorted({tuple(ck) for _, _, ck, _ in cases}))


def mvdr_device_channels():
    """The C of every adn_mvdr case of tests/test_gpu_beamform.py that is compared with the float64 restatement."""
    return tuple(sorted({c for _, _, c, _ in bc.parity_cases()} | {c for _, _, c, _ in bc.variant_cases()}))


def mvdr_online_device_channels():
    """The C of every adn_mvdr_online case of tests/test_gpu_beamform_stream.py that is compared with the float64 restatement."""
    return tuple(sorted({c for _, c, _, _ in bsc.parity_cases()} | {c for _, c, _, _ in bsc.variant_cases()}))


def uncovered(variants, device):
    """The keys of `variants` none of whose parameter sets is in `device`."""
    have = set(device)
    return sorted(k for k, members in variants.items() if not have.intersection(members))


def main():
    for name, variants, device in (("adn_wpe", wpe_variants(), wpe_device_taps()),
                                   ("adn_wpe_mc", wpe_mc_variants(), wpe_mc_device_pairs()),
                                   ("adn_mvdr", mvdr_variants(), mvdr_device_channels()),
                                   ("adn_mvdr_online", mvdr_variants(), mvdr_online_device_channels())):
        print(f"{name}: {len(variants)} keys, {len(uncovered(variants, device))} without a device case")
        for key in sorted(variants):
            ran = [p for p in variants[key] if p in set(device)]
            print(f"  {key}: legal {variants[key]}; on the device {ran or 'NONE'}")


if __name__ == "__main__":
    main()
