"""SHA-256 digests of U-Net forwards over every kernel-choice switch, dtype and batch size: one line per configuration.

A change that must not move a bit of the output (a refactoring of the host side: kernel choice, split counts, weight packing,
workspace plan) is checked by running this script at both commits on the same machine and comparing the two outputs as text:

    python tools/forward_digest.py > before.txt ; ...other commit... ; python tools/forward_digest.py > after.txt ; diff before.txt after.txt

Every line: mode, dtype, shape, adn_unet_workspace_bytes of that handle and shape, sha256(y), and with taps the sha256 of each block
output.  Fixed seeds, weights from make_state_dict.  The switches are read when a handle is created, so every mode runs in a fresh
child process; a child that fails ends the run (nothing more is started on the GPU)."""
import concurrent.futures
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SWITCHES = ("ADN_BATCH_INVARIANT", "ADN_WINO_TILE", "ADN_CONV_ALGO", "ADN_WINO_SPLITK", "ADN_CONVT_SPLIT", "ADN_F16_CONV",
            "ADN_F16_FIRST", "ADN_F16_CONVT", "ADN_AUTO_GRID", "ADN_AUTO_GRID64", "ADN_WINO_GEMM")
MODES = {                                   # tests/test_gpu_variants.py::MODES + the fp16 path's switches
    "default": {},
    "batch_invariant": {"ADN_BATCH_INVARIANT": "1"},
    "f2x2": {"ADN_WINO_TILE": "2"},
    "f4x4_forced": {"ADN_WINO_TILE": "4"},
    "direct": {"ADN_CONV_ALGO": "direct"},
    "splitk": {"ADN_WINO_SPLITK": "1"},
    "convt_exact": {"ADN_CONVT_SPLIT": "0"},
    "wino_gemm_off": {"ADN_WINO_GEMM": "0"},            # the three-stage F(4x4,3x3) form never / wherever its V and M fit
    "wino_gemm_all": {"ADN_WINO_GEMM": "2"},
    "f16_conv32": {"ADN_F16_CONV": "32"},
    "f16_first0": {"ADN_F16_FIRST": "0"},
    "f16_convt_dma": {"ADN_F16_CONVT": "dma"},
}
SHAPES = [(n, 513, 256) for n in (1, 2, 4, 16, 64)] + [(n, f, t) for f, t in ((257, 188), (40, 33)) for n in (1, 3)]


def sha(t):
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def digest_lines(mode, net, dtype, shapes, label=""):
    import torch
    from audiodenoiser_amd import _lib
    dev = torch.device("cuda", 0)
    need = ctypes.c_size_t()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        for n, f, t in shapes:
            x = (torch.rand((n, net.in_channels, f, t), generator=torch.Generator().manual_seed(7 + n)) * 4).to(dev)
            for with_taps in (False, True):
                with torch.no_grad():
                    out = net(x, return_taps=with_taps)
                y, taps = out if with_taps else (out, {})
                torch.cuda.synchronize()
                _lib.check(_lib.load().adn_unet_workspace_bytes(net._handle, n, f, t, ctypes.byref(need)), "adn_unet_workspace_bytes")
                names = ["y"] + list(taps)
                hashes = list(pool.map(sha, [y] + list(taps.values())))
                print(f"{mode}{label} {dtype} N={n} {f}x{t} taps={int(with_taps)} ws={need.value} "
                      + " ".join(f"{k}={h}" for k, h in zip(names, hashes)), flush=True)
                del out, y, taps


def child(mode):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from audiodenoiser_amd.model import UNet
    from audiodenoiser_amd.weights import make_state_dict
    dev = torch.device("cuda", 0)
    for dtype in ("f32", "f16"):
        digest_lines(mode, bench.make_net(make_state_dict(1234), dev, dtype), dtype, SHAPES)
        if mode == "default":                                 # UNet(2, 3): first / last convolution as their own launches
            net = UNet(2, 3)
            net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(1234, 2, 3).items()}, strict=True)
            digest_lines(mode, net.to(dev).eval().set_compute_dtype(dtype), dtype, [(2, 40, 33)], label="/UNet(2,3)")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for mode in (sys.argv[1:] or list(MODES)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env={**base, **MODES[mode]}, timeout=600).returncode
        if rc != 0:
            sys.exit(f"forward_digest: mode {mode} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
