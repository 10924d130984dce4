"""`from loss import CombinedPerceptualLoss` (reference code/loss.py) resolved to the device implementation
(per-clip kernels; `loss.backward()` runs the HIP backward, as in train.py:67-68)."""
from audiodenoiser_amd.loss import CombinedPerceptualLoss  # noqa: F401
