"""Float64 statement of the reference's SSIM / L1 loss (lib/utils/loss_utils.py) for the tests of
gaussianrpg_amd.loss.  Pinned by tests/golden/ref_ssim.npz (tests/golden/make_golden_ssim.py).

The window is the reference's: the 1-D Gaussian (sigma 1.5) normalised in float32, its outer product
rounded to float32, then widened -- so a float64 run reproduces the reference's float64 run to rounding.
The mask zeroes both images; the SSIM mean covers every position, the L1 mean the selected elements."""
import math

import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def window(dtype=torch.float64):
    g = torch.tensor([math.exp(-((k - 5) ** 2) / 4.5) for k in range(11)], dtype=torch.float32)
    g = g / g.sum()
    return (g[:, None] * g[None, :]).to(dtype)


def _moments(x1, x2, w):
    """[..., C, H, W] -> the five windowed moments, each [..., C, H, W] (zero padding)."""
    shape = x1.shape
    C, H, W = shape[-3:]
    a = x1.reshape(-1, C, H, W)
    b = x2.reshape(-1, C, H, W)
    # one depthwise conv over the five stacked inputs
    stack = torch.cat([a, b, a * a, b * b, a * b], 1)
    k = w.to(device=stack.device, dtype=stack.dtype).expand(5 * C, 1, 11, 11)
    out = F.conv2d(stack, k, padding=5, groups=5 * C)
    return [t.reshape(shape) for t in out.split(C, 1)]


def ssim_map(img1, img2, mask=None):
    if mask is not None:
        img1 = torch.where(mask, img1, torch.zeros_like(img1))
        img2 = torch.where(mask, img2, torch.zeros_like(img2))
    mu1, mu2, e11, e22, e12 = _moments(img1, img2, window(img1.dtype))
    s1 = e11 - mu1 * mu1
    s2 = e22 - mu2 * mu2
    s12 = e12 - mu1 * mu2
    num = (2 * mu1 * mu2 + C1) * (2 * s12 + C2)
    den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2)
    return num / den


def ssim(img1, img2, size_average=True, mask=None):
    m = ssim_map(img1, img2, mask)
    if size_average:
        return m.mean()
    return m.flatten(1).mean(1)


def l1(img1, img2, mask=None):
    d = (img1 - img2).abs()
    if mask is None:
        return d.mean()
    sel = torch.broadcast_to(mask, d.shape)
    return d[sel].mean()


def mix(img1, img2, mask=None, lambda_l1=1.0, lambda_dssim=0.2):
    """train.py:118"""
    return (1.0 - lambda_dssim) * lambda_l1 * l1(img1, img2, mask) + lambda_dssim * (1.0 - ssim(img1, img2, mask=mask))
