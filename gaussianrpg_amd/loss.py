"""Fused SSIM + L1 training loss on the gfx950 kernels of csrc/ssim.hip.

Drop-ins for the reference's loss code (lib/utils/loss_utils.py) and its training mix (train.py:116-118):

  ssim(img1, img2, window_size=11, size_average=True, mask=None)   == loss_utils.ssim
  l1_loss(network_output, gt, mask=None)                            == loss_utils.l1_loss
  l1_ssim_loss(image, gt, mask=None, lambda_l1=1.0, lambda_dssim=0.2)
      == (1 - lambda_dssim) * lambda_l1 * l1_loss(image, gt, mask)
         + lambda_dssim * (1 - ssim(image, gt, mask=mask))
      in one forward and one backward launch chain; returns (loss, Ll1, ssim), the last two detached
      device scalars for logging.

Inputs are float32 device tensors [C,H,W] or [B,C,H,W] (non-contiguous ones are copied).  The mask is a
bool (or uint8) tensor that broadcasts against the image the way ``torch.where(mask, img, 0)`` does.
Only the first image receives a gradient.  No host synchronisation in forward or backward.  There is no
CPU or PyTorch fallback: CPU tensors, other dtypes, window_size != 11, mismatched shapes and a second
image that requires a gradient are errors.
"""
import torch

from .rasterizer import _C

__all__ = ["ssim", "l1_loss", "l1_ssim_loss"]


def _check(img1, img2, what=("img1", "img2")):
    for t, n in zip((img1, img2), what):
        if not isinstance(t, torch.Tensor):
            raise TypeError("gaussianrpg_amd.loss: %s must be a torch.Tensor" % n)
        if t.dtype != torch.float32:
            raise TypeError("gaussianrpg_amd.loss: %s must be float32 (got %s)" % (n, t.dtype))
    if img1.shape != img2.shape:
        raise ValueError("gaussianrpg_amd.loss: %s and %s must have the same shape (got %s and %s)"
                         % (what[0], what[1], tuple(img1.shape), tuple(img2.shape)))
    if img1.dim() not in (3, 4):
        raise ValueError("gaussianrpg_amd.loss: images must be [C,H,W] or [B,C,H,W] (got %s)" % (tuple(img1.shape),))
    if img2.requires_grad:
        raise ValueError("gaussianrpg_amd.loss: %s requires a gradient; the fused loss differentiates only %s "
                         "(the reference's ground truth never requires one)" % (what[1], what[0]))
    for t, n in zip((img1, img2), what):
        if not t.is_cuda:
            raise RuntimeError("gaussianrpg_amd.loss: %s must live on a ROCm/HIP device (torch device 'cuda'); "
                               "the fused loss is MI355X-native and has no CPU path" % n)
    if img1.device != img2.device:
        raise ValueError("gaussianrpg_amd.loss: images on different devices")


def _as4(img):
    return (img if img.dim() == 4 else img.unsqueeze(0)).contiguous()


def _mask4(mask, img, B, C, H, W):
    """mask broadcast like torch.where(mask, img, 0) -> uint8 [1|B, 1|C, H, W] (empty: no mask)."""
    if mask is None:
        return torch.empty(0, dtype=torch.uint8, device=img.device)
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError("gaussianrpg_amd.loss: mask must be a bool (or uint8) tensor")
    if mask.device != img.device:
        raise ValueError("gaussianrpg_amd.loss: mask must be on %s (got %s)" % (img.device, mask.device))
    if mask.dim() > img.dim():
        raise ValueError("gaussianrpg_amd.loss: mask %s has more dimensions than the image %s"
                         % (tuple(mask.shape), tuple(img.shape)))
    m = mask.reshape((1,) * (4 - mask.dim()) + tuple(mask.shape))
    for have, want in zip(m.shape, (B, C, H, W)):
        if have not in (1, want):
            raise ValueError("gaussianrpg_amd.loss: mask %s does not broadcast against the image %s"
                             % (tuple(mask.shape), tuple(img.shape)))
    if m.shape[2] != H or m.shape[3] != W:
        m = m.expand(m.shape[0], m.shape[1], H, W)
    return m.to(torch.uint8).contiguous()


class _FusedLoss(torch.autograd.Function):
    """[B,C,H,W] images -> stats [4 + B]: loss, L1 mean, SSIM mean, selected count, SSIM per image."""

    @staticmethod
    def forward(ctx, img1, img2, mask, w_l1, w_ssim):
        stats, saved = _C.ssim_forward(img1, img2, mask, float(w_l1), float(w_ssim), bool(ctx.needs_input_grad[0]))
        ctx.save_for_backward(img1, img2, mask, stats, saved)
        ctx.w = (float(w_l1), float(w_ssim))
        return stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats):
        img1, img2, mask, stats, saved = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = _C.ssim_backward(img1, img2, mask, ctx.w[0], ctx.w[1], stats, saved, grad_stats.contiguous())
        return g, None, None, None, None


def _run(img1, img2, mask, w_l1, w_ssim):
    a, b = _as4(img1), _as4(img2)
    B, C, H, W = a.shape
    return _FusedLoss.apply(a, b, _mask4(mask, img1, B, C, H, W), w_l1, w_ssim)


def ssim(img1, img2, window_size=11, size_average=True, mask=None):
    """loss_utils.ssim: mean SSIM (11x11 Gaussian window, sigma 1.5); with [B,C,H,W] input and
    size_average=False the per-image means [B]."""
    if window_size != 11:
        raise ValueError("gaussianrpg_amd.loss.ssim: only window_size == 11 is supported (got %r)" % (window_size,))
    _check(img1, img2)
    if not size_average and img1.dim() != 4:
        raise ValueError("gaussianrpg_amd.loss.ssim: size_average=False needs [B,C,H,W] input "
                         "(the reference's ssim_map.mean(1).mean(1).mean(1) fails on [C,H,W])")
    stats = _run(img1, img2, mask, 0.0, 0.0)
    return stats[2] if size_average else stats[4:]


def l1_loss(network_output, gt, mask=None):
    """loss_utils.l1_loss: mean |network_output - gt| over the selected elements (NaN for an all-false mask)."""
    _check(network_output, gt, ("network_output", "gt"))
    return _run(network_output, gt, mask, 0.0, 0.0)[1]


def l1_ssim_loss(image, gt, mask=None, lambda_l1=1.0, lambda_dssim=0.2):
    """train.py:116-118: (1 - lambda_dssim) * lambda_l1 * L1 + lambda_dssim * (1 - SSIM).
    Returns (loss, Ll1, ssim); Ll1 and ssim are detached device scalars."""
    _check(image, gt, ("image", "gt"))
    stats = _run(image, gt, mask, (1.0 - lambda_dssim) * lambda_l1, lambda_dssim)
    return stats[0], stats[1].detach(), stats[2].detach()
