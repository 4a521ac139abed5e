"""Float64 statements of the reference's per-Gaussian regularisers and of its PSNR, for the tests of
gaussianrpg_amd.loss.scale_flatten_loss / opacity_sparse_loss / gaussian_reg_loss / psnr, written out as the reference
writes them.  Differentiable with autograd.  The float32 twins are the reference's own arithmetic.

  scale_flatten: gaussian_model.py:271-280 behind get_scaling = exp(_scaling); torch.sort(stable=True), so equal values
                 keep their index order
  opacity_sparse: train.py:197-203 behind get_opacity = cat(sigmoid(_opacity) of every model); the boolean gather by
                 visibility_filter = radii > 0
  psnr:          loss_utils.py:61-78"""
import torch


def _scale_flatten(scaling, activated, dtype):
    scales = scaling.to(dtype)
    if not activated:
        scales = torch.exp(scales)
    sorted_scales = torch.sort(scales, dim=1, descending=False, stable=True).values
    s1, s2, s3 = sorted_scales[:, 0], sorted_scales[:, 1], sorted_scales[:, 2]
    s1 = torch.clamp(s1, 0, 30)
    s2 = torch.clamp(s2, 1e-5, 30)
    s3 = torch.clamp(s3, 1e-5, 30)
    scale_flatten_loss = torch.abs(s1).mean()
    scale_flatten_loss = scale_flatten_loss + torch.abs(s2 / s3 + s3 / s2 - 2.).mean()
    return scale_flatten_loss


def scale_flatten64(scaling, activated=False):
    return _scale_flatten(scaling, activated, torch.float64)


def scale_flatten32(scaling, activated=False):
    return _scale_flatten(scaling, activated, torch.float32)


def _opacity_sparse(opacities, radii, activated, dtype):
    if isinstance(opacities, torch.Tensor):
        opacities = [opacities]
    parts = [o.to(dtype).reshape(-1, 1) for o in opacities]
    opacity = torch.cat([p if activated else torch.sigmoid(p) for p in parts], dim=0)    # get_opacity
    visibility_filter = radii > 0
    opacity = opacity.clamp(1e-6, 1 - 1e-6)
    log_opacity = opacity * torch.log(opacity)
    log_one_minus_opacity = (1 - opacity) * torch.log(1 - opacity)
    return -1 * (log_opacity + log_one_minus_opacity)[visibility_filter].mean()


def opacity_sparse64(opacities, radii, activated=False):
    return _opacity_sparse(opacities, radii, activated, torch.float64)


def opacity_sparse32(opacities, radii, activated=False):
    return _opacity_sparse(opacities, radii, activated, torch.float32)


def _psnr(img1, img2, mask, dtype):
    img1 = img1.to(dtype).permute(1, 2, 0)
    img2 = img2.to(dtype).permute(1, 2, 0)
    if mask is not None:
        mask = mask.reshape(mask.shape[-2:]).bool()     # mask.squeeze(0)
        img1 = img1[mask]
        img2 = img2[mask]
    mse = torch.mean((img1 - img2) ** 2)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def psnr64(img1, img2, mask=None):
    return _psnr(img1, img2, mask, torch.float64)


def psnr32(img1, img2, mask=None):
    return _psnr(img1, img2, mask, torch.float32)
