"""Float64 statement of the reference's mono-normal training term (train.py:206-225) behind the renderer's
F.normalize(normals, dim=0) (street_gaussian_renderer.py:245-246), for the tests of gaussianrpg_amd.loss.normal_loss,
written out as the reference writes it: the permutes, the matmul with R.T, the boolean gathers.  Differentiable with
autograd.  The same in float32 (terms32) is the reference's own arithmetic.

  normals, mono_normal: [3,H,W]; world_view_transform: [4,4]; mask, sky_mask: bool [1,H,W] (or [H,W]) or None
  normalize: normals are the raw planes and F.normalize(dim=0) is applied first

Named deviation: with sky_mask None the reference indexes [H,W,3] with the un-squeezed [1,H,W] mask, which raises for
H > 1; the squeezed mask is used here, which is what the code intends.  With neither mask every pixel is selected."""
import torch


def selection(mask, sky_mask, H, W, top_rows=50):
    """train.py:208-213 -> bool [H,W]."""
    if mask is None:
        mask = torch.ones(1, H, W, dtype=torch.bool, device=sky_mask.device if sky_mask is not None else None)
    mask = mask.reshape(1, H, W).bool()
    if sky_mask is None:
        return mask.squeeze(0)
    normal_mask = torch.logical_and(mask, ~sky_mask.reshape(1, H, W).bool())
    normal_mask = normal_mask.squeeze(0).clone()
    normal_mask[:top_rows] = False
    return normal_mask


def _terms(normals, mono_normal, world_view_transform, mask, sky_mask, normalize, top_rows, dtype):
    normals = normals.to(dtype)
    if normalize:
        normals = torch.nn.functional.normalize(normals, dim=0)
    H, W = normals.shape[1:]
    normal_mask = selection(mask, sky_mask, H, W, top_rows).to(normals.device)
    normal_gt = mono_normal.to(dtype).permute(1, 2, 0)
    R_c2w = world_view_transform.to(dtype)[:3, :3]
    normal_gt = torch.matmul(normal_gt, R_c2w.T)
    normal_pred = normals.permute(1, 2, 0)
    normal_l1_loss = torch.abs(normal_pred[normal_mask] - normal_gt[normal_mask]).mean()
    normal_cos_loss = (1. - torch.sum(normal_pred[normal_mask] * normal_gt[normal_mask], dim=-1)).mean()
    return normal_l1_loss, normal_cos_loss, int(normal_mask.sum())


def terms64(normals, mono_normal, world_view_transform, mask=None, sky_mask=None, normalize=True, top_rows=50):
    """(normal_l1_loss, normal_cos_loss, n_selected) in float64."""
    return _terms(normals, mono_normal, world_view_transform, mask, sky_mask, normalize, top_rows, torch.float64)


def terms32(normals, mono_normal, world_view_transform, mask=None, sky_mask=None, normalize=True, top_rows=50):
    return _terms(normals, mono_normal, world_view_transform, mask, sky_mask, normalize, top_rows, torch.float32)


def loss64(*a, **k):
    l1, cos, _ = terms64(*a, **k)
    return l1 + cos


def loss32(*a, **k):
    l1, cos, _ = terms32(*a, **k)
    return l1 + cos
