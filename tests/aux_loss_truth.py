"""Float64 statement of the reference's auxiliary training terms (train.py:121-127 sky, 145-158 obj_acc_loss,
164-176 lidar depth) for the tests of gaussianrpg_amd.loss.aux_loss.  Differentiable with autograd.

The reference runs in float32, and three of its float32 details decide which pixels and which branches count,
so they are kept here while the arithmetic is float64:
  * the clamp bounds 1e-6 and 1 - 1e-6 and the 1e-10 of acc + 1e-10 are the float32 roundings of those constants;
  * the lidar term's selection -- which errors are among the k smallest -- is made on the reference's float32
    error |depth / (acc + 1e-10) - lidar| (uint32 bit order: NaN above +inf), k = int(0.95 * N);
  * ties at the k-th float32 error t share its weight: c_lt errors below t get 1/k, the c_eq equal to t get
    (k - c_lt) / c_eq / k each (any choice among ties gives the same value; this is the subgradient the fused
    kernel uses).
The guard is the reference's torch.nonzero(depth_mask).any(): 0 with a zero gradient when N == 0 or the one
selected pixel is flat index 0; N == 1 elsewhere gives k == 0 and NaN with a zero gradient."""
import numpy as np
import torch

LO = float(np.float32(1e-6))
HI = float(np.float32(1.0 - 1e-6))
EPS = float(np.float32(1e-10))


def selection(lidar, mask=None):
    sel = lidar > 0
    if mask is not None:
        sel = sel & mask.bool()
    return sel


def errors32(depth, acc, lidar):
    """The reference's float32 error plane (no FMA: one rounding per operation)."""
    d, a, l = depth.float(), acc.float(), lidar.float()
    return torch.abs(d / (a + 1e-10) - l)


def lidar_weights(depth, acc, lidar, mask=None):
    """-> (weights [same shape, float64, 0 outside the k smallest], N, k, t (float32), c_lt, c_eq, zero)."""
    sel = selection(lidar, mask)
    N = int(sel.sum())
    k = int(0.95 * N)
    zero = not bool(torch.nonzero(sel).any())
    w = torch.zeros(sel.shape, dtype=torch.float64, device=sel.device)
    if zero or k == 0:
        return w, N, k, 0.0, 0, 0, zero
    keys = errors32(depth, acc, lidar).view(torch.int32).to(torch.int64)   # |x| bits: non-negative
    keys = torch.where(sel, keys, torch.full_like(keys, 1 << 40))
    tkey = int(torch.sort(keys.reshape(-1)).values[k - 1])
    c_lt = int((keys < tkey).sum())
    c_eq = int((keys == tkey).sum())
    w = torch.where(keys < tkey, torch.full_like(w, 1.0 / k), w)
    w = torch.where(keys == tkey, torch.full_like(w, (k - c_lt) / c_eq / k), w)
    t = float(torch.tensor([tkey], dtype=torch.int32).view(torch.float32))
    return w, N, k, t, c_lt, c_eq, zero


def lidar(depth, acc, lidar_depth, mask=None):
    w, N, k, t, c_lt, c_eq, zero = lidar_weights(depth.detach(), acc.detach(), lidar_depth, mask)
    no = torch.zeros(depth.shape, dtype=torch.bool, device=depth.device)
    nothing = torch.where(no, depth, 0).sum() + torch.where(no, acc, 0).sum()   # 0, zero gradient, even with NaN
    if zero:
        return nothing
    if k == 0:
        return nothing + float("nan")
    keep = w > 0     # the other pixels get no gradient (not even a NaN one from an excluded NaN error)
    one = torch.ones_like(w)
    d = torch.where(keep, depth.double(), one)
    a = torch.where(keep, acc.double(), one)
    e = torch.abs(d / (a + EPS) - torch.where(keep, lidar_depth.double(), one))
    return (w * e).sum()


def _clamp(x):
    return torch.clamp(x.double(), min=LO, max=HI)


def sky(acc, sky_mask, scale=1.0):
    a = _clamp(acc)
    return torch.where(sky_mask.bool(), -torch.log(1 - a), -torch.log(a)).mean() * scale


def obj(acc_obj, obj_bound):
    a = _clamp(acc_obj)
    return torch.where(obj_bound.bool(), -(a * torch.log(a) + (1 - a) * torch.log(1 - a)), -torch.log(1 - a)).mean()


def total(depth, acc, *, lidar_depth=None, mask=None, sky_mask=None, sky_scale=1.0, acc_obj=None, obj_bound=None,
          lambda_depth_lidar=0.0, lambda_sky=0.0, lambda_reg=0.0):
    out = 0.0
    if lambda_depth_lidar > 0 and lidar_depth is not None:
        out = out + lambda_depth_lidar * lidar(depth, acc, lidar_depth, mask)
    if lambda_sky > 0 and sky_mask is not None:
        out = out + lambda_sky * sky(acc, sky_mask, sky_scale)
    if lambda_reg > 0 and acc_obj is not None and obj_bound is not None:
        out = out + lambda_reg * obj(acc_obj, obj_bound)
    return out
