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
bool (or uint8) tensor that broadcasts against the image the way ``torch.where(mask, img, 0)`` does, and selects the
way it does: an element under a false mask counts as 0 whatever it holds.  Only the first image receives a gradient.  No host synchronisation in forward or backward.  There is no
CPU or PyTorch fallback: CPU tensors, other dtypes, window_size != 11, mismatched shapes and a second
image that requires a gradient are errors.

The auxiliary terms of train.py (csrc/aux_loss.hip), on float32 planes [H,W] or [1,H,W] and bool (or uint8)
masks of the same H x W:

  lidar_depth_loss(depth, acc, lidar_depth, mask=None)   == train.py:164-176 (lidar_depth_loss)
  sky_loss(acc, sky_mask, scale=1.0)                      == train.py:121-127 (sky_loss, times lambda_sky_scale)
  obj_acc_loss(acc_obj, obj_bound)                        == train.py:145-158 (obj_acc_loss)
  aux_loss(depth, acc, *, lidar_depth=None, mask=None, sky_mask=None, sky_scale=1.0, acc_obj=None,
           obj_bound=None, lambda_depth_lidar=0.0, lambda_sky=0.0, lambda_reg=0.0)
      == lambda_depth_lidar * lidar + lambda_sky * sky + lambda_reg * obj in one forward and one backward launch
      chain; returns (loss, terms), terms a dict of detached device scalars for scalar_dict with the keys of the
      terms that are on ('lidar_depth_loss', 'sky_loss', 'obj_acc_loss').  A lambda of 0 or a missing
      lidar_depth / sky_mask / acc_obj / obj_bound turns its term off (not evaluated, no gradient).

The lidar term keeps the reference's guard exactly, on the device: 0 with a zero gradient when no pixel is selected
or only flat index 0 is; NaN with a zero gradient when one other pixel is.  Ties at the k-th smallest error share
its weight evenly.  No host synchronisation in forward or backward.

The semantic term of train.py (csrc/semantic_loss.hip), on float32 planes [S,H,W] or [1,S,H,W] and int64 (or int32)
labels [H,W] or [1,H,W]:

  semantic_loss(semantic, gt_semantic, mode='logits', ignore_index=-1)   == train.py:129-143 (semantic_loss)
      F.cross_entropy(semantic[None], gt_semantic, ignore_index=-1, reduction='mean'), and 0 with a zero gradient
      when every label is -1: the reference's torch.all(gt_semantic == -1) guard, evaluated on the device.
      mode='probabilities' takes the RAW rendered planes and applies the normalise + log of
      street_gaussian_renderer.py:248-256 itself, log(x / (sum_c x + 1e-8) + 1e-8): do not transform them first.
  semantic_loss_stats(semantic, gt_semantic, mode='logits', ignore_index=-1)
      without a gradient: a dict of device tensors, 'loss' (float32), 'n_valid', 'n_bad', 'n_correct' (exact int64)
      and, for S <= 256, 'labels' (uint8 [H,W], the argmax channel, ties to the lowest).

A label outside [-1, S) is counted in n_bad and ignored (PyTorch raises a device assert there).  Only
ignore_index == -1 is provided.  No host synchronisation in forward or backward.

The mono-normal term of train.py (csrc/normal_loss.hip), on float32 planes [3,H,W]:

  normal_loss(normals, mono_normal, world_view_transform, mask=None, sky_mask=None, *, normalize=True, top_rows=50)
      == train.py:206-225 (normal_l1_loss + normal_cos_loss).  normalize=True takes the RAW planes (feature[:3] of
      forward_features) and applies the renderer's F.normalize(dim=0) itself; normalize=False takes
      render_pkg['normals'] as the reference holds it.  The rotation world_view_transform[:3,:3] is read on the device.
      With a sky mask the selection is mask & ~sky_mask minus the first top_rows rows; without one it is mask alone
      (squeezed: the reference's un-squeezed index raises for H > 1); without either, every pixel.
  normal_loss_terms(...same...)
      without a gradient: a dict of device tensors, 'normal_l1_loss', 'normal_cos_loss' (float32) and 'n_selected'
      (exact int64).

The per-Gaussian regularisers of train.py (csrc/reg_loss.hip):

  scale_flatten_loss(scaling, activated=False)             == gaussians.background.scale_flatten_loss()
      scaling: the raw _scaling, float32 [N,3] (exp is applied here); activated=True: get_scaling, used as given.
  opacity_sparse_loss(opacities, radii, activated=False)   == train.py:197-203
      opacities: one float32 [N_i,1] (or [N_i]) tensor or a list of them, each model's raw _opacity in composed
      order (the sigmoid is applied here; the get_opacity concatenation never runs); radii: int32 [sum N_i], the
      visibility filter is radii > 0, taken on the device.
  gaussian_reg_loss(*, scaling=None, opacities=None, radii=None, lambda_scale_flatten=0.0, lambda_opacity_sparse=0.0)
      == lambda_scale_flatten * scale_flatten + lambda_opacity_sparse * opacity_sparse in one forward and one
      backward launch chain; returns (loss, terms), terms a dict of detached device scalars under
      'scale_flatten_loss' / 'opacity_sparse_loss' for the terms that are on.  A lambda of 0 or a missing input turns
      its term off (not evaluated, no gradient).

  psnr(img1, img2, mask=None)                               == loss_utils.psnr (csrc/metrics.hip)
      float32 [C,H,W] images, a [1,H,W] or [H,W] mask selecting pixels; a detached device scalar.  NO gradient is
      provided (the reference calls it under torch.no_grad()).

An empty selection (no pixel, no visible Gaussian, N == 0) gives NaN with an exactly-zero gradient, as mean() of an
empty gather does.  No host synchronisation in any forward or backward, no atomics.

What a deselected element holds never reaches a result: the ops select as the reference's boolean gather and
torch.where do, they do not multiply by a 0/1 mask.  NaN, +-Inf or garbage in the elements below changes no bit of a
value, a count or a gradient, and the gradient there is exactly 0 (tests/test_gpu_selection.py):

  ssim, l1_loss, l1_ssim_loss            img1 / img2 where the (broadcast) mask is false
  psnr                                   img1 / img2 where the mask is false
  lidar_depth_loss, aux_loss (lidar)     depth and acc where !(lidar_depth > 0) or the mask is false (acc only while
                                         the sky term is off); lidar_depth where the mask is false is only compared
                                         with 0, and a NaN there deselects itself
  semantic_loss, semantic_loss_stats     every channel of a pixel whose label is -1 or outside [-1, S) (the 'labels'
                                         plane is the argmax of every pixel and does read them)
  normal_loss, normal_loss_terms         normals / mono_normal outside mask & ~sky_mask & (row >= top_rows)
  opacity_sparse_loss, gaussian_reg_loss the opacities of Gaussians with radii <= 0
  optim.densification_stats_update       the viewspace_grad rows of Gaussians with radii <= 0

sky_loss and obj_acc_loss read EVERY pixel, by the reference's own definition: their masks only choose the branch of
a torch.where over the whole plane, so a NaN anywhere in acc / acc_obj makes the term NaN.  scale_flatten_loss reads
every Gaussian.  A NaN at a selected element of the ops above shows in the value as it does in the reference (in the
lidar term by its top-k rule: a NaN error sorts above +inf).
"""
import torch

from .rasterizer import _C

__all__ = ["ssim", "l1_loss", "l1_ssim_loss", "aux_loss", "lidar_depth_loss", "sky_loss", "obj_acc_loss",
           "lidar_selection", "semantic_loss", "semantic_loss_stats", "normal_loss", "normal_loss_terms",
           "scale_flatten_loss", "opacity_sparse_loss", "gaussian_reg_loss", "psnr"]


_FLOAT = ((torch.float32,), "float32")
_MASK = ((torch.bool, torch.uint8), "a bool (or uint8) tensor")
_LABEL = ((torch.int64, torch.int32), "int64 or int32")
_RADII = ((torch.int32,), "int32")


def _tensor_of(t, name, kind=None):
    """t is a torch.Tensor, of one of the dtypes of kind = (dtypes, how the message names them)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("gaussianrpg_amd.loss: %s must be a torch.Tensor" % name)
    if kind is not None and t.dtype not in kind[0]:
        raise TypeError("gaussianrpg_amd.loss: %s must be %s (got %s)" % (name, kind[1], t.dtype))


def _on_device(named, device, different):
    """Every (name, tensor) of named lives on a ROCm device, and on this one; different(name, tensor) words the
    complaint about another."""
    for n, t in named:
        if not t.is_cuda:
            raise RuntimeError("gaussianrpg_amd.loss: %s must live on a ROCm/HIP device (torch device 'cuda'); "
                               "the fused loss is MI355X-native and has no CPU path" % n)
        if t.device != device:
            raise ValueError("gaussianrpg_amd.loss: " + different(n, t))


def _check(img1, img2, what=("img1", "img2")):
    for t, n in zip((img1, img2), what):
        _tensor_of(t, n, _FLOAT)
    if img1.shape != img2.shape:
        raise ValueError("gaussianrpg_amd.loss: %s and %s must have the same shape (got %s and %s)"
                         % (what[0], what[1], tuple(img1.shape), tuple(img2.shape)))
    if img1.dim() not in (3, 4):
        raise ValueError("gaussianrpg_amd.loss: images must be [C,H,W] or [B,C,H,W] (got %s)" % (tuple(img1.shape),))
    if img2.requires_grad:
        raise ValueError("gaussianrpg_amd.loss: %s requires a gradient; the fused loss differentiates only %s "
                         "(the reference's ground truth never requires one)" % (what[1], what[0]))
    _on_device(zip(what, (img1, img2)), img1.device, lambda n, t: "images on different devices")


def _as4(img):
    return (img if img.dim() == 4 else img.unsqueeze(0)).contiguous()


def _mask4(mask, img, B, C, H, W):
    """mask broadcast like torch.where(mask, img, 0) -> uint8 [1|B, 1|C, H, W] (empty: no mask)."""
    if mask is None:
        return torch.empty(0, dtype=torch.uint8, device=img.device)
    if not isinstance(mask, torch.Tensor) or mask.dtype not in _MASK[0]:   # one message for both faults
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


# ---- auxiliary terms: lidar depth, sky, object alpha (csrc/aux_loss.hip) ----

def _aux_plane(t, name, hw, mask=False):
    """None or a [H,W] / [1,H,W] device plane -> (flat contiguous tensor or None, hw)."""
    if t is None:
        return None, hw
    _tensor_of(t, name, _MASK if mask else _FLOAT)
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)):
        raise ValueError("gaussianrpg_amd.loss: %s must be [H,W] or [1,H,W] (got %s)" % (name, tuple(t.shape)))
    if hw is not None and tuple(t.shape[-2:]) != hw[:2]:
        raise ValueError("gaussianrpg_amd.loss: %s is %s, another plane is %dx%d" % (name, tuple(t.shape), *hw[:2]))
    flat = t.reshape(-1)
    if mask:
        flat = flat.contiguous().view(torch.uint8) if flat.dtype == torch.bool else flat.contiguous()
    else:
        flat = flat.contiguous()
    return flat, (int(t.shape[-2]), int(t.shape[-1]), t.device)


class _AuxLoss(torch.autograd.Function):
    """flat planes -> (stats [9]: total, lidar, sky, obj, N, k, t, c_lt, c_eq; workspace)."""

    @staticmethod
    def forward(ctx, depth, acc, acc_obj, lidar, mask, sky, bound, cfg):
        H, W, sky_scale, lams = cfg
        stats, ws = _C.aux_loss_forward(H, W, depth, acc, lidar, mask, sky, acc_obj, bound, sky_scale, *lams)
        ctx.save_for_backward(depth, acc, acc_obj, lidar, mask, sky, bound, ws)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(ws)
        return stats, ws

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats, _grad_ws):
        depth, acc, acc_obj, lidar, mask, sky, bound, ws = ctx.saved_tensors
        H, W, sky_scale, lams = ctx.cfg
        want = [bool(ctx.needs_input_grad[i]) and t.numel() > 0 for i, t in enumerate((depth, acc, acc_obj))]
        if not any(want):
            return (None,) * 8
        if grad_stats is None:
            grad_stats = torch.zeros(9, dtype=torch.float32, device=ws.device)
        gd, ga, go = _C.aux_loss_backward(H, W, depth, acc, lidar, mask, sky, acc_obj, bound, sky_scale, *lams,
                                          grad_stats.contiguous(), ws, *want)
        return (gd if want[0] else None, ga if want[1] else None, go if want[2] else None) + (None,) * 5


def _aux_run(depth, acc, lidar_depth, mask, sky_mask, sky_scale, acc_obj, obj_bound, lambda_depth_lidar,
             lambda_sky, lambda_reg):
    lam_l, lam_s, lam_r = float(lambda_depth_lidar), float(lambda_sky), float(lambda_reg)
    lidar_on = lam_l > 0 and lidar_depth is not None
    sky_on = lam_s > 0 and sky_mask is not None
    obj_on = lam_r > 0 and acc_obj is not None and obj_bound is not None
    if lidar_on and (depth is None or acc is None):
        raise ValueError("gaussianrpg_amd.loss: the lidar depth term needs depth and acc")
    if sky_on and acc is None:
        raise ValueError("gaussianrpg_amd.loss: the sky term needs acc")
    if lidar_on and lidar_depth.requires_grad:
        raise ValueError("gaussianrpg_amd.loss: lidar_depth requires a gradient; the fused loss differentiates only "
                         "depth, acc and acc_obj (the reference's lidar depth never requires one)")
    hw = None
    planes = {}
    for name, t, on, is_mask in (("depth", depth, lidar_on, False), ("acc", acc, lidar_on or sky_on, False),
                                 ("lidar_depth", lidar_depth, lidar_on, False), ("mask", mask, lidar_on, True),
                                 ("sky_mask", sky_mask, sky_on, True), ("acc_obj", acc_obj, obj_on, False),
                                 ("obj_bound", obj_bound, obj_on, True)):
        planes[name], hw = _aux_plane(t if on else None, name, hw, is_mask)
    if hw is None:
        raise ValueError("gaussianrpg_amd.loss: no auxiliary term is on (every lambda is 0 or its plane is missing)")
    _on_device([(name, t) for name, t in planes.items() if t is not None], hw[2],
               lambda name, t: "%s on %s, another plane on %s" % (name, t.device, hw[2]))
    empty = torch.empty(0, device=hw[2])
    args = [planes[k] if planes[k] is not None else empty
            for k in ("depth", "acc", "acc_obj", "lidar_depth", "mask", "sky_mask", "obj_bound")]
    stats, ws = _AuxLoss.apply(*args, (hw[0], hw[1], float(sky_scale), (lam_l, lam_s, lam_r)))
    return stats, ws, (lidar_on, sky_on, obj_on)


def aux_loss(depth, acc, *, lidar_depth=None, mask=None, sky_mask=None, sky_scale=1.0, acc_obj=None,
             obj_bound=None, lambda_depth_lidar=0.0, lambda_sky=0.0, lambda_reg=0.0):
    """lambda_depth_lidar * lidar + lambda_sky * sky + lambda_reg * obj (train.py:121-127,145-158,164-176).
    Returns (loss, terms); terms holds detached device scalars of the terms that are on."""
    stats, _, on = _aux_run(depth, acc, lidar_depth, mask, sky_mask, sky_scale, acc_obj, obj_bound,
                            lambda_depth_lidar, lambda_sky, lambda_reg)
    terms = {name: stats[i].detach() for i, name, flag in
             ((1, "lidar_depth_loss", on[0]), (2, "sky_loss", on[1]), (3, "obj_acc_loss", on[2])) if flag}
    return stats[0], terms


def lidar_depth_loss(depth, acc, lidar_depth, mask=None):
    """train.py:164-176: mean of the smallest 95 % of |depth / (acc + 1e-10) - lidar_depth| over
    (lidar_depth > 0) & mask, with the reference's zero-term guard."""
    return _aux_run(depth, acc, lidar_depth, mask, None, 1.0, None, None, 1.0, 0.0, 0.0)[0][1]


def sky_loss(acc, sky_mask, scale=1.0):
    """train.py:121-127: mean(where(sky_mask, -log(1 - a), -log(a))) * scale, a = clamp(acc, 1e-6, 1 - 1e-6)."""
    return _aux_run(None, acc, None, None, sky_mask, scale, None, None, 0.0, 1.0, 0.0)[0][2]


def obj_acc_loss(acc_obj, obj_bound):
    """train.py:145-158: mean(where(obj_bound, -(a log a + (1 - a) log(1 - a)), -log(1 - a))),
    a = clamp(acc_obj, 1e-6, 1 - 1e-6)."""
    return _aux_run(None, None, None, None, None, 1.0, acc_obj, obj_bound, 0.0, 0.0, 1.0)[0][3]


def lidar_selection(depth, acc, lidar_depth, mask=None):
    """The lidar term's selection as the device computed it, without a gradient: a dict of device tensors,
    'N', 'k', 'c_lt', 'c_eq' (exact int64) and 't' (float32, the k-th smallest error; 0 when k == 0)."""
    with torch.no_grad():
        _, ws, _ = _aux_run(depth, acc, lidar_depth, mask, None, 1.0, None, None, 1.0, 0.0, 0.0)
    counts = ws[:32].view(torch.int64)
    return {"N": counts[0], "k": counts[1], "c_lt": counts[2], "c_eq": counts[3], "t": ws[32:36].view(torch.float32)[0]}


# ---- semantic cross-entropy (csrc/semantic_loss.hip) ----

_SEMANTIC_MODES = {"logits": 0, "probabilities": 1}


class _SemanticLoss(torch.autograd.Function):
    """[S,H,W] planes, [H,W] labels -> (stats [4]: loss, n_valid, n_bad, n_correct; workspace; labels)."""

    @staticmethod
    def forward(ctx, semantic, target, mode, want_labels):
        stats, ws, labels = _C.semantic_ce_forward(semantic, target, mode, want_labels)
        ctx.save_for_backward(semantic, target, ws)
        ctx.mode = mode
        ctx.mark_non_differentiable(ws, labels)
        return stats, ws, labels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats, _grad_ws, _grad_labels):
        semantic, target, ws = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if grad_stats is None:
            grad_stats = torch.zeros(4, dtype=torch.float32, device=ws.device)
        return _C.semantic_ce_backward(semantic, target, ctx.mode, grad_stats.contiguous(), ws), None, None, None


def _semantic_run(semantic, gt_semantic, mode, ignore_index, want_labels):
    if mode not in _SEMANTIC_MODES:
        raise ValueError("gaussianrpg_amd.loss: mode must be 'logits' or 'probabilities' (got %r)" % (mode,))
    if ignore_index != -1:
        raise ValueError("gaussianrpg_amd.loss: only ignore_index == -1 is supported (got %r)" % (ignore_index,))
    _tensor_of(semantic, "semantic")
    _tensor_of(gt_semantic, "gt_semantic")
    _tensor_of(semantic, "semantic", _FLOAT)
    _tensor_of(gt_semantic, "gt_semantic", _LABEL)
    if not (semantic.dim() == 3 or (semantic.dim() == 4 and semantic.shape[0] == 1)):
        raise ValueError("gaussianrpg_amd.loss: semantic must be [S,H,W] or [1,S,H,W] (got %s)"
                         % (tuple(semantic.shape),))
    if not (gt_semantic.dim() == 2 or (gt_semantic.dim() == 3 and gt_semantic.shape[0] == 1)):
        raise ValueError("gaussianrpg_amd.loss: gt_semantic must be [H,W] or [1,H,W] (got %s)"
                         % (tuple(gt_semantic.shape),))
    if tuple(semantic.shape[-2:]) != tuple(gt_semantic.shape[-2:]):
        raise ValueError("gaussianrpg_amd.loss: semantic is %s, gt_semantic is %s"
                         % (tuple(semantic.shape), tuple(gt_semantic.shape)))
    if semantic.shape[-3] < 1 or semantic.shape[-2] < 1 or semantic.shape[-1] < 1:
        raise ValueError("gaussianrpg_amd.loss: semantic must have S >= 1 planes of at least one pixel (got %s)"
                         % (tuple(semantic.shape),))
    if gt_semantic.requires_grad:
        raise ValueError("gaussianrpg_amd.loss: gt_semantic requires a gradient; the fused loss differentiates only "
                         "semantic")
    _on_device((("semantic", semantic), ("gt_semantic", gt_semantic)), semantic.device,
               lambda n, t: "gt_semantic on %s, semantic on %s" % (t.device, semantic.device))
    sem = semantic.reshape(semantic.shape[-3:]).contiguous()
    tgt = gt_semantic.reshape(gt_semantic.shape[-2:]).contiguous()
    return _SemanticLoss.apply(sem, tgt, _SEMANTIC_MODES[mode], bool(want_labels) and sem.shape[0] <= 256)


def semantic_loss(semantic, gt_semantic, mode="logits", ignore_index=-1):
    """train.py:129-143: F.cross_entropy(semantic[None], gt_semantic, ignore_index=-1), 0 when every label is -1.
    mode='probabilities': semantic holds the raw rendered planes; log(x / (sum_c x + 1e-8) + 1e-8) is applied here."""
    return _semantic_run(semantic, gt_semantic, mode, ignore_index, False)[0][0]


def semantic_loss_stats(semantic, gt_semantic, mode="logits", ignore_index=-1):
    """The semantic term as the device computed it, without a gradient: a dict of device tensors, 'loss' (float32),
    'n_valid', 'n_bad', 'n_correct' (exact int64) and, for S <= 256, 'labels' (uint8 [H,W], the argmax channel)."""
    with torch.no_grad():
        stats, ws, labels = _semantic_run(semantic, gt_semantic, mode, ignore_index, True)
    counts = ws[:24].view(torch.int64)
    out = {"loss": stats[0], "n_valid": counts[0], "n_bad": counts[1], "n_correct": counts[2]}
    if labels.numel():
        out["labels"] = labels
    return out


# ---- mono-normal term (csrc/normal_loss.hip) ----

class _NormalLoss(torch.autograd.Function):
    """[3,H,W] planes -> (stats [4]: loss, normal_l1_loss, normal_cos_loss, n; workspace)."""

    @staticmethod
    def forward(ctx, normals, mono, wvt, mask, sky, normalize, top_rows):
        stats, ws = _C.normal_loss_forward(normals, mono, wvt, mask, sky, normalize, top_rows)
        ctx.save_for_backward(normals, mono, wvt, mask, sky, ws)
        ctx.cfg = (normalize, top_rows)
        ctx.mark_non_differentiable(ws)
        return stats, ws

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats, _grad_ws):
        normals, mono, wvt, mask, sky, ws = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        if grad_stats is None:
            grad_stats = torch.zeros(4, dtype=torch.float32, device=ws.device)
        g = _C.normal_loss_backward(normals, mono, wvt, mask, sky, *ctx.cfg, grad_stats.contiguous(), ws)
        return (g,) + (None,) * 6


def _normal_run(normals, mono_normal, world_view_transform, mask, sky_mask, normalize, top_rows):
    for t, n in ((normals, "normals"), (mono_normal, "mono_normal"), (world_view_transform, "world_view_transform")):
        _tensor_of(t, n)
    for t, n in ((normals, "normals"), (mono_normal, "mono_normal"), (world_view_transform, "world_view_transform")):
        _tensor_of(t, n, _FLOAT)
    if normals.dim() != 3 or normals.shape[0] != 3 or normals.shape[1] < 1 or normals.shape[2] < 1:
        raise ValueError("gaussianrpg_amd.loss: normals must be [3,H,W] (got %s)" % (tuple(normals.shape),))
    if mono_normal.shape != normals.shape:
        raise ValueError("gaussianrpg_amd.loss: normals is %s, mono_normal is %s"
                         % (tuple(normals.shape), tuple(mono_normal.shape)))
    if tuple(world_view_transform.shape) != (4, 4):
        raise ValueError("gaussianrpg_amd.loss: world_view_transform must be [4,4] (got %s)"
                         % (tuple(world_view_transform.shape),))
    if mono_normal.requires_grad:
        raise ValueError("gaussianrpg_amd.loss: mono_normal requires a gradient; the fused loss differentiates only "
                         "normals")
    if int(top_rows) < 0:
        raise ValueError("gaussianrpg_amd.loss: top_rows must not be negative (got %r)" % (top_rows,))
    dev = normals.device
    hw = (int(normals.shape[1]), int(normals.shape[2]), dev)
    mk, _ = _aux_plane(mask, "mask", hw, True)
    sk, _ = _aux_plane(sky_mask, "sky_mask", hw, True)
    named = [("normals", normals), ("mono_normal", mono_normal), ("world_view_transform", world_view_transform)]
    named += [(n, t) for n, t in (("mask", mk), ("sky_mask", sk)) if t is not None]
    _on_device(named, dev, lambda n, t: "%s on %s, normals on %s" % (n, t.device, dev))
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    return _NormalLoss.apply(normals.contiguous(), mono_normal.contiguous(), world_view_transform.detach(),
                             empty if mk is None else mk, empty if sk is None else sk, bool(normalize), int(top_rows))


def normal_loss(normals, mono_normal, world_view_transform, mask=None, sky_mask=None, *, normalize=True, top_rows=50):
    """train.py:206-225: normal_l1_loss + normal_cos_loss over the selected pixels, a device scalar with a gradient for
    ``normals``.  normalize=True: normals are the raw planes and x / max(|x|, 1e-12) is applied here."""
    return _normal_run(normals, mono_normal, world_view_transform, mask, sky_mask, normalize, top_rows)[0][0]


def normal_loss_terms(normals, mono_normal, world_view_transform, mask=None, sky_mask=None, *, normalize=True,
                      top_rows=50):
    """The normal term as the device computed it, without a gradient: a dict of device tensors, 'normal_l1_loss',
    'normal_cos_loss' (float32) and 'n_selected' (exact int64)."""
    with torch.no_grad():
        stats, ws = _normal_run(normals, mono_normal, world_view_transform, mask, sky_mask, normalize, top_rows)
    return {"normal_l1_loss": stats[1], "normal_cos_loss": stats[2], "n_selected": ws[:8].view(torch.int64)[0]}


# ---- scale-flatten and opacity-sparse regularisers (csrc/reg_loss.hip) ----

class _RegLoss(torch.autograd.Function):
    """scaling [N,3], opacities [N_i,1]..., radii -> (stats [4]: total, scale_flatten, opacity_sparse, n_visible;
    workspace)."""

    @staticmethod
    def forward(ctx, cfg, radii, scaling, *opacities):
        lam_s, lam_o, act_s, act_o = cfg
        stats, ws = _C.reg_loss_forward(scaling, act_s, list(opacities), act_o, radii, lam_s, lam_o)
        ctx.save_for_backward(radii, scaling, ws, *opacities)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(ws)
        return stats, ws

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stats, _grad_ws):
        radii, scaling, ws, *opacities = ctx.saved_tensors
        lam_s, lam_o, act_s, act_o = ctx.cfg
        want_s = bool(ctx.needs_input_grad[2]) and lam_s > 0
        want_o = [bool(w) and lam_o > 0 for w in ctx.needs_input_grad[3:]]
        if not (want_s or any(want_o)):
            return (None,) * (3 + len(opacities))
        if grad_stats is None:
            grad_stats = torch.zeros(4, dtype=torch.float32, device=ws.device)
        gs, go = _C.reg_loss_backward(scaling, act_s, list(opacities), act_o, radii, lam_s, lam_o,
                                      grad_stats.contiguous(), ws, want_s, want_o)
        return (None, None, gs if want_s else None) + tuple(g if w else None for g, w in zip(go, want_o))


def _reg_run(scaling, scale_activated, opacities, radii, opacity_activated, lambda_scale_flatten,
             lambda_opacity_sparse):
    lam_s, lam_o = float(lambda_scale_flatten), float(lambda_opacity_sparse)
    scale_on = lam_s > 0 and scaling is not None
    opacity_on = lam_o > 0 and opacities is not None and radii is not None
    if not (scale_on or opacity_on):
        raise ValueError("gaussianrpg_amd.loss: no regulariser is on (every lambda is 0 or its input is missing)")
    named = []
    if scale_on:
        _tensor_of(scaling, "scaling", _FLOAT)
        if scaling.dim() != 2 or scaling.shape[1] != 3:
            raise ValueError("gaussianrpg_amd.loss: scaling must be [N,3] (got %s)" % (tuple(scaling.shape),))
        named.append(("scaling", scaling))
    ops = []
    if opacity_on:
        ops = [opacities] if isinstance(opacities, torch.Tensor) else list(opacities)
        for i, t in enumerate(ops):
            _tensor_of(t, "opacities[%d]" % i, _FLOAT)
            if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)):
                raise ValueError("gaussianrpg_amd.loss: opacities[%d] must be [N,1] or [N] (got %s)"
                                 % (i, tuple(t.shape)))
            named.append(("opacities[%d]" % i, t))
        _tensor_of(radii, "radii", _RADII)
        total = sum(int(t.shape[0]) for t in ops)
        if radii.dim() != 1 or int(radii.shape[0]) != total:
            raise ValueError("gaussianrpg_amd.loss: radii is %s, the opacities hold %d Gaussians"
                             % (tuple(radii.shape), total))
        named.append(("radii", radii))
    dev = named[0][1].device
    _on_device(named, dev, lambda n, t: "%s on %s, %s on %s" % (n, t.device, named[0][0], dev))
    s = scaling.contiguous() if scale_on else torch.empty(0, device=dev)
    r = radii.contiguous() if opacity_on else torch.empty(0, dtype=torch.int32, device=dev)
    stats, _ = _RegLoss.apply((lam_s if scale_on else 0.0, lam_o if opacity_on else 0.0, bool(scale_activated),
                               bool(opacity_activated)), r, s, *[t.contiguous() for t in ops])
    return stats, (scale_on, opacity_on)


def scale_flatten_loss(scaling, activated=False):
    """gaussian_model.py:271-280: mean|s1| + mean|s2/s3 + s3/s2 - 2| over the stably sorted, clamped scales of every
    Gaussian.  scaling: the raw _scaling [N,3] (exp applied here); activated=True: get_scaling."""
    return _reg_run(scaling, activated, None, None, False, 1.0, 0.0)[0][1]


def opacity_sparse_loss(opacities, radii, activated=False):
    """train.py:197-203: mean over the visible Gaussians (radii > 0) of -(o log o + (1 - o) log(1 - o)),
    o = clamp(sigmoid(x), 1e-6, 1 - 1e-6).  opacities: one raw _opacity tensor or a list, one per model."""
    return _reg_run(None, False, opacities, radii, activated, 0.0, 1.0)[0][2]


def gaussian_reg_loss(*, scaling=None, opacities=None, radii=None, lambda_scale_flatten=0.0,
                      lambda_opacity_sparse=0.0):
    """lambda_scale_flatten * scale_flatten + lambda_opacity_sparse * opacity_sparse (train.py:190-204).
    Returns (loss, terms); terms holds detached device scalars of the terms that are on."""
    stats, on = _reg_run(scaling, False, opacities, radii, False, lambda_scale_flatten, lambda_opacity_sparse)
    terms = {name: stats[i].detach() for i, name, flag in
             ((1, "scale_flatten_loss", on[0]), (2, "opacity_sparse_loss", on[1])) if flag}
    return stats[0], terms


# ---- PSNR (csrc/metrics.hip) ----

def psnr(img1, img2, mask=None):
    """loss_utils.psnr: 20 log10(1 / sqrt(mse)), mse the mean of (img1 - img2)^2 over the selected elements; NaN for
    an empty selection, inf for identical images.  A detached device scalar: no gradient is provided."""
    for t, n in ((img1, "img1"), (img2, "img2")):
        _tensor_of(t, n)
    for t, n in ((img1, "img1"), (img2, "img2")):
        _tensor_of(t, n, _FLOAT)
    if img1.dim() != 3 or img1.shape != img2.shape or img1.numel() == 0:
        raise ValueError("gaussianrpg_amd.loss: psnr takes two [C,H,W] images of one shape (got %s and %s)"
                         % (tuple(img1.shape), tuple(img2.shape)))
    dev = img1.device
    mk, _ = _aux_plane(mask, "mask", (int(img1.shape[1]), int(img1.shape[2]), dev), True)
    _on_device([("img1", img1), ("img2", img2)] + ([("mask", mk)] if mk is not None else []), dev,
               lambda n, t: "%s on %s, img1 on %s" % (n, t.device, dev))
    with torch.no_grad():
        return _C.psnr_forward(img1.detach().contiguous(), img2.detach().contiguous(),
                               torch.empty(0, dtype=torch.uint8, device=dev) if mk is None else mk)[0]
