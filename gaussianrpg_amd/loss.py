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
"""
import torch

from .rasterizer import _C

__all__ = ["ssim", "l1_loss", "l1_ssim_loss", "aux_loss", "lidar_depth_loss", "sky_loss", "obj_acc_loss",
           "lidar_selection", "semantic_loss", "semantic_loss_stats"]


_FLOAT = ((torch.float32,), "float32")
_MASK = ((torch.bool, torch.uint8), "a bool (or uint8) tensor")
_LABEL = ((torch.int64, torch.int32), "int64 or int32")


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
