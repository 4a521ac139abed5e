"""The tail of the reference's training iteration on the device: ``optimizer.step()`` of every model and the
densification statistics, each in one HIP launch (csrc/optim.hip).

* ``FusedAdam`` -- ``torch.optim.Adam`` (``amsgrad=False, weight_decay=0, maximize=False``) as a
  ``torch.optim.Optimizer`` whose ``state`` has Adam's layout (``state[p] = {'step', 'exp_avg', 'exp_avg_sq'}``), so
  the reference's optimizer surgery (``gaussian_model.py:344-408``: a group's parameter replaced, its moments
  sliced / concatenated / zeroed) and ``state_dict()`` / ``load_state_dict()`` interchange with ``torch.optim.Adam``
  work unchanged.  ``step()`` is one launch over all tensors of all groups.
* ``fused_adam_step(optimizers)`` -- the step of several ``FusedAdam`` instances (the reference keeps one per model,
  ``street_gaussian_model.py:536-541``) in one launch.
* ``densification_stats_update`` -- ``set_max_radii2D`` + ``add_densification_stats``
  (``street_gaussian_model.py:555-578``) for all models of a composed frame in one launch, without the five
  boolean-mask gathers / scatters (a ``nonzero`` host synchronisation each) per model.

Nothing here synchronises the host with the device.  There is no CPU path and no PyTorch fallback: what the kernels
do not cover is an error that names the restriction.
"""
import math
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

__all__ = ["FusedAdam", "fused_adam_step", "densification_stats_update"]


def _C():
    from .rasterizer import _C as ext     # loads the native code; fails loudly when it has not been built
    return ext


def _check_group(group):
    if group.get("weight_decay", 0) != 0:
        raise ValueError("FusedAdam: weight_decay != 0 is not supported (the fused step has no decay term)")
    if group.get("amsgrad", False):
        raise ValueError("FusedAdam: amsgrad=True is not supported")
    if group.get("maximize", False):
        raise ValueError("FusedAdam: maximize=True is not supported")
    if group.get("differentiable", False):
        raise ValueError("FusedAdam: differentiable=True is not supported")
    beta1, beta2 = group["betas"]
    if not 0.0 <= group["lr"]:
        raise ValueError("FusedAdam: invalid learning rate: %r" % (group["lr"],))
    if not 0.0 <= group["eps"]:
        raise ValueError("FusedAdam: invalid epsilon value: %r" % (group["eps"],))
    if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
        raise ValueError("FusedAdam: invalid betas: %r" % (group["betas"],))


def _check_dtype(p):
    if p.dtype != torch.float32:
        raise TypeError("FusedAdam: parameters must be float32 (got %s); other precisions are not supported" % p.dtype)


class FusedAdam(torch.optim.Optimizer):
    """``FusedAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)``; ``params`` as for ``torch.optim.Adam``, the
    reference's list of named groups with a per-group ``lr`` included (``gaussian_model.py:292-304``).  ``lr`` is
    read from the group at every step, like torch does (learning-rate schedules write it there).  A parameter whose
    ``.grad`` is ``None`` is skipped: its moments do not decay and its step count does not advance.

    The groups carry every key of ``torch.optim.Adam``'s (so a state dict loads either way); ``weight_decay != 0``,
    ``amsgrad``, ``maximize``, non-float32 parameters (checked here and at every step) and parameters that are not
    on a ROCm/HIP device (checked at the step: a model may be built on the host and moved) are errors."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False):
        if isinstance(lr, torch.Tensor):
            raise TypeError("FusedAdam: lr must be a Python number (a tensor lr would need a host synchronisation)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=False)
        super().__init__(params, defaults)
        for group in self.param_groups:
            _check_group(group)
            for p in group["params"]:
                _check_dtype(p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        fused_adam_step([self])
        return loss


def _collect(optimizers) -> List[Tuple[torch.Tensor, torch.Tensor, dict, dict]]:
    """(param, grad, state, group) of every parameter that steps, validated; nothing is modified."""
    work = []
    for opt in optimizers:
        if not isinstance(opt, FusedAdam):
            raise TypeError("fused_adam_step: expected FusedAdam instances, got %s" % type(opt).__name__)
        for group in opt.param_groups:
            _check_group(group)
            if isinstance(group["lr"], torch.Tensor):
                raise TypeError("FusedAdam: lr must be a Python number (a tensor lr would need a host synchronisation)")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                _check_dtype(p)
                if not p.is_cuda:
                    raise RuntimeError("FusedAdam: parameters must live on a ROCm/HIP device (no CPU path)")
                if g.is_sparse:
                    raise RuntimeError("FusedAdam: sparse gradients are not supported")
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise RuntimeError("FusedAdam: a gradient must have its parameter's dtype, device and shape")
                if not p.is_contiguous():
                    raise RuntimeError("FusedAdam: parameters must be contiguous")
                state = opt.state[p]
                if len(state) != 0:
                    for k in ("exp_avg", "exp_avg_sq"):
                        m = state[k]
                        if (m.dtype != torch.float32 or m.device != p.device or m.shape != p.shape
                                or not m.is_contiguous()):
                            raise RuntimeError("FusedAdam: state['%s'] must be a contiguous float32 tensor of its "
                                               "parameter's shape on its device" % k)
                work.append((p, g, state, group))
    return work


@torch.no_grad()
def fused_adam_step(optimizers: Iterable[FusedAdam]) -> None:
    """The step of all ``optimizers`` (``FusedAdam`` instances) in ONE launch per device: what
    ``StreetGaussianModel.update_optimizer`` does model by model.  Equal, bit for bit, to calling ``step()`` on each.
    Gradients are left in place (call ``zero_grad`` as before)."""
    work = _collect(list(optimizers))
    by_dev = {}
    for p, g, state, group in work:
        if len(state) == 0:
            # torch.optim.Adam's layout; `step` is a CPU scalar, as on Adam's default (non-capturable) path
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step_t = state["step"]
        if not isinstance(step_t, torch.Tensor):
            step_t = state["step"] = torch.tensor(float(step_t), dtype=torch.float32)
        elif step_t.device.type != "cpu":       # a state dict of a capturable / fused Adam: one copy, once
            step_t = state["step"] = step_t.cpu()
        step_t += 1
        t = step_t.item()
        beta1, beta2 = group["betas"]
        # in double, from this parameter's own step count, as torch's non-capturable path; rounded once below
        step_size = group["lr"] / (1.0 - beta1 ** t)
        bc2_sqrt = math.sqrt(1.0 - beta2 ** t)
        lists = by_dev.setdefault(p.device, ([], [], [], [], []))
        lists[0].append(p)
        lists[1].append(g if g.is_contiguous() else g.contiguous())
        lists[2].append(state["exp_avg"])
        lists[3].append(state["exp_avg_sq"])
        lists[4].append((step_size, bc2_sqrt, beta2, 1.0 - beta1, 1.0 - beta2, group["eps"]))
    ext = _C() if by_dev else None
    for params, grads, exp_avgs, exp_avg_sqs, coef in by_dev.values():
        coef_t = torch.from_numpy(np.asarray(coef, dtype=np.float64).astype(np.float32).reshape(-1, 6))
        ext.adam_step(params, grads, exp_avgs, exp_avg_sqs, coef_t)


@torch.no_grad()
def densification_stats_update(viewspace_grad: torch.Tensor, radii: torch.Tensor,
                               ranges: Sequence[Tuple[int, int]], accum: Sequence[torch.Tensor],
                               denom: Sequence[torch.Tensor], max_radii2D: Sequence[torch.Tensor]) -> None:
    """``set_max_radii2D(radii, radii > 0)`` + ``add_densification_stats(viewspace_points, radii > 0)`` of the
    reference for all models of a composed frame, in place, in one launch.

    ``viewspace_grad``: ``viewspace_points.grad``, float32 ``[P,3]``; ``radii``: the rasterizer's int32 ``[P]``.
    ``ranges[k] = (start, end)`` is model k's slice of the composed frame as a HALF-OPEN range, ascending and
    disjoint -- the reference's ``graph_gaussian_range`` holds the inclusive ``[start, end - 1]``, so pass
    ``(start, end + 1)`` of its entries.  ``accum[k]`` ``[n,2]`` (``xyz_gradient_accum``), ``denom[k]`` ``[n,1]``
    and ``max_radii2D[k]`` ``[n]`` are model k's float32 tensors, ``n = end - start``.  For every Gaussian with
    ``radii > 0``: ``accum[:,0] += |grad.xy|``, ``accum[:,1] += |grad.z|``, ``denom += 1``,
    ``max_radii2D = max(max_radii2D, radii)``; rows of the others are not touched."""
    if not (len(ranges) == len(accum) == len(denom) == len(max_radii2D)):
        raise ValueError("densification_stats_update: one range, accum, denom and max_radii2D per model")
    if not isinstance(viewspace_grad, torch.Tensor):
        raise TypeError("densification_stats_update: viewspace_grad must be a tensor (viewspace_points.grad)")
    if not viewspace_grad.is_cuda or not radii.is_cuda:
        raise RuntimeError("densification_stats_update: tensors must live on a ROCm/HIP device (no CPU path)")
    if viewspace_grad.dtype != torch.float32:
        raise TypeError("densification_stats_update: viewspace_grad must be float32")
    if radii.dtype != torch.int32:
        raise TypeError("densification_stats_update: radii must be int32 (the rasterizer's radii)")
    if viewspace_grad.dim() != 2 or viewspace_grad.shape[1] != 3 or radii.shape != viewspace_grad.shape[:1]:
        raise ValueError("densification_stats_update: viewspace_grad must be [P,3] and radii [P]")
    for a, d, m in zip(accum, denom, max_radii2D):
        for t in (a, d, m):
            if t.dtype != torch.float32:
                raise TypeError("densification_stats_update: accum, denom and max_radii2D must be float32")
    rng = torch.from_numpy(np.asarray([(int(s), int(e)) for s, e in ranges], dtype=np.int64).reshape(-1, 2))
    _C().densify_stats(viewspace_grad.contiguous(), radii.contiguous(), rng, list(accum), list(denom),
                       list(max_radii2D))
