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

* ``densify_and_prune`` -- ``StreetGaussianModel.densify_and_prune`` (``street_gaussian_model.py:580-593``) for all
  models in one call: one classification launch, one scan, one gather pass that carries the Adam moments along, and
  the optimizer surgery of ``prune_optimizer`` / ``cat_optimizer``.  One host wait (the new sizes).

Apart from that one wait nothing here synchronises the host with the device.  There is no CPU path and no PyTorch
fallback: what the kernels do not cover is an error that names the restriction.
"""
import math
from dataclasses import dataclass
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["FusedAdam", "fused_adam_step", "densification_stats_update", "DensifyRule", "DensifyModel",
           "DensifyResult", "densify_and_prune"]


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


# the groups the reference's prune_points / densification_postfix move (gaussian_model.py:416-442)
DENSIFY_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic")
_DENSIFY_REQUIRED = ("xyz", "opacity", "scaling", "rotation")      # the rules read these; widths 3, 1, 3, 4


@dataclass
class DensifyRule:
    """The thresholds of one model's ``densify_and_prune``.  ``grad_column``: 0, or 1 for the AbsGS column of
    ``xyz_gradient_accum``.  A row with ``g = accum / denom >= max_grad`` is cloned when its largest scale is
    ``<= percent_dense * extent`` and split otherwise.  A candidate row is pruned when its opacity is below
    ``min_opacity``; with ``prune_big`` when its largest scale exceeds ``extent * percent_big_ws`` -- under the sphere
    rule (``sphere_center`` / ``sphere_radius``, the background model) unless it lies farther than two radii from the
    centre -- and under the box rule (``box_min`` / ``box_max``, the actor model) when either of its two samples
    falls outside the box.  ``prune_big`` has no default under the box rule: the reference runs the box test only
    when it prunes big points, so the caller must say which."""
    max_grad: float
    min_opacity: float
    extent: float
    percent_dense: float = 0.01
    percent_big_ws: float = 0.1
    prune_big: Optional[bool] = None
    grad_column: int = 0
    sphere_center: Optional[Sequence[float]] = None
    sphere_radius: Optional[float] = None
    box_min: Optional[Sequence[float]] = None
    box_max: Optional[Sequence[float]] = None

    @classmethod
    def background(cls, max_grad, min_opacity, prune_big_points, *, scene_radius, sphere_center, sphere_radius,
                   percent_dense=0.01, percent_big_ws=0.1, grad_abs=False):
        """``GaussianModelBkgd.densify_and_prune`` (``gaussian_model_bkgd.py:74-114``); ``max_grad`` is the caller's
        ``densify_grad_threshold_bkgd`` when the config has one, ``grad_abs`` its ``densify_grad_abs_bkgd``."""
        return cls(max_grad=max_grad, min_opacity=min_opacity, extent=scene_radius, percent_dense=percent_dense,
                   percent_big_ws=percent_big_ws, prune_big=bool(prune_big_points), grad_column=1 if grad_abs else 0,
                   sphere_center=tuple(float(v) for v in sphere_center), sphere_radius=float(sphere_radius))

    @classmethod
    def actor(cls, max_grad, min_opacity, prune_big_points, *, extent, box_min, box_max, percent_dense=0.01,
              percent_big_ws=0.1, grad_abs=False):
        """``GaussianModelActor.densify_and_prune`` (``gaussian_model_actor.py:206-263``); ``box_min`` / ``box_max``
        are its ``min_xyz`` / ``max_xyz``."""
        return cls(max_grad=max_grad, min_opacity=min_opacity, extent=extent, percent_dense=percent_dense,
                   percent_big_ws=percent_big_ws, prune_big=bool(prune_big_points), grad_column=1 if grad_abs else 0,
                   box_min=tuple(float(v) for v in box_min), box_max=tuple(float(v) for v in box_max))

    def _row(self) -> List[float]:
        """Validated, as the binding's float64 row."""
        if self.grad_column not in (0, 1):
            raise ValueError("densify_and_prune: grad_column must be 0 or 1")
        if not (isinstance(self.max_grad, (int, float)) and math.isfinite(self.max_grad) and self.max_grad > 0):
            raise ValueError("densify_and_prune: max_grad must be a finite number > 0 (with max_grad <= 0 the "
                             "reference splits its own fresh clones, whose gradient is 0)")
        has_sphere = self.sphere_center is not None or self.sphere_radius is not None
        has_box = self.box_min is not None or self.box_max is not None
        if has_sphere and (self.sphere_center is None or self.sphere_radius is None
                           or len(self.sphere_center) != 3):
            raise ValueError("densify_and_prune: the sphere rule needs sphere_center (3 values) and sphere_radius")
        if has_box and (self.box_min is None or self.box_max is None or len(self.box_min) != 3
                        or len(self.box_max) != 3):
            raise ValueError("densify_and_prune: the box rule needs box_min and box_max (3 values each)")
        if has_box and has_sphere:
            raise ValueError("densify_and_prune: a rule is plain, sphere or box, not sphere and box")
        if has_box and not isinstance(self.prune_big, bool):
            raise ValueError("densify_and_prune: a box rule must set prune_big (True or False): the reference tests "
                             "the box only when it prunes big points")
        sphere = list(self.sphere_center) + [self.sphere_radius] if has_sphere else [0.0] * 4
        box = list(self.box_min) + list(self.box_max) if has_box else [0.0] * 6
        row = [float(self.grad_column), float(self.max_grad), float(self.percent_dense), float(self.extent),
               float(self.min_opacity), float(bool(self.prune_big)), float(self.percent_big_ws), float(has_sphere)] \
            + [float(v) for v in sphere] + [float(has_box)] + [float(v) for v in box]
        if not all(math.isfinite(v) for v in row):
            raise ValueError("densify_and_prune: non-finite rule value")
        return row


@dataclass
class DensifyModel:
    """One model of a ``densify_and_prune`` call: its optimizer (a ``FusedAdam`` or a ``torch.optim.Adam`` whose
    groups carry the reference's ``name``s, one parameter each), its ``xyz_gradient_accum`` ``[P,2]`` and ``denom``
    ``[P,1]`` and its rule.  ``split_noise`` ``[P,2,3]`` / ``box_noise`` ``[P,4,2,3]`` replace the standard-normal
    draws the call would make itself."""
    optimizer: torch.optim.Optimizer
    xyz_gradient_accum: torch.Tensor
    denom: torch.Tensor
    rule: DensifyRule
    split_noise: Optional[torch.Tensor] = None
    box_noise: Optional[torch.Tensor] = None


class DensifyResult(NamedTuple):
    params: Dict[str, torch.nn.Parameter]     # {group name: new parameter}, already installed in the optimizer
    xyz_gradient_accum: torch.Tensor          # zeros [P_new,2]
    denom: torch.Tensor                       # zeros [P_new,1]
    max_radii2D: torch.Tensor                 # zeros [P_new]
    scalars: Dict[str, int]                   # the reference's scalar_dict
    src_index: torch.Tensor                   # int32 [P_new]: the source row of every new row


def _densify_tensor_check(t, what, seen, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("densify_and_prune: %s must be a tensor" % what)
    if t.dtype != torch.float32:
        raise TypeError("densify_and_prune: %s must be float32 (got %s)" % (what, t.dtype))
    seen.append((t, what))                    # the device check comes last, after every check of shape and type
    if not t.is_contiguous():
        raise RuntimeError("densify_and_prune: %s must be contiguous" % what)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("densify_and_prune: %s must be %s, got %s" % (what, list(shape), list(t.shape)))


@torch.no_grad()
def densify_and_prune(models: Sequence[DensifyModel], *, generator: Optional[torch.Generator] = None
                      ) -> List[DensifyResult]:
    """``densify_and_prune`` of every model in ``models`` (``DensifyModel`` instances, or dicts of their fields) in
    one call: clone, split, prune of the split parents and prune, in the reference's row order (surviving originals,
    clones, first children, second children), with each optimizer left as ``prune_optimizer`` / ``cat_optimizer``
    leave it: ``group['params'][0]`` is a new ``nn.Parameter``, its state entry is re-keyed with ``step`` kept,
    moments moved with surviving originals and zero for new rows; a group without state stays without.  Groups named
    other than the reference's seven are not touched.  The random draws come from ``torch.randn(...,
    generator=generator)`` on the device: ``torch.normal(0, std)`` in law, not the reference's stream.

    One host wait (the new sizes).  Not covered: ``GaussianModelSky`` (its transformed ``get_xyz``),
    ``reset_opacity``, and ``max_screen_size``, which the reference computes and ignores."""
    models = [DensifyModel(**m) if isinstance(m, dict) else m for m in models]
    seen = []                                  # every tensor of the call, for the device check
    work = []
    for k, m in enumerate(models):
        if not isinstance(m, DensifyModel):
            raise TypeError("densify_and_prune: entries must be DensifyModel instances or dicts of their fields")
        if not isinstance(m.optimizer, (FusedAdam, torch.optim.Adam)):
            raise TypeError("densify_and_prune: expected a FusedAdam or torch.optim.Adam, got %s"
                            % type(m.optimizer).__name__)
        if not isinstance(m.rule, DensifyRule):
            raise TypeError("densify_and_prune: rule must be a DensifyRule")
        row = m.rule._row()
        groups = {}
        for group in m.optimizer.param_groups:
            name = group.get("name")
            if name in DENSIFY_GROUPS:
                if name in groups:
                    raise ValueError("densify_and_prune: model %d has two groups named '%s'" % (k, name))
                if len(group["params"]) != 1:
                    raise ValueError("densify_and_prune: group '%s' must hold exactly one parameter" % name)
                groups[name] = group
        for name in _DENSIFY_REQUIRED:
            if name not in groups:
                raise KeyError("densify_and_prune: model %d's optimizer has no group named '%s'" % (k, name))
        if len(groups) > 8:
            raise ValueError("densify_and_prune: at most 8 tensors per model")
        names = [n for n in DENSIFY_GROUPS if n in groups]
        if not isinstance(m.xyz_gradient_accum, torch.Tensor) or m.xyz_gradient_accum.dim() != 2:
            raise ValueError("densify_and_prune: xyz_gradient_accum must be a [P,2] tensor")
        P = m.xyz_gradient_accum.shape[0]
        _densify_tensor_check(m.xyz_gradient_accum, "xyz_gradient_accum", seen, (P, 2))
        if not isinstance(m.denom, torch.Tensor) or m.denom.shape[:1] != (P,) or m.denom.numel() != P:
            raise ValueError("densify_and_prune: denom must be [P,1] with xyz_gradient_accum's P")
        _densify_tensor_check(m.denom, "denom", seen)
        params, exp_avgs, exp_avg_sqs, has_state = [], [], [], []
        for name in names:
            p = groups[name]["params"][0]
            if p.dim() < 1 or p.shape[0] != P:
                raise ValueError("densify_and_prune: '%s' has %s rows, xyz_gradient_accum %d: every tensor of a model "
                                 "must have the same P" % (name, p.shape[0] if p.dim() else "no", P))
            _densify_tensor_check(p, "'%s'" % name, seen)
            state = m.optimizer.state.get(p, None)
            live = state is not None and "exp_avg" in state
            if live:
                for key in ("exp_avg", "exp_avg_sq"):
                    _densify_tensor_check(state[key], "state['%s'] of '%s'" % (key, name), seen, p.shape)
            params.append(p.detach())
            exp_avgs.append(state["exp_avg"] if live else p.detach())
            exp_avg_sqs.append(state["exp_avg_sq"] if live else p.detach())
            has_state.append(1 if live else 0)
        for name, width in zip(_DENSIFY_REQUIRED, (3, 1, 3, 4)):
            p = groups[name]["params"][0]
            if p.numel() != P * width:
                raise ValueError("densify_and_prune: '%s' must have %d values per row" % (name, width))
        for noise, what, shape in ((m.split_noise, "split_noise", (P, 2, 3)), (m.box_noise, "box_noise", (P, 4, 2, 3))):
            if noise is not None:
                _densify_tensor_check(noise, what, seen, shape)
        special = [names.index(n) for n in _DENSIFY_REQUIRED]
        work.append((m, groups, names, P, params, exp_avgs, exp_avg_sqs, has_state, special, row))
    if not work:
        return []
    device = seen[0][0].device
    for t, what in seen:
        if not t.is_cuda:
            raise RuntimeError("densify_and_prune: %s must live on a ROCm/HIP device (no CPU path)" % what)
        if t.device != device:
            raise RuntimeError("densify_and_prune: %s is on %s, the call's other tensors on %s"
                               % (what, t.device, device))
    ext = _C()
    split_noise, box_noise = [], []
    for m, groups, names, P, *_rest, row in work:
        split_noise.append(m.split_noise if m.split_noise is not None else
                           torch.randn((P, 2, 3), generator=generator, device=device, dtype=torch.float32))
        if row[12] and row[5]:          # box rule, pruning big points
            box_noise.append(m.box_noise if m.box_noise is not None else
                             torch.randn((P, 4, 2, 3), generator=generator, device=device, dtype=torch.float32))
        else:
            box_noise.append(torch.empty(0, device=device, dtype=torch.float32))
    outs, counts = ext.densify_and_prune(
        [w[4] for w in work], [w[5] for w in work], [w[6] for w in work], [w[7] for w in work],
        [w[0].xyz_gradient_accum for w in work], [w[0].denom.reshape(-1) for w in work], split_noise, box_noise,
        torch.tensor([w[8] for w in work], dtype=torch.int64).reshape(-1, 4),
        torch.tensor([w[9] for w in work], dtype=torch.float64).reshape(-1, 19))
    results = []
    for (m, groups, names, P, _p, _m, _v, has_state, _s, row), out, cnt in zip(work, outs, counts.tolist()):
        new_p, new_m, new_v, accum, denom, max_radii, src_index = out
        installed = {}
        opt = m.optimizer
        for t, name in enumerate(names):
            group = groups[name]
            old = group["params"][0]
            stored = opt.state.get(old, None)
            param = torch.nn.Parameter(new_p[t].requires_grad_(True))
            if stored is not None:
                if has_state[t]:
                    stored["exp_avg"] = new_m[t]
                    stored["exp_avg_sq"] = new_v[t]
                del opt.state[old]
                group["params"][0] = param
                if len(stored) != 0:
                    opt.state[param] = stored
            else:
                group["params"][0] = param
            installed[name] = param
        scalars = {"points_total": P, "points_clone": cnt[5], "points_split": cnt[6],
                   "points_below_min_opacity": cnt[7], "points_big_ws": cnt[8], "points_pruned": cnt[9]}
        results.append(DensifyResult(installed, accum, denom, max_radii, scalars, src_index))
    return results
