"""Fused scene-graph composition in front of the rasterizer (additive API).

Every frame the reference's ``StreetGaussianModel`` rebuilds the op's flat inputs in PyTorch
(lib/models/street_gaussian_model.py:296-453): per model ``exp`` / ``sigmoid`` / ``normalize`` of the
raw parameters (gaussian_model.py:224-251), per visible actor a rigid transform of the means and a
quaternion product for the rotations with the tracked pose (street_gaussian_model.py:318-365), an
inverse DFT of the actor's Fourier colour coefficients (gaussian_model_actor.py:73-82) and a
``torch.cat`` over the models -- about twenty small kernels and two extra passes over the op's whole
input.  ``ComposedRasterizer`` hands the models' RAW parameter tensors and the per-frame poses to
``_C.rasterize_gaussians_composed`` instead; the arithmetic happens inside the HIP preprocess and the
concatenated tensors are never materialised.

    models = [ModelParams(...background...), ModelParams(...actor 1...), ...]
    poses  = [None, ActorPose(obj_rot, obj_trans, fourier_time), ...]
    color, radii, depth, alpha = ComposedRasterizer(raster_settings)(models, poses)

``poses`` may also be a ``PoseRows`` -- the frame's poses as two device tensors, what ``tracks.PoseBatch.frame``
makes of the tracklets in one launch -- wherever the list form is accepted, or a ``PoseTable`` -- the pose batch's own
device rows and one row index per model, what ``tracks.PoseBatch.rows`` returns without a launch: the poses then never
visit the host (C ABI ``grpg_bind_device_poses``), and the frame is bit for bit the one the other two forms give.

Evaluation (``torch.no_grad()`` or nothing requires grad): forward only.  TRAINING (round 3): when
any raw parameter tensor -- or an actor's ``obj_rot`` / ``obj_trans`` given as a tensor -- requires
grad, the call goes through an autograd function whose backward (C ABI ``grpg_backward_composed``)
returns the gradients with respect to the RAW parameters (``_xyz``, ``_scaling``, ``_rotation``,
``_opacity``, ``_features_dc``, ``_features_rest``) and the poses: the chain rule through exp /
sigmoid / normalize, the Fourier DC sum, the rigid transform and the quaternion product runs inside
the preprocess backward kernel.  ``means2D`` (zeros ``[P,3]`` requiring grad, as
street_gaussian_renderer.py:157-162 creates it) receives the densification statistic.  The flip
augmentation of rigid actors (street_gaussian_model.py:286-293) is ``ModelParams.flip``.  Feature planes --
the semantic concatenation (:420-435) and the normals (:463-484) -- ride through
``ComposedRasterizer.forward_features``; ``forward`` itself renders none.  Not fused (stay in the caller's
PyTorch): pose-correction modules -- a corrected pose is simply an ``obj_rot`` / ``obj_trans`` tensor with a
graph behind it.
"""
import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .rasterizer import GaussianRasterizationSettings, _C, _frame_result, _layers_result, _or_empty, _white

MAX_FOURIER = 8     # GRPG_MAX_FOURIER


class ModelParams(NamedTuple):
    """Raw (pre-activation) parameters of one Gaussian model, as the reference stores them
    (gaussian_model.py:36-47): ``_xyz [N,3]``, ``_scaling [N,3]`` (log), ``_rotation [N,4]``,
    ``_opacity [N,1]`` (logit), ``_features_dc [N,F,3]`` (F = fourier_dim, 1 for the background),
    ``_features_rest [N,M-1,3]``.  ``flip`` (optional, bool ``[N]``): this iteration's flip mask of a
    rigid actor -- the training symmetry prior, ``torch.rand_like(xyz[:, 0]) < flip_prob``
    (street_gaussian_model.py:286-293); flipped Gaussians have their local y mirrored and their local
    rotation pre-multiplied by the quaternion of diag(-1, 1, -1) (:57-61, :332, :360).  The mask of a static model
    (pose ``None``) is ignored, in the forward and in the backward: the reference mirrors posed actors only."""
    xyz: torch.Tensor
    scaling: torch.Tensor
    rotation: torch.Tensor
    opacity: torch.Tensor
    features_dc: torch.Tensor
    features_rest: torch.Tensor
    flip: Optional[torch.Tensor] = None


class ActorPose(NamedTuple):
    """Pose of one actor for one frame: ``obj_rot`` (w,x,y,z) and ``obj_trans`` in world space, ego
    pose already applied (street_gaussian_model.py:268-273); ``fourier_time`` =
    fourier_scale * (frame - start_frame) / (end_frame - start_frame) (gaussian_model_actor.py:74-75).
    ``obj_rot`` / ``obj_trans`` are sequences of floats or tensors ([4] / [3]); tensors that require
    grad (optimised tracking, street_gaussian_model.py:319-320) receive gradients in training."""
    obj_rot: Sequence[float]
    obj_trans: Sequence[float]
    fourier_time: float = 0.0


class PoseRows(NamedTuple):
    """The poses of one frame as two tensors instead of a list of ``ActorPose``: ``rot [n,4]`` (w,x,y,z) and ``trans
    [n,3]``, one row per model, on the device, ego pose applied -- what ``tracks.PoseBatch.frame`` returns.  ``posed``:
    one flag per model, False = a static model (its row is ignored, like a ``None`` in the list form);
    ``fourier_time``: one value per model.  Every entry point that takes the list form takes this one; the rows go to
    the host in one copy and keep their graph in training, with no per-actor Python."""
    rot: torch.Tensor
    trans: torch.Tensor
    posed: Sequence[bool]
    fourier_time: Sequence[float]


class PoseTable(NamedTuple):
    """The poses of one frame left where ``TrackedActorPoses.poses`` wrote them: ``rot [A,4]`` (w,x,y,z) and ``trans
    [A,3]`` on the device, one row per ACTOR of the track table (``PoseBatch.rot[t]`` / ``.trans[t]``, views), and
    ``row``: per MODEL of the frame the row it takes its pose from, -1 for a model that takes none from the device.
    ``posed`` / ``fourier_time``: one entry per model, as in ``PoseRows``.  ``host_pose`` (optional): per model None, or
    ``(obj_rot, obj_trans)`` as floats for a posed model whose ``row`` is -1 -- an actor the host poses.  What
    ``tracks.PoseBatch.rows`` returns; every entry point that takes the list form takes this one.  Nothing is copied to
    the host: the library's segment table takes the rows from device memory behind its own upload, on the call's stream
    (``grpg_bind_device_poses``), and in training the pose gradient comes back as dense ``[A,4]`` / ``[A,3]`` tensors,
    zero for the actors the frame does not show."""
    rot: torch.Tensor
    trans: torch.Tensor
    row: Sequence[int]
    posed: Sequence[bool]
    fourier_time: Sequence[float]
    host_pose: Optional[Sequence] = None


def _posed_flags(poses):
    """one flag per model: the model has a pose (an actor)"""
    if isinstance(poses, (PoseRows, PoseTable)):
        return [bool(f) for f in poses.posed]
    return [p is not None for p in poses]


def _pack_table(n_models, poses: PoseTable):
    """The pose argument of a PoseTable, (pose_t [n,8] on the host, rot, trans, row int32 [n] on the host) -- what the
    binding's `poses` takes in place of pose_t alone -- and the Fourier times.  pose_t holds the posed flag and zeros
    (the host poses of `host_pose` where given); the device tensors are handed on as they are and never read."""
    n = len(poses.posed)
    if n != n_models or len(poses.fourier_time) != n or len(poses.row) != n:
        raise ValueError("one row index, posed flag and fourier_time per model")
    if poses.rot.dim() != 2 or poses.rot.shape[1] != 4 or tuple(poses.trans.shape) != (poses.rot.shape[0], 3):
        raise ValueError("pose table must be rot [A,4] and trans [A,3], got %s and %s"
                         % (tuple(poses.rot.shape), tuple(poses.trans.shape)))
    if poses.rot.dtype != torch.float32 or poses.trans.dtype != torch.float32:
        raise TypeError("pose table must be float32, got %s and %s" % (poses.rot.dtype, poses.trans.dtype))
    A = int(poses.rot.shape[0])
    rows = []
    for i in range(n):
        r, f = int(poses.row[i]), bool(poses.posed[i])
        if r < -1 or r >= A:
            raise ValueError("model %d: row %d is neither -1 nor one of the table's %d rows" % (i, r, A))
        row = list(_ZERO_ROW)
        if f:
            row[0] = 1.0
            if r < 0:
                hp = None if poses.host_pose is None else poses.host_pose[i]
                if hp is None:
                    raise ValueError("model %d is posed, but has neither a table row nor a host pose" % i)
                row[1:5] = [float(x) for x in hp[0]]
                row[5:8] = [float(x) for x in hp[1]]
        elif r >= 0:
            raise ValueError("model %d is static, but names row %d of the pose table" % (i, r))
        rows.append(row)
    pose_t = torch.from_numpy(np.asarray(rows, dtype=np.float32).reshape(n, 8))
    row_t = torch.from_numpy(np.asarray([int(r) for r in poses.row], dtype=np.int32).reshape(n))
    times = [float(t) if f else 0.0 for t, f in zip(poses.fourier_time, poses.posed)]
    return (pose_t, poses.rot.detach().contiguous(), poses.trans.detach().contiguous(), row_t), times


def _scatter_pose_grads(pose_arg, g_poses, want_rot, want_trans):
    """dL_dposes [n,8] of a PoseTable frame -> dense gradients of the table, ([A,4], [A,3]): zero for the actors the
    frame does not show, summed for an actor it shows twice.  One memset and one index add per tensor."""
    _, rot, _, row_t = pose_arg
    sel = torch.nonzero(row_t >= 0).view(-1)          # host arithmetic on the host index list
    dev = g_poses.device
    src = g_poses.index_select(0, sel.to(dev, non_blocking=True))
    to = row_t[sel].long().to(dev, non_blocking=True)
    A = rot.shape[0]
    g_rot = g_poses.new_zeros(A, 4).index_add_(0, to, src[:, 0:4]) if want_rot else None
    g_trans = g_poses.new_zeros(A, 3).index_add_(0, to, src[:, 4:7]) if want_trans else None
    return g_rot, g_trans


def _pack_rows(n_models, poses: PoseRows):
    """pose_t [n,8] of a PoseRows: ONE host copy, made from the two tensors directly"""
    n = len(poses.posed)
    if n != n_models or len(poses.fourier_time) != n:
        raise ValueError("one pose row, posed flag and fourier_time per model")
    if tuple(poses.rot.shape) != (n, 4) or tuple(poses.trans.shape) != (n, 3):
        raise ValueError("pose rows must be rot [%d,4] and trans [%d,3], got %s and %s"
                         % (n, n, tuple(poses.rot.shape), tuple(poses.trans.shape)))
    flag = torch.tensor([bool(f) for f in poses.posed]).view(n, 1)
    host = torch.cat([poses.rot.detach().float(), poses.trans.detach().float()], 1).cpu()
    pose_t = torch.cat([flag.float(), host], 1).masked_fill_(~flag, 0.0)   # a static model's row is zero, like _ZERO_ROW
    times = [float(t) if f else 0.0 for t, f in zip(poses.fourier_time, poses.posed)]
    return pose_t, times


def idft_weights(time: float, dim: int) -> List[float]:
    """IDFT(time, dim) of lib/utils/sh_utils.py:120-130: even k -> cos(pi t k), odd k -> sin(pi t (k+1)),
    evaluated in float32 like the reference (pinned by tests/golden/ref_idft.npz)."""
    t = torch.tensor(float(time)).view(-1, 1).float()
    idft = torch.zeros(1, dim)
    indices = torch.arange(dim)
    even, odd = indices[::2], indices[1::2]
    idft[:, even] = torch.cos(torch.pi * t * even)
    idft[:, odd] = torch.sin(torch.pi * t * (odd + 1))
    return [float(v) for v in idft[0]]


_ZERO_ROW = [0.0] * 8
_NO_FLIP = torch.empty(0, dtype=torch.bool)
_IDFT_CONST = {}   # dims tuple -> (multiplier [1, MAX_FOURIER] float32, takes-cos mask, drop mask [n, MAX_FOURIER])


def _idft_rows(times: Sequence[float], dims: Sequence[int]) -> torch.Tensor:
    """IDFT(time_i, dim_i) for all models at once, [n, MAX_FOURIER] float32 (zero beyond dim_i): the
    reference's formula (sh_utils.py:120-130) applied to a column of times -- the same float32
    elementwise operations in the same order ((pi t) k, then cos / sin), hence the same bits as one call per
    model (tests/test_compose.py pins both against the reference-derived fixture), at a fraction of the host time:
    a per-actor call costs 50 us of Python / dispatcher overhead, and everything that depends on the models only
    (the multipliers as float32 -- exact small integers, what the reference's int64 -> float32 promotion yields --,
    which columns take the cosine, which columns a model does not use) is built once per set of Fourier dimensions.
    This runs once per FRAME in the simulator's loop, in front of the frame's first launch (the GPU waits for it):
    seven small tensor operations (round 6: 60 -> 25 -> 17 us)."""
    key = dims if isinstance(dims, tuple) else tuple(int(d) for d in dims)
    c = _IDFT_CONST.get(key)
    if c is None:
        indices = torch.arange(MAX_FOURIER)
        is_even = (indices % 2 == 0).view(1, -1)
        mult = torch.where(is_even, indices.view(1, -1), indices.view(1, -1) + 1).float()   # k (even k), k + 1 (odd k)
        keep = indices.view(1, -1) < torch.tensor(key).view(-1, 1)
        c = _IDFT_CONST[key] = (mult, is_even.expand(len(key), -1).contiguous(), ~keep)
    mult, takes_cos, drop = c
    t = torch.from_numpy(np.asarray(times, dtype=np.float32)).view(-1, 1)
    arg = (torch.pi * t) * mult                     # (pi t) k in float32, like torch.pi * t * even / (odd + 1)
    return torch.where(takes_cos, torch.cos(arg), torch.sin(arg)).masked_fill_(drop, 0.0)


def _model_lists(models: Sequence[ModelParams]):
    dims = []
    for m in models:
        F = int(m.features_dc.shape[1])
        if F > MAX_FOURIER:
            raise ValueError("fourier_dim %d > %d" % (F, MAX_FOURIER))
        dims.append(F)
    lists = [[m[f] for m in models] for f in range(6)]
    lists.append([_NO_FLIP if m.flip is None else m.flip for m in models])
    return lists, tuple(dims)


def _pack(models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]]):
    if isinstance(poses, PoseRows):
        lists, dims = _model_lists(models)
        pose_t, times = _pack_rows(len(models), poses)
        return lists, pose_t, _idft_rows(times, dims)
    if isinstance(poses, PoseTable):   # pose_t: the tuple the binding takes in its place, device poses included
        lists, dims = _model_lists(models)
        pose_t, times = _pack_table(len(models), poses)
        return lists, pose_t, _idft_rows(times, dims)
    if len(models) != len(poses):
        raise ValueError("one pose entry (None for a static model) per model")
    lists, dims = _model_lists(models)
    rows, times = [], []
    tens, slots = [], []   # tensor-valued pose parts and where they go: ONE host copy for all of them
    for i, p in enumerate(poses):
        if p is None:      # a static model has fourier_dim 1: weight cos(0) = 1
            rows.append(_ZERO_ROW)
            times.append(0.0)
            continue
        row = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        for off, v, n in ((1, p.obj_rot, 4), (5, p.obj_trans, 3)):
            if isinstance(v, torch.Tensor):
                if v.numel() != n:
                    raise ValueError("pose component of %d elements, expected %d" % (v.numel(), n))
                tens.append(v.detach().reshape(-1).float())
                slots.append((i, off, n))
            else:
                if len(v) != n:
                    raise ValueError("pose component of %d elements, expected %d" % (len(v), n))
                row[off:off + n] = [float(x) for x in v]
        rows.append(row)
        times.append(p.fourier_time)
    if tens:
        # tracked poses usually live on the GPU: a .cpu() per actor would be a device sync per actor and
        # frame; stack them first (one small kernel) and copy once
        if len({t.device for t in tens}) == 1:
            flat_vals = torch.cat(tens).cpu().tolist()
        else:
            flat_vals = torch.cat([t.cpu() for t in tens]).tolist()
        k = 0
        for i, off, n in slots:
            rows[i][off:off + n] = flat_vals[k:k + n]
            k += n
    pose_t = torch.from_numpy(np.asarray(rows, dtype=np.float32))     # [n, 8] (float64 -> float32 like torch.tensor)
    idft_t = _idft_rows(times, dims)
    return lists, pose_t, idft_t


def _object_flags(object_models):
    """uint8 [n] on the host, 1 = the model belongs to the object layer; empty: every posed model (actor) does."""
    if object_models is None:
        return torch.empty(0, dtype=torch.uint8)
    return torch.tensor([1 if f else 0 for f in object_models], dtype=torch.uint8)


def compose(models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]]):
    """The composition alone: (means3D [P,3], scales [P,3], rotations [P,4], opacity [P,1],
    shs [P,M,3]) -- what get_xyz / get_scaling / get_rotation / get_opacity / get_features of the
    reference return -- computed by the same HIP code the fused rasterizer uses."""
    lists, pose_t, idft_t = _pack(models, poses)
    return _C.compose(*lists, pose_t, idft_t)


def _pose_tensors(poses):
    if isinstance(poses, (PoseRows, PoseTable)):
        return [poses.rot, poses.trans]
    return [t for p in poses if p is not None for t in (p.obj_rot, p.obj_trans) if isinstance(t, torch.Tensor)]


def _pose_graph(poses, pose_tensors):
    """poses as [n,4] / [n,3] tensors that keep their graph (rows of static models: constants)"""
    if isinstance(poses, PoseRows):   # as they are: a static model's row receives a zero gradient
        return poses.rot.float(), poses.trans.float()
    if isinstance(poses, PoseTable):  # the table itself, [A,4] / [A,3]: the backward scatters into its shape
        return poses.rot, poses.trans
    if not pose_tensors:
        return None, None
    one = torch.tensor([1.0, 0.0, 0.0, 0.0])
    zero3 = torch.zeros(3)
    dev = pose_tensors[0].device
    as_t = lambda v, d: v.to(dev).float() if isinstance(v, torch.Tensor) else \
        torch.tensor([float(x) for x in v], device=dev)   # noqa: E731
    pose_rot = torch.stack([one.to(dev) if p is None else as_t(p.obj_rot, dev) for p in poses])
    pose_trans = torch.stack([zero3.to(dev) if p is None else as_t(p.obj_trans, dev) for p in poses])
    return pose_rot, pose_trans


_NO_SEMANTIC = torch.empty(0)


def _split(flat, nm):
    """The head of a Function's flat tensor arguments -> the six per-field lists of nm tensors (_model_lists' order)."""
    return [list(flat[f * nm:(f + 1) * nm]) for f in range(6)]


def _semantic_list(models, semantics):
    """One [N_i,S] float32 device tensor per model (None -> an empty tensor: zeros); S.  No fallback: a CPU
    tensor, another dtype or disagreeing S is an error."""
    if semantics is None:
        return [], 0
    if len(semantics) != len(models):
        raise ValueError("one semantic tensor (or None) per model")
    out, S = [], None
    for i, (m, t) in enumerate(zip(models, semantics)):
        if t is None:
            out.append(_NO_SEMANTIC)
            continue
        if not t.is_cuda:
            raise RuntimeError("gaussianrpg_amd: semantics of model %d must live on the device: there is no CPU path" % i)
        if t.dtype != torch.float32:
            raise TypeError("semantics of model %d must be float32, got %s" % (i, t.dtype))
        if t.dim() != 2 or t.shape[0] != m.xyz.shape[0]:
            raise ValueError("semantics of model %d must be [N,S]" % i)
        if S is not None and t.shape[1] != S:
            raise ValueError("all models must carry the same number of semantic channels (%d and %d)" % (S, t.shape[1]))
        S = int(t.shape[1])
        out.append(t)
    if S is None:
        return [], 0
    return out, S


def _check_models(models):
    for i, m in enumerate(models):
        for name, t in zip(ModelParams._fields[:6], m[:6]):
            if not t.is_cuda:
                raise RuntimeError("gaussianrpg_amd: %s of model %d must live on the device: there is no CPU path" % (name, i))
            if t.dtype != torch.float32:
                raise TypeError("%s of model %d must be float32, got %s" % (name, i, t.dtype))


class _ComposeFeatures(torch.autograd.Function):
    """compose_features with a graph: backward = _C.compose_features_backward (C ABI grpg_compose_features_backward)."""

    @staticmethod
    def forward(ctx, nm, pose_t, idft_t, flips, normals, campos, pose_rot, S, *flat):
        lists = _split(flat, nm)
        sems = list(flat[6 * nm:])
        ctx.nm, ctx.pose_t, ctx.idft_t, ctx.flips, ctx.normals, ctx.campos, ctx.S = nm, pose_t, idft_t, flips, normals, campos, S
        ctx.pose_dev = None if pose_rot is None else pose_rot.device
        ctx.save_for_backward(*flat[:6 * nm])
        return _C.compose_features(*lists, flips, pose_t, idft_t, sems, normals, campos)

    @staticmethod
    def backward(ctx, g_features):
        nm = ctx.nm
        lists = _split(ctx.saved_tensors, nm)
        need = ctx.needs_input_grad
        want_sem = [bool(n) for n in need[8 + 6 * nm:]] or [False] * nm
        g_rot, g_sem, g_poses = _C.compose_features_backward(
            *lists, ctx.flips, ctx.pose_t, ctx.idft_t, ctx.S, want_sem, ctx.normals, ctx.campos, g_features.contiguous())
        grads = [None] * (6 * nm)
        for i in range(nm):
            if need[8 + 2 * nm + i] and ctx.normals:
                grads[2 * nm + i] = g_rot[i]
        sem_grads = [g if (n and g.numel()) else None for g, n in zip(g_sem, need[8 + 6 * nm:])]
        if isinstance(ctx.pose_t, tuple):   # a PoseTable: dense over the table's rows
            g_pose_rot = _scatter_pose_grads(ctx.pose_t, g_poses, need[6], False)[0]
        else:
            g_pose_rot = g_poses[:, 0:4].to(ctx.pose_dev) if need[6] else None
        return (None, None, None, None, None, None, g_pose_rot, None) + tuple(grads) + tuple(sem_grads)


def compose_features(models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]], semantics=None,
                     normals: bool = False, campos=None):
    """The feature array of a composed frame alone, ``[P,F]`` with ``F = 3 * normals + S``: the normals first
    (``GaussianModel.get_normals``, gaussian_model.py:256-269, on the world rotations / scales / means ``compose``
    returns; for actors ``R_obj n_local`` with the sign taken in the world frame), then the models' semantic arrays
    (``semantics``: one ``[N_i,S]`` tensor or None -- zeros -- per model; street_gaussian_model.py:420-435), computed
    by the HIP code ``ComposedRasterizer.forward_features`` uses.  Differentiable with respect to the raw rotations,
    tensor-valued ``obj_rot`` and the semantic arrays (none through the axis choice, the sign, the means or the
    scales, like the reference)."""
    _check_models(models)
    sems, S = _semantic_list(models, semantics)
    if normals and campos is None:
        raise ValueError("normals=True needs campos (the camera centre the normals are turned towards)")
    lists, pose_t, idft_t = _pack(models, poses)
    dev = models[0].xyz.device
    campos = _NO_SEMANTIC if campos is None else campos.detach().to(device=dev, dtype=torch.float32).reshape(-1)
    normals = bool(normals)
    rot_tensors = [poses.rot] if isinstance(poses, (PoseRows, PoseTable)) else \
        [p.obj_rot for p in poses if p is not None and isinstance(p.obj_rot, torch.Tensor)]
    train = torch.is_grad_enabled() and any(
        t.requires_grad for t in (lists[2] if normals else []) + (rot_tensors if normals else []) + list(sems))
    if not train:
        with torch.no_grad():
            return _C.compose_features(*lists, pose_t, idft_t, sems, normals, campos)
    pose_rot, _ = _pose_graph(poses, rot_tensors)
    flat = [t for per_field in lists[:6] for t in per_field]
    return _ComposeFeatures.apply(len(models), pose_t, idft_t, lists[6], normals, campos, pose_rot, S, *flat, *sems)


def gaussian_normals(scaling, rotation, xyz, campos):
    """Drop-in for ``GaussianModel.get_normals(camera)`` (gaussian_model.py:256-269) on one static model: the raw
    ``_scaling`` / ``_rotation`` / ``_xyz`` and ``camera.camera_center`` -> ``[N,3]``."""
    n = xyz.shape[0]
    dc = xyz.new_zeros(n, 1, 3)   # (colour and opacity take no part)
    m = ModelParams(xyz, scaling, rotation, xyz.new_zeros(n, 1), dc, xyz.new_zeros(n, 0, 3))
    return compose_features([m], [None], None, True, campos)


def _rasterize(rs, lists, pose_t, idft_t, sems, normals, S, for_backward):
    """One composed forward: _C.rasterize_gaussians_composed for a frame without feature planes (F = 3 * normals + S
    = 0), _C.rasterize_gaussians_composed_features otherwise -> the latter's tuple (num_rendered, color, depth, alpha,
    features [F,H,W], radii, geom, binning, img, feature blob)."""
    camera = (rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
              rs.image_width, rs.sh_degree, rs.campos, rs.debug, for_backward)
    if not normals and S == 0:
        num_rendered, color, depth, alpha, radii, geom, binning, img = _C.rasterize_gaussians_composed(
            rs.bg, *lists, pose_t, idft_t, *camera)
        features = alpha.new_empty(0, rs.image_height, rs.image_width)
        return num_rendered, color, depth, alpha, features, radii, geom, binning, img, _NO_SEMANTIC
    return _C.rasterize_gaussians_composed_features(rs.bg, *lists, pose_t, idft_t, sems, normals, *camera)


class _ComposedRasterize(torch.autograd.Function):
    """Training path of forward (F = 0) and forward_features: forward = _rasterize(for_backward=True), backward =
    _C.rasterize_gaussians_composed_backward (C ABI grpg_backward_composed at F = 0, grpg_backward_composed_features
    otherwise)."""

    @staticmethod
    def forward(ctx, owner, rs, nm, pose_t, idft_t, flips, normals, S, pose_rot, pose_trans, means2D, *flat):
        num_rendered, color, depth, alpha, features, radii, geom, binning, img, blob = _rasterize(
            rs, _split(flat, nm) + [flips], pose_t, idft_t, list(flat[6 * nm:]), normals, S, True)
        ctx.rs, ctx.nm, ctx.num_rendered, ctx.normals, ctx.S = rs, nm, num_rendered, normals, S
        owner.num_rendered = num_rendered   # like the evaluation branch of ComposedRasterizer._render
        ctx.pose_t, ctx.idft_t, ctx.flips = pose_t, idft_t, flips
        ctx.pose_dev = (None if pose_rot is None else pose_rot.device,
                        None if pose_trans is None else pose_trans.device)
        ctx.save_for_backward(radii, alpha, geom, binning, img, blob, *flat[:6 * nm])
        ctx.mark_non_differentiable(radii)
        return color, radii, depth, alpha, features

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth, g_alpha, g_features):
        # forward's arguments: 8 without a gradient, pose_rot, pose_trans, means2D, 6 * nm parameters, the semantics
        return (None,) * 8 + _composed_backward(ctx, 11, ctx.saved_tensors[:6], ctx.saved_tensors[6:], g_color, g_depth,
                                                g_alpha, g_features)


def _composed_backward(ctx, first, state, params, g_color, g_depth, g_alpha, g_features, objects=None):
    """The one backward call of a composed training frame -> (g_pose_rot, g_pose_trans, g_means2D, parameter
    gradients..., semantic gradients...).  forward's arguments: pose_rot, pose_trans, means2D at 8, 9, 10, the
    6 * nm parameters from `first`, then the semantics.  objects: (alpha_object, workspace, g_alpha_object) of
    forward_objects -- the object-alpha plane's gradient rides along (C ABI grpg_backward_composed_objects)."""
    rs, nm = ctx.rs, ctx.nm
    radii, alpha, geom, binning, img, blob = state
    need = ctx.needs_input_grad
    need_params, need_sem = need[first:first + 6 * nm], need[first + 6 * nm:]
    F = 3 * int(ctx.normals) + ctx.S
    zeros = lambda *shape: alpha.new_zeros(*shape, *alpha.shape[-2:])   # noqa: E731  (an output the loss does not touch)
    if F == 0:
        g_features = _NO_SEMANTIC
    args = (rs.bg, *_split(params, nm), ctx.flips, ctx.pose_t, ctx.idft_t, ctx.S,
            [bool(n) for n in need_sem] or [False] * nm, ctx.normals, rs.scale_modifier, rs.viewmatrix, rs.projmatrix,
            rs.tanfovx, rs.tanfovy, rs.sh_degree, rs.campos, radii, alpha, geom, ctx.num_rendered, binning, img, blob,
            g_color if g_color is not None else zeros(3),
            g_depth if g_depth is not None else zeros(1),
            g_alpha if g_alpha is not None else zeros(1),
            g_features if g_features is not None else zeros(F))
    if objects is None:
        out = _C.rasterize_gaussians_composed_backward(*args, rs.debug)
    else:
        out = _C.rasterize_gaussians_composed_objects_backward(*args, *objects, rs.debug)
    *g_params, g_sem, g_means2D, g_poses = out
    if isinstance(ctx.pose_t, tuple):   # a PoseTable: dense over the table's rows
        g_rot, g_trans = _scatter_pose_grads(ctx.pose_t, g_poses, need[8], need[9])
    else:
        g_rot = g_poses[:, 0:4].to(ctx.pose_dev[0]) if need[8] else None
        g_trans = g_poses[:, 4:7].to(ctx.pose_dev[1]) if need[9] else None
    grads = [g for per_field in g_params for g in per_field]
    flat_grads = tuple(g if n else None for g, n in zip(grads, need_params))
    sem_grads = tuple(g if (n and g.numel()) else None for g, n in zip(g_sem, need_sem))
    return (g_rot, g_trans, g_means2D if need[10] else None) + flat_grads + sem_grads


_NO_CLASS = torch.empty(0, dtype=torch.uint8)
_CLASS_CACHE = {}   # (counts, flags, device) -> uint8 [P] on the device; the last set of models only


def _layer_class(models, flags, device):
    """uint8 [P] on the device, 1 = the Gaussian's model is an object: built once per set of models (their counts and
    flags), not per frame."""
    counts = tuple(int(m.xyz.shape[0]) for m in models)
    key = (counts, tuple(flags), str(device))
    t = _CLASS_CACHE.get(key)
    if t is None:
        _CLASS_CACHE.clear()
        host = torch.repeat_interleave(torch.tensor(flags, dtype=torch.uint8), torch.tensor(counts))
        t = _CLASS_CACHE[key] = host.to(device)
    return t


def _objects_frame(owner, rs, nm, pose_t, idft_t, flips, normals, S, layer_class, any_object, flat):
    """The composed TRAINING forward and the object-alpha forward on its blobs -> ((color, radii, depth, alpha,
    features, alpha_object), (geom, binning, img, feature blob, workspace))."""
    num_rendered, color, depth, alpha, features, radii, geom, binning, img, blob = _rasterize(
        rs, _split(flat, nm) + [flips], pose_t, idft_t, list(flat[6 * nm:]), normals, S, True)
    owner.num_rendered = num_rendered
    if any_object:
        alpha_object, workspace = _C.object_alpha_forward(geom, binning, img, radii.shape[0], layer_class,
                                                          rs.image_height, rs.image_width)
    else:   # the plane is exactly zero and the backward the plain one
        alpha_object, workspace = torch.zeros_like(alpha), _NO_CLASS
    return (color, radii, depth, alpha, features, alpha_object), (geom, binning, img, blob, workspace)


class _ComposedRasterizeObjects(torch.autograd.Function):
    """Training path of forward_objects: forward = the composed training forward (_rasterize(for_backward=True))
    followed by _C.object_alpha_forward on its blobs (C ABI grpg_object_alpha_forward); backward = ONE call,
    grpg_backward_composed_objects -- or the plain composed backward when the loss does not touch alpha_object or
    no model is an object."""

    @staticmethod
    def forward(ctx, owner, rs, nm, pose_t, idft_t, flips, normals, S, pose_rot, pose_trans, means2D, layer_class,
                any_object, *flat):
        outs, state = _objects_frame(owner, rs, nm, pose_t, idft_t, flips, normals, S, layer_class, any_object, flat)
        ctx.rs, ctx.nm, ctx.num_rendered, ctx.normals, ctx.S, ctx.any_object = rs, nm, owner.num_rendered, normals, S, any_object
        ctx.pose_t, ctx.idft_t, ctx.flips = pose_t, idft_t, flips
        ctx.pose_dev = (None if pose_rot is None else pose_rot.device,
                        None if pose_trans is None else pose_trans.device)
        ctx.save_for_backward(outs[1], outs[3], *state, outs[5], *flat[:6 * nm])   # radii, alpha, ..., alpha_object
        ctx.mark_non_differentiable(outs[1])
        return outs

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth, g_alpha, g_features, g_alpha_object):
        workspace, alpha_object = ctx.saved_tensors[6:8]
        objects = None
        if g_alpha_object is not None and ctx.any_object:
            objects = (alpha_object, workspace, g_alpha_object)
        # forward's arguments: 8 without a gradient, pose_rot, pose_trans, means2D, layer_class, any_object, then the
        # 6 * nm parameters and the semantics
        g = _composed_backward(ctx, 13, ctx.saved_tensors[:6], ctx.saved_tensors[8:], g_color, g_depth, g_alpha,
                               g_features, objects)
        return (None,) * 8 + g[:3] + (None, None) + g[3:]


class ComposedRasterizer(nn.Module):
    """``GaussianRasterizer`` for a scene graph: takes per-model raw parameters + per-frame actor
    poses, returns ``(color, radii, depth, alpha)`` like the classic module (no semantics).
    Differentiable with respect to the raw parameters, tensor-valued poses and ``means2D``."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward_layers(self, models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]],
                       object_models: Optional[Sequence[bool]] = None, layer_bg=None) -> dict:
        """Evaluation only: the composition AND the three renders of the reference's
        ``StreetGaussianRenderer.render_all`` (street_gaussian_renderer.py:13-40: all models, the background
        model alone, the object models alone -- the last two on ``layer_bg``, default white) from ONE call on the
        raw parameters (C ABI ``grpg_forward_composed_layers``).  ``object_models``: one flag per model, default
        "every posed model (actor) is an object".  Returns the dict of ``GaussianRasterizer.forward_layers``;
        every plane is bit-identical to that call on ``compose(models, poses)``'s output."""
        rs = self.raster_settings
        lists, pose_t, idft_t = _pack(models, poses)
        if layer_bg is None:
            layer_bg = _white(models[0].xyz.device)
        with torch.no_grad():
            out = _C.rasterize_gaussians_composed_layers(
                rs.bg, layer_bg, _object_flags(object_models), *lists, pose_t, idft_t, rs.scale_modifier,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.sh_degree,
                rs.campos, rs.debug)
        self.num_rendered = out[0]
        return _layers_result(out)

    def forward_frame(self, models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]], *,
                      sky_cube=None, ray_matrix=None, sky_fill=0.0, clamp=True, planes=False, rgb8=True,
                      truncate=True, out=None, layers=False, object_models: Optional[Sequence[bool]] = None,
                      layer_bg=None, affine=None) -> dict:
        """The reference's whole per-frame evaluation path as ONE call on the raw parameters (C ABI
        ``grpg_forward_composed_frame``): scene-graph composition (street_gaussian_model.py:296-453), the op,
        ``StreetGaussianRenderer.render``'s clamp / sky composite / clamp (street_gaussian_renderer.py:106-116,
        236-237) and the simulator's uint8 [H,W,3] conversion (simulator.py:313-314) -- the last three inside the
        render's epilogue.  ``layers=True`` also returns render_all's two layer renders (forward_layers); the
        simulator reads ``result['rgb']`` only and does not need them.  Returns a dict: ``rgb8`` (uint8 [H,W,3] on the
        device; ``out``: a preallocated device tensor, or a PINNED HOST tensor -- the bytes then land in host memory
        while the render runs, no copy behind the launch: what the simulator wants; synchronise with the stream before
        reading), with ``planes=True`` also ``rgb`` (the FINAL colour) / ``depth`` /
        ``alpha``, with ``layers=True`` the four layer planes; ``radii``, ``num_rendered``.  ``affine``: the colour
        correction of ``GaussianRasterizer.forward_frame`` (a float32 [3,4] device tensor, applied to the composition
        between the sky composite and the final clamp); it rides on the same call as device poses (``PoseBatch.rows``)."""
        rs = self.raster_settings
        lists, pose_t, idft_t = _pack(models, poses)
        if layers and layer_bg is None:
            layer_bg = _white(models[0].xyz.device)
        layer_bg, sky_cube, ray_matrix = _or_empty(layer_bg, sky_cube, ray_matrix)
        with torch.no_grad():
            ret = _C.rasterize_gaussians_composed_frame(
                rs.bg, layer_bg, _object_flags(object_models), bool(layers), *lists, pose_t, idft_t,
                rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                rs.image_width, rs.sh_degree, rs.campos, rs.debug, sky_cube, ray_matrix, float(sky_fill), bool(clamp),
                bool(planes), bool(rgb8), bool(truncate), out, affine)
        self.num_rendered = ret[0]
        return _frame_result(ret, rgb8, planes, layers)

    def _render(self, models, poses, semantics, normals, means2D):
        """forward (no feature planes) and forward_features -> (color, radii, depth, alpha, features [F,H,W])"""
        rs = self.raster_settings
        sems, S = _semantic_list(models, semantics)
        lists, pose_t, idft_t = _pack(models, poses)
        flat = [t for per_field in lists[:6] for t in per_field]
        pose_tensors = _pose_tensors(poses)
        train = torch.is_grad_enabled() and any(
            t.requires_grad for t in flat + pose_tensors + list(sems) + ([means2D] if means2D is not None else []))
        if not train:
            with torch.no_grad():
                num_rendered, color, depth, alpha, features, radii = _rasterize(
                    rs, lists, pose_t, idft_t, sems, normals, S, False)[:6]
            self.num_rendered = num_rendered
            return color, radii, depth, alpha, features
        pose_rot, pose_trans = _pose_graph(poses, pose_tensors)
        return _ComposedRasterize.apply(self, rs, len(models), pose_t, idft_t, lists[6], normals, S, pose_rot,
                                        pose_trans, means2D, *flat, *sems)

    def forward(self, models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]], means2D=None):
        return self._render(models, poses, None, False, means2D)[:4]

    def forward_objects(self, models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]],
                        object_models: Optional[Sequence[bool]] = None, semantics=None, normals: bool = False,
                        means2D=None):
        """``forward_features`` plus the object-alpha plane of the SAME frame: returns ``(color, radii, depth, alpha,
        features, alpha_object)`` with ``alpha_object [1,H,W]`` = the ``alpha`` a ``forward`` over the object models
        alone returns, bit for bit -- what train.py:145-158 renders a second time (``render_object``) to read
        ``acc_obj`` for the object-alpha loss.  ``object_models``: one flag per model, default "every posed model
        (actor) is an object", as in ``forward_layers``.  The plane is blended from the tile lists and projected
        records the main render left behind (C ABI ``grpg_object_alpha_forward``), and its gradient joins the frame's
        ONE backward call (``grpg_backward_composed_objects``) between the blend backward and the preprocess
        backward: no second composition, preprocess, binning or preprocess backward.  A loss that does not touch
        ``alpha_object``, or a frame without object models (the plane is exactly zero), takes the plain backward.
        Under ``torch.no_grad()`` the same tuple is returned and no state is kept -- but the frame underneath is still a
        TRAINING forward (gradient records carved, ``n_contrib`` and blend checkpoints written): the plane is blended
        from a training frame's blobs only.  An evaluation loop that wants the object layer uses ``forward_layers``.

        ``means2D.grad`` is the SUM of both planes' terms on the object rows -- as if one leaf had fed both renders
        of the reference (which creates a leaf per render and reads the main render's for densification); rows of
        background models see the main render's term only."""
        if object_models is not None and len(object_models) != len(models):
            raise ValueError("object_models: one flag per model (%d flags, %d models)" % (len(object_models), len(models)))
        _check_models(models)
        rs = self.raster_settings
        sems, S = _semantic_list(models, semantics)
        lists, pose_t, idft_t = _pack(models, poses)
        flags = _posed_flags(poses) if object_models is None else [bool(f) for f in object_models]
        # default flags: the class comes from the frame's own segment table on the device
        layer_class = _NO_CLASS if object_models is None else _layer_class(models, flags, models[0].xyz.device)
        flat = [t for per_field in lists[:6] for t in per_field]
        pose_tensors = _pose_tensors(poses)
        train = torch.is_grad_enabled() and any(
            t.requires_grad for t in flat + pose_tensors + list(sems) + ([means2D] if means2D is not None else []))
        head = (rs, len(models), pose_t, idft_t, lists[6], bool(normals), S)
        if not train:
            with torch.no_grad():
                return _objects_frame(self, *head, layer_class, any(flags), flat + list(sems))[0]
        pose_rot, pose_trans = _pose_graph(poses, pose_tensors)
        return _ComposedRasterizeObjects.apply(self, *head, pose_rot, pose_trans, means2D, layer_class, any(flags),
                                               *flat, *sems)

    def forward_features(self, models: Sequence[ModelParams], poses: Sequence[Optional[ActorPose]], semantics=None,
                         normals: bool = False, means2D=None):
        """``forward`` with ``F = 3 * normals + S`` feature planes (C ABI ``grpg_forward_composed_features`` /
        ``grpg_backward_composed_features``): returns ``(color, radii, depth, alpha, features [F,H,W])``, the normal
        planes first, then the semantic ones -- the order of street_gaussian_renderer.py:205-215.  ``semantics``: one
        ``[N_i,S]`` tensor, or None (zeros), per model.  The planes are raw: ``F.normalize(dim=0)`` of the normals and
        the ``probabilities`` transform of the semantics stay with the caller (``semantic_loss(mode=...)`` takes raw
        planes).  Differentiable like ``forward``, and with respect to the semantic arrays; the normals' gradient
        reaches the raw rotations and tensor-valued ``obj_rot``.  A backward needs F <= 32; the forward takes any F."""
        _check_models(models)
        return self._render(models, poses, semantics, bool(normals), means2D)
