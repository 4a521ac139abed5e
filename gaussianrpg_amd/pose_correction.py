"""Pose correction of the background on the HIP library (csrc/pose_correction.hip; additive API).

A scene trained with ``use_pose_correction: true`` moves every background Gaussian by a learned rigid transform, one
per image or per frame (lib/models/camera_pose.py); ``StreetGaussianModel.get_xyz`` / ``get_rotation`` apply it in
train and evaluate mode (street_gaussian_model.py:319-320, 345-346).  This module provides it both ways:

    pc = PoseCorrection(num_images, mode='image').cuda()
    xyz = pc.correct_gaussian_xyz(camera, xyz)                  # the reference's calls, one launch each way
    rotation = pc.correct_gaussian_rotation(camera, rotation)
    xyz, rotation = pc.correct(camera, xyz, rotation)           # both in ONE launch

    # composed route: the background is a posed model, its row read from device memory by the frame's own kernels
    poses, object_models = pc.rows(batch, t, camera, visible_actor_indices, fourier_times)
    out = rasterizer.forward_objects(models, poses, object_models)

The correction row is read from device memory (``pose_correction_rots[id]`` is a view: no host copy, no host wait), the
backward recomputes what it needs from its inputs and sums the row's gradient in a fixed order without atomics:
identical calls give identical bits.

The two routes differ in one step.  The classic op is the reference's arithmetic: ``quaternion_raw_multiply(q^,
rotation)`` is NOT normalised behind it (camera_pose.py:112).  The composed route goes through ``compose_one``'s rigid
path, which normalises the product, as the reference does for an actor; with an activated (unit) ``rotation`` the two
agree to rounding.

``regularization_loss`` and the [4,4] matrix of ``forward`` are a handful of numbers and stay PyTorch.
"""
from typing import Optional, Sequence

import torch
import torch.nn as nn

from .composed import PoseTable
from .rasterizer import _C


class _PoseCorrect(torch.autograd.Function):
    """(R(q^) xyz + trans, q^ (x) rotation); either of xyz / rotation may be None, and so is its output."""

    @staticmethod
    def forward(ctx, xyz, rotation, rot, trans):
        out_xyz, out_rotation = _C.pose_correct(xyz, rotation, rot, trans)
        ctx.set_materialize_grads(False)
        ctx.has = (xyz is not None, rotation is not None)
        ctx.save_for_backward(*[t for t in (xyz, rotation) if t is not None], rot, trans)
        return out_xyz, out_rotation

    @staticmethod
    def backward(ctx, grad_xyz, grad_rotation):
        saved = list(ctx.saved_tensors)
        xyz = saved.pop(0) if ctx.has[0] else None
        rotation = saved.pop(0) if ctx.has[1] else None
        rot, trans = saved
        if grad_xyz is None and grad_rotation is None:
            return None, None, None, None
        need_xyz, need_rotation, need_rot, need_trans = ctx.needs_input_grad
        need_xyz = need_xyz and grad_xyz is not None
        need_rotation = need_rotation and grad_rotation is not None
        need_trans = need_trans and grad_xyz is not None      # trans only moves xyz'
        if not (need_xyz or need_rotation or need_rot or need_trans):
            return None, None, None, None
        g_xyz, g_rotation, g_rot, g_trans = _C.pose_correct_backward(
            xyz, rotation, rot, trans, grad_xyz, grad_rotation, need_xyz, need_rotation, need_rot, need_trans)
        return (g_xyz if need_xyz else None, g_rotation if need_rotation else None,
                g_rot.reshape(rot.shape) if need_rot else None, g_trans.reshape(trans.shape) if need_trans else None)


def pose_correct(xyz: Optional[torch.Tensor], rotation: Optional[torch.Tensor], rot: torch.Tensor, trans: torch.Tensor):
    """``(xyz', rotation')`` of camera_pose.py:89-114 for float32 device tensors ``xyz [N,3]`` / ``rotation [N,4]``
    (either may be None, and then so is its output) and ANY float32 device tensors ``rot [4]`` (w,x,y,z, raw) /
    ``trans [3]``, e.g. views of the module's parameters: ``xyz' = quaternion_to_matrix(F.normalize(rot)) xyz + trans``,
    ``rotation' = quaternion_raw_multiply(F.normalize(rot), rotation)`` with no normalisation behind it.  One launch;
    differentiable w.r.t. all four (one launch and one finishing workgroup)."""
    return _PoseCorrect.apply(xyz, rotation, rot, trans)


class _PoseRows(torch.autograd.Function):
    """The frame's pose table with the background's row in it: the actors' rows, then the raw correction row id."""

    @staticmethod
    def forward(ctx, rot, trans, corr_rots, corr_trans, id):
        ctx.n, ctx.id, ctx.A = int(corr_rots.shape[0]), int(id), int(rot.shape[0])
        return _C.pose_rows(rot, trans, corr_rots, corr_trans, int(id))

    @staticmethod
    def backward(ctx, grad_rot, grad_trans):
        g_rots = g_trans = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            g_rots, g_trans = _C.pose_rows_backward(grad_rot, grad_trans, ctx.n, ctx.id)
        A = ctx.A
        return (grad_rot[:A] if ctx.needs_input_grad[0] else None, grad_trans[:A] if ctx.needs_input_grad[1] else None,
                g_rots if ctx.needs_input_grad[2] else None, g_trans if ctx.needs_input_grad[3] else None, None)


class PoseCorrection(nn.Module):
    """Drop-in for lib/models/camera_pose.py:PoseCorrection: the same parameter names, shapes and initial values, the
    same ``get_id`` / ``forward`` / ``correct_gaussian_xyz`` / ``correct_gaussian_rotation`` / ``regularization_loss``
    and the same ``{'params': ...}`` state-dict layout, so state dicts interchange.  ``num_poses`` is
    ``metadata['num_images']`` for ``mode='image'`` (one row per ``camera.id``) and ``metadata['num_frames']`` for
    ``mode='frame'`` (one per ``camera.meta['frame_idx']``).

    ``active`` is the reference's ``cfg.mode in ['train', 'evaluate']`` gate: with ``active=False`` (trajectory and
    simulator modes) the correcting methods return their input untouched and ``table`` / ``rows`` leave the background
    static.  The optimizer is the caller's (``optim.FusedAdam`` or torch's)."""

    def __init__(self, num_poses: int, mode: str = "image", active: bool = True):
        super().__init__()
        if mode not in ("image", "frame"):
            raise ValueError("Invalid mode: %s" % mode)
        self.mode = mode
        self.active = bool(active)
        # not part of the state dict: the reference keeps it as a plain attribute
        self.register_buffer("identity_matrix", torch.eye(4).float()[:3].clone(), persistent=False)
        self.pose_correction_trans = nn.Parameter(torch.zeros(int(num_poses), 3).float())
        self.pose_correction_rots = nn.Parameter(torch.tensor([[1, 0, 0, 0]]).repeat(int(num_poses), 1).float())

    def save_state_dict(self, is_final: bool = True):
        state_dict = {"params": self.state_dict()}
        if not is_final and getattr(self, "optimizer", None) is not None:
            state_dict["optimizer"] = self.optimizer.state_dict()
        return state_dict

    def load_state_dict(self, state_dict, strict: bool = True):
        return super().load_state_dict(state_dict["params"], strict=strict)

    def get_id(self, camera):
        if self.mode == "image":
            return camera.id
        return camera.meta["frame_idx"]

    def row(self, camera):
        """(rot [4], trans [3]) of the camera: views of the parameters."""
        id = self.get_id(camera)
        return self.pose_correction_rots[id], self.pose_correction_trans[id]

    def forward(self, camera):
        # sixteen numbers: stays PyTorch (camera_pose.py:77-87); quaternion_to_matrix's expressions of q^ / |q^|
        rot, trans = self.row(camera)
        q = torch.nn.functional.normalize(rot.unsqueeze(0)).squeeze(0)
        r, x, y, z = (q / torch.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])).unbind(0)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).view(3, 3)
        padding = torch.tensor([[0, 0, 0, 1]], dtype=R.dtype, device=R.device)
        return torch.cat([torch.cat([R, trans[:, None]], dim=-1), padding], dim=0)

    def correct_gaussian_xyz(self, camera, xyz: torch.Tensor):
        if not self.active:
            return xyz
        return pose_correct(xyz, None, *self.row(camera))[0]

    def correct_gaussian_rotation(self, camera, rotation: torch.Tensor):
        if not self.active:
            return rotation
        return pose_correct(None, rotation, *self.row(camera))[1]

    def correct(self, camera, xyz: torch.Tensor, rotation: torch.Tensor):
        """``(correct_gaussian_xyz(camera, xyz), correct_gaussian_rotation(camera, rotation))`` in ONE launch."""
        if not self.active:
            return xyz, rotation
        return pose_correct(xyz, rotation, *self.row(camera))

    def regularization_loss(self):
        # a few numbers per pose: stays PyTorch (camera_pose.py:116-121)
        loss_trans = torch.abs(self.pose_correction_trans).mean()
        rots_norm = torch.nn.functional.normalize(self.pose_correction_rots, dim=-1)
        one = torch.tensor([[1, 0, 0, 0]], dtype=rots_norm.dtype, device=rots_norm.device)
        loss_rots = torch.abs(rots_norm - one).mean()
        return loss_trans + loss_rots

    # ---- composed route ----
    def table(self, camera):
        """For a scene WITHOUT tracked actors: ``(poses, object_models)`` for ``ComposedRasterizer`` with the
        background as the frame's only model, posed by its correction row.  ``poses`` is a ``composed.PoseTable``
        straight over the parameter tensors (row = id): no launch, no copy; in training the dense ``[n,4]`` / ``[n,3]``
        parameter gradients come back, zero outside row id.

        ``object_models`` is ``[False]``: pass it on.  ``forward_layers``, ``forward_frame`` and ``forward_objects``
        default to "every posed model is an object", which is wrong for a posed background.  Inactive: the background
        is static."""
        if not self.active:
            return PoseTable(self.pose_correction_rots, self.pose_correction_trans, [-1], [False], [0.0]), [False]
        return PoseTable(self.pose_correction_rots, self.pose_correction_trans, [int(self.get_id(camera))], [True],
                         [0.0]), [False]

    def rows(self, batch, t: int, camera, actors: Sequence[int], fourier_time: Optional[Sequence[float]] = None):
        """``PoseBatch.rows`` with the background's correction in it: ``(poses, object_models)`` for
        ``ComposedRasterizer``.  ``poses`` is a ``composed.PoseTable`` over an ``[A+1]``-row table made in ONE launch
        (``_C.pose_rows``): rows ``0..A-1`` are ``batch.rot[t]`` / ``batch.trans[t]``, row ``A`` is the RAW correction
        row of the camera (``compose_one`` normalises it itself).  The background is model 0 and reads row ``A``; the
        actors ``actors`` follow with their own rows and ``fourier_time``.  Everything keeps its graph: the actors'
        gradients are the table gradient's first ``A`` rows, the parameters' come back dense, zero outside row id.

        ``object_models`` is background ``False``, actors ``True``: pass it on.  ``forward_layers``, ``forward_frame``
        and ``forward_objects`` default to "every posed model is an object", which is wrong for a posed background.
        Inactive: the background stays static and the result equals ``batch.rows(t, actors, fourier_time)``."""
        base = batch.rows(t, actors, fourier_time)      # checks the actor indices and the times
        flags = [False] + [True] * len(actors)
        if not self.active:
            return base, flags
        A = int(batch.rot.shape[1])
        rot, trans = _PoseRows.apply(batch.rot[t], batch.trans[t], self.pose_correction_rots,
                                     self.pose_correction_trans, int(self.get_id(camera)))
        return PoseTable(rot, trans, [A] + list(base.row[1:]), [True] * (len(actors) + 1),
                         list(base.fourier_time)), flags
