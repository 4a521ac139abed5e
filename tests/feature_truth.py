"""PyTorch restatement of the feature array of a composed frame (csrc/features.hip) -- TEST INFRASTRUCTURE ONLY.

``features(models, poses, semantics, normals, campos, dtype)`` -> ``[P,F]``, F = 3 * normals + S, normals first
(the reference's order, lib/models/street_gaussian_renderer.py:205-215), in ``dtype`` (float64: the truth; float32:
the yardstick of the gradient tests), differentiable by autograd.

* semantic channels: ``torch.cat`` of the models' arrays (street_gaussian_model.py:420-435); None -> zeros.
* normal channels: ``GaussianModel.get_normals`` (lib/models/gaussian_model.py:256-269) on the WORLD values of the
  composition: k = argmin of exp(_scaling) (:257, :259), R = quaternion_to_matrix(world rotation)
  (:258, general_utils.py:125-146), n = R[i, :, k] (:260-261), dir = world mean - camera centre (:264), negated
  unless sum(-dir / |dir| * n) >= 0 (:265-267).  The world rotation is normalize(_rotation) for a static model and
  normalize(obj_rot (x) [flip (x)] normalize(_rotation)) for an actor (street_gaussian_model.py:314-338), the world
  mean R(obj_rot) x + obj_trans (:340-365).  For actors this replaces street_gaussian_model.py:463-484, which raises
  (:480 ``torch.nn.functinal``) and takes the sign of a local normal against a world camera centre (:474).
"""
import torch

from oracle import compose_torch as ct


def world(models, poses, dtype=torch.float64):
    """(means [P,3], scales [P,3], rotations [P,4]) of the composition in `dtype`; poses: None or
    (obj_rot, obj_trans, ...) per model, tensors keep their graph."""
    means, scales, rots = [], [], []
    for m, p in zip(models, poses):
        n = m.xyz.shape[0]
        dev = m.xyz.device
        xyz = m.xyz.to(dtype)
        scales.append(torch.exp(m.scaling.to(dtype)))
        rot = torch.nn.functional.normalize(m.rotation.to(dtype))
        flip = getattr(m, "flip", None)
        if flip is not None and p is not None:
            fq = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=dtype, device=dev).expand(n, 4)
            rot = torch.where(flip[:, None], ct.quaternion_raw_multiply(fq, rot), rot)
            xyz = torch.where(flip[:, None] & (torch.arange(3, device=dev) == 1)[None], -xyz, xyz)
        if p is not None:
            obj_rot = torch.as_tensor(p[0]).to(device=dev, dtype=dtype).reshape(1, 4).expand(n, -1)
            obj_trans = torch.as_tensor(p[1]).to(device=dev, dtype=dtype).reshape(1, 3).expand(n, -1)
            xyz = torch.einsum("bij, bj -> bi", ct.quaternion_to_matrix(obj_rot), xyz) + obj_trans
            rot = torch.nn.functional.normalize(ct.quaternion_raw_multiply(obj_rot, rot))
        means.append(xyz)
        rots.append(rot)
    return torch.cat(means, 0), torch.cat(scales, 0), torch.cat(rots, 0)


def normals_of(means, scales, rots, campos, with_details=False):
    """gaussian_model.py:256-269 on world values."""
    R = ct.quaternion_to_matrix(rots)
    k = torch.argmin(scales, dim=-1)
    n = R[torch.arange(k.shape[0], device=k.device), :, k]
    dir_pp = means - campos.to(means)[None]
    dir_n = dir_pp / dir_pp.norm(dim=1, keepdim=True)
    dot = torch.sum(-dir_n * n, dim=1, keepdim=True)
    out = torch.where(dot >= 0, n, -n)
    return (out, k, dot[:, 0]) if with_details else out


def features(models, poses, semantics=None, normals=False, campos=None, dtype=torch.float64):
    parts = []
    if normals:
        parts.append(normals_of(*world(models, poses, dtype), campos))
    if semantics is not None and any(s is not None for s in semantics):
        S = next(s.shape[1] for s in semantics if s is not None)
        parts.append(torch.cat([torch.zeros(m.xyz.shape[0], S, dtype=dtype, device=m.xyz.device) if s is None
                                else s.to(dtype) for m, s in zip(models, semantics)], 0))
    if not parts:
        P = sum(m.xyz.shape[0] for m in models)
        return torch.zeros(P, 0, dtype=dtype, device=models[0].xyz.device)
    return torch.cat(parts, 1)
