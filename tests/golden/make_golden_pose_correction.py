"""Generate tests/golden/ref_pose_correction.json + ref_pose_correction.npz.  Needs a checkout of the reference
(GaussianRPG); never run by a test:

    python tests/golden/make_golden_pose_correction.py <path to the reference>

Cuts ``get_id``, ``forward``, ``correct_gaussian_xyz``, ``correct_gaussian_rotation`` and ``regularization_loss`` out of
the reference's lib/models/camera_pose.py, and ``quaternion_to_matrix`` / ``quaternion_raw_multiply`` out of
lib/utils/general_utils.py, with ``ast`` (the modules themselves import the config and the CUDA extensions, which are
not installed here) and executes them on CPU tensors over a stub object that holds what ``PoseCorrection.__init__``
sets up (camera_pose.py:10-25: ``mode`` and the two parameters), in both modes.  The hard-coded ``device='cuda'`` of
``quaternion_to_matrix``'s ``torch.zeros`` is dropped as make_golden.py does, and ``Tensor.cuda()`` of the constant
paddings returns the tensor itself; the arithmetic is untouched.  ``cfg.mode`` is 'train' (the methods correct).

The files hold numbers only.  Inputs are not stored: a case names its builders in tests/pose_correction_truth.py and
their arguments (legacy numpy RandomState: stable) and records the sha256 of the input bytes.  Recorded per case: the
[4,4] matrix of ``forward``, what the two correcting methods returned, their autograd gradients at the input and at the
two parameters (upstream gradient: the named builder), ``get_id``'s value, and ``regularization_loss`` with its
gradients.
"""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pose_correction_truth as pt   # noqa: E402  (the input builders)

METHODS = ["get_id", "forward", "correct_gaussian_xyz", "correct_gaussian_rotation", "regularization_loss"]
FUNCTIONS = ["quaternion_to_matrix", "quaternion_raw_multiply"]
NUM = 3     # poses per parameter


class _TorchNoDevice:
    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def zeros(*a, **kw):
        kw.pop("device", None)
        return torch.zeros(*a, **kw)


class _Cfg:
    mode = "train"


def _reference(ref):
    torch.Tensor.cuda = lambda self, *a, **k: self          # no device in this process: the constants stay where they are
    ns = {"torch": _TorchNoDevice(), "Camera": object, "cfg": _Cfg()}
    path = os.path.join(ref, "lib", "utils", "general_utils.py")
    with open(path) as f:
        fns = [n for n in ast.parse(f.read()).body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS]
    assert sorted(n.name for n in fns) == sorted(FUNCTIONS)
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns, type_ignores=[])), path, "exec"), ns)
    path = os.path.join(ref, "lib", "models", "camera_pose.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PoseCorrection"][0]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in methods) == sorted(METHODS)
    stub = ast.ClassDef(name="PoseCorrectionMethods", bases=[], keywords=[], body=methods, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[stub], type_ignores=[])), path, "exec"), ns)
    return ns


class _Camera:
    def __init__(self, id, frame_idx):
        self.id = id
        self.meta = dict(frame_idx=frame_idx)


def params(kind):
    """([NUM,4], [NUM,3]) float32: row n is build_row(kind, seed = n)."""
    rows = [pt.build_row(kind, seed=n) for n in range(NUM)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def _stub(ns, mode, kind):
    o = ns["PoseCorrectionMethods"]()
    o.mode = mode
    rots, trans = params(kind)
    o.pose_correction_rots = torch.nn.Parameter(torch.from_numpy(rots))
    o.pose_correction_trans = torch.nn.Parameter(torch.from_numpy(trans))
    return o


def _cases():
    out = []
    for mode, (cam_id, frame_idx) in (("image", (2, 0)), ("frame", (0, 1))):
        for n, kind in ((65, "near"), (257, "wide"), (63, "norm3"), (64, "small")):
            out.append(dict(name="%s_%d_%s" % (mode, n, kind), mode=mode, N=n, kind=kind, camera_id=cam_id,
                            camera_frame_idx=frame_idx, xyz=dict(N=n, seed=n), rotation=dict(N=n, seed=n + 1),
                            grad_xyz=dict(N=n, C=3, seed=n + 2), grad_rotation=dict(N=n, C=4, seed=n + 3)))
    return out


def _grads(o):
    g = (o.pose_correction_rots.grad, o.pose_correction_trans.grad)
    o.pose_correction_rots.grad = o.pose_correction_trans.grad = None
    return [None if x is None else x.numpy().copy() for x in g]


def main(ref):
    ns = _reference(ref)
    arrays, rows = {}, []
    for c in _cases():
        o = _stub(ns, c["mode"], c["kind"])
        camera = _Camera(c["camera_id"], c["camera_frame_idx"])
        xyz_np, rot_np = pt.build_xyz(**c["xyz"]), pt.build_rotation(**c["rotation"])
        gx_np, gr_np = pt.build_grad(**c["grad_xyz"]), pt.build_grad(**c["grad_rotation"])
        rec = dict(matrix=o.forward(camera).detach().numpy())
        xyz = torch.from_numpy(xyz_np.copy()).requires_grad_(True)
        out = o.correct_gaussian_xyz(camera, xyz)
        out.backward(torch.from_numpy(gx_np.copy()))
        g_rots, g_trans = _grads(o)
        rec.update(xyz=out.detach().numpy(), grad_xyz=xyz.grad.numpy(), xyz_grad_rots=g_rots, xyz_grad_trans=g_trans)
        rotation = torch.from_numpy(rot_np.copy()).requires_grad_(True)
        out = o.correct_gaussian_rotation(camera, rotation)
        out.backward(torch.from_numpy(gr_np.copy()))
        g_rots, g_trans = _grads(o)
        assert g_trans is None
        rec.update(rotation=out.detach().numpy(), grad_rotation=rotation.grad.numpy(), rotation_grad_rots=g_rots)
        loss = o.regularization_loss()
        loss.backward()
        g_rots, g_trans = _grads(o)
        rec.update(reg_loss=loss.detach().numpy().reshape(1), reg_grad_rots=g_rots, reg_grad_trans=g_trans)
        for k, v in rec.items():
            assert v.dtype == np.float32 and np.all(np.isfinite(v)), (c["name"], k)
            arrays["%s/%s" % (c["name"], k)] = v
        rots, trans = params(c["kind"])
        rows.append(dict(c, id=int(o.get_id(camera)), num_poses=NUM,
                         sha256=pt.sha256(xyz_np, rot_np, gx_np, gr_np, rots, trans)))
        print("%-24s id %d" % (c["name"], rows[-1]["id"]))
    source = ("lib/models/camera_pose.py (%s) and lib/utils/general_utils.py (%s) of the reference, cut with ast and "
              "executed on CPU torch %s over a stub" % (", ".join(METHODS), ", ".join(FUNCTIONS),
                                                         torch.__version__.split("+")[0]))
    with open(os.path.join(HERE, "ref_pose_correction.json"), "w") as f:
        json.dump({"source": source, "cases": rows}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_pose_correction.npz"), **arrays)
    print("wrote %d cases, %d arrays" % (len(rows), len(arrays)))


if __name__ == "__main__":
    main(sys.argv[1])
