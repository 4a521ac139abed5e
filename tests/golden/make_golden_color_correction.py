"""Generate tests/golden/ref_color_correction.json + ref_color_correction.npz.  Needs a checkout of the reference
(GaussianRPG); never run by a test:

    python tests/golden/make_golden_color_correction.py <path to the reference>

Cuts ``forward``, ``get_affine_trans``, ``get_id`` and ``regularization_loss`` out of the reference's
lib/models/color_correction.py with ``ast`` (the module itself imports the config and the CUDA extensions, which are not
installed here) and executes them on CPU tensors over a stub object that holds what ``ColorCorrection.__init__`` sets up
for the explicit variant (color_correction.py:10-13,52-55: ``identity_matrix``, ``config.use_mlp = False``, ``mode``,
the two ``[N,3,4]`` parameters), in both modes and with ``use_sky`` both ways.

The files hold numbers only.  Inputs are not stored: a case names its builders in tests/color_correction_truth.py and
their arguments (legacy numpy RandomState: stable) and records the sha256 of the input bytes.  Recorded per case: what
``forward`` returned, its autograd gradients at the image and at the parameter the matrix was taken from (upstream
gradient: the named builder), ``get_id``'s value, and ``regularization_loss`` with its gradients at both parameters.
"""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the truth module reads oracle/ for the sky part
import color_correction_truth as ct   # noqa: E402  (the input builders)

METHODS = ["get_id", "get_affine_trans", "forward", "regularization_loss"]
N = 3     # corrections per parameter


def _reference(ref):
    ns = {"torch": torch, "Camera": object}
    path = os.path.join(ref, "lib", "models", "color_correction.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ColorCorrection"][0]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in methods) == sorted(METHODS)
    stub = ast.ClassDef(name="ColorCorrectionMethods", bases=[], keywords=[], body=methods, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[stub], type_ignores=[])), path, "exec"), ns)
    return ns


class _Config:
    use_mlp = False


class _Camera:
    def __init__(self, id, cam):
        self.id = id
        self.meta = dict(cam=cam)


def params(kind):
    """[N,3,4] float32: row n is build_affine(kind, seed = n) / (kind, seed = 100 + n) for the sky parameter."""
    a = np.stack([ct.build_affine(kind, seed=n) for n in range(N)])
    s = np.stack([ct.build_affine(kind, seed=100 + n) for n in range(N)])
    return a, s


def _stub(ns, mode, kind):
    o = ns["ColorCorrectionMethods"]()
    o.identity_matrix = torch.eye(4).float()[:3]
    o.config = _Config()
    o.mode = mode
    a, s = params(kind)
    o.affine_trans = torch.nn.Parameter(torch.from_numpy(a))
    o.affine_trans_sky = torch.nn.Parameter(torch.from_numpy(s))
    o.cur_affine_trans = None
    return o


def _cases():
    out = []
    for mode, (cam_id, cam_cam) in (("image", (2, 0)), ("sensor", (0, 1))):
        for use_sky in (False, True):
            for (H, W), kind in (((5, 67), "near"), ((9, 130), "wide"), ((1, 1), "identity")):
                out.append(dict(name="%s_%s_%dx%d_%s" % (mode, "sky" if use_sky else "plain", H, W, kind), mode=mode,
                                use_sky=use_sky, H=H, W=W, kind=kind, camera_id=cam_id, camera_cam=cam_cam,
                                image=dict(H=H, W=W, seed=H), grad=dict(H=H, W=W, seed=W)))
    return out


def main(ref):
    ns = _reference(ref)
    arrays, rows = {}, []
    for c in _cases():
        o = _stub(ns, c["mode"], c["kind"])
        camera = _Camera(c["camera_id"], c["camera_cam"])
        image_np, g_np = ct.build_image(**c["image"]), ct.build_grad(**c["grad"])
        image = torch.from_numpy(image_np.copy()).requires_grad_(True)
        out = o.forward(camera, image, use_sky=c["use_sky"])
        out.backward(torch.from_numpy(g_np.copy()))
        p = o.affine_trans_sky if c["use_sky"] else o.affine_trans
        other = o.affine_trans if c["use_sky"] else o.affine_trans_sky
        assert other.grad is None
        rec = dict(out=out.detach().numpy(), grad_image=image.grad.numpy(), grad_param=p.grad.numpy().copy())
        o.affine_trans.grad = o.affine_trans_sky.grad = None
        loss = o.regularization_loss(camera)
        loss.backward()
        rec.update(reg_loss=loss.detach().numpy().reshape(1), reg_grad=o.affine_trans.grad.numpy(),
                   reg_grad_sky=o.affine_trans_sky.grad.numpy())
        for k, v in rec.items():
            assert v.dtype == np.float32 and np.all(np.isfinite(v)), (c["name"], k)
            arrays["%s/%s" % (c["name"], k)] = v
        a, s = params(c["kind"])
        rows.append(dict(c, id=int(o.get_id(camera)), num_corrections=N,
                         sha256=ct.sha256(image_np, g_np, a, s)))
        print("%-32s id %d  out %s" % (c["name"], rows[-1]["id"], out.shape))
    source = ("lib/models/color_correction.py (%s) of the reference, cut with ast and executed on CPU torch %s over a "
              "stub of the explicit variant" % (", ".join(METHODS), torch.__version__.split("+")[0]))
    with open(os.path.join(HERE, "ref_color_correction.json"), "w") as f:
        json.dump({"source": source, "cases": rows}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_color_correction.npz"), **arrays)
    print("wrote %d cases, %d arrays" % (len(rows), len(arrays)))


if __name__ == "__main__":
    main(sys.argv[1])
