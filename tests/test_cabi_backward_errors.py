"""The backward entry points of the C ABI -- grpg_backward, grpg_backward_composed, grpg_backward_composed_features,
grpg_backward_composed_objects, grpg_compose_features_backward, and grpg_object_alpha_forward, which shares their
state check -- answer every case below with the same (return code, grpg_last_error() text) pair as the library did
before the backward half of csrc/api.hip was moved onto one request struct: which check fires first is part of the
contract of every entry, and so is what becomes of a pending pose binding.

ctypes only (no _C); the signatures are read from the header.  Without a device every entry answers
GRPG_ERR_NO_DEVICE whatever its arguments (the pointers are host memory nobody dereferences).  On a device the blobs
of one real training frame are made through the library handle under test -- two segments of 32 Gaussians, the second
rigid, M = 4, D = 1, 64 x 48 pixels, S = 2 with normals, plus its object-alpha workspace -- and one flat frame of
P = 64 for grpg_backward; every case changes one thing (a few: two things, to record the order of the checks) from a
call that passes.  A refused case returns before anything is enqueued; a case that passes must leave every output
finite that was poisoned with NaN before the call.

The expected pairs (tests/golden/cabi_backward_errors.json) were recorded from a library built from commit 8e4fb9e
("Add use_mlp colour correction: pose to 3x4 matrices in one HIP launch"), the commit BEFORE the move
(tools/build_lib_from_commit.py), with this file run as a script:
    python tests/test_cabi_backward_errors.py <libgrpg_rasterizer.so of that commit> <json>
once without a device ("no_device") and once on an MI355X ("device").
"""
import ctypes
import functools
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cabi_backward_errors.json")

COMPOSED = ["grpg_backward_composed", "grpg_backward_composed_features", "grpg_backward_composed_objects"]
ENTRIES = ["grpg_backward"] + COMPOSED + ["grpg_compose_features_backward", "grpg_object_alpha_forward"]
FORWARDS = ["grpg_forward_flags", "grpg_forward_composed_features"]     # make the device frames
OK, NO_DEVICE = 0, -2
GRPG_FORWARD_NO_BACKWARD = 1
GRPG_MAX_SEGMENTS = 1024
NSEG, COUNT, P, M, D, W, H, S, NORMALS = 2, 32, 64, 4, 1, 64, 48, 2, 1
F = 3 * NORMALS + S

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
SEG_ARRAYS = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest")


class Segment(ctypes.Structure):     # grpg_model_segment
    _fields_ = [(f, ctypes.c_void_p) for f in SEG_ARRAYS] + [
        ("count", ctypes.c_int), ("fourier_dim", ctypes.c_int), ("rigid", ctypes.c_int),
        ("obj_rot", ctypes.c_float * 4), ("obj_trans", ctypes.c_float * 3), ("idft", ctypes.c_float * 8),
        ("flip", ctypes.c_void_p)]


class SegmentGrad(ctypes.Structure):     # grpg_model_segment_grad
    _fields_ = [(f, ctypes.c_void_p) for f in SEG_ARRAYS]


def _signatures(names):
    """entry -> [(parameter name, ctypes type)], read from the header's declarations."""
    text = open(HEADER).read()
    sigs = {}
    for name in names:
        m = re.search(r"GRPG_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, "no declaration of %s in the header" % name
        params = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            pname = re.search(r"(\w+)$", p).group(1)
            ctype = p[:-len(pname)].strip()
            if ctype == "grpg_alloc_fn":
                t = ALLOC_FN
            elif ctype.endswith("*"):
                t = ctypes.c_void_p
            else:
                t = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float}[ctype]
            params.append((pname, t))
        sigs[name] = params
    return sigs


def _load(lib_path):
    import torch  # noqa: F401  (loads the libamdhip64 the library links against, as test_cabi_exports does)
    lib = ctypes.CDLL(lib_path)
    sigs = _signatures(ENTRIES + FORWARDS)
    for name, params in sigs.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, [t for _, t in params]
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_object_alpha_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_object_alpha_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.grpg_bind_device_poses.restype = ctypes.c_int
    lib.grpg_bind_device_poses.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.grpg_device_poses_bound.restype = ctypes.c_int
    return lib, sigs


def _invoke(lib, sigs, name, vals):
    args = []
    for pname, t in sigs[name]:
        assert pname in vals, (name, pname)
        args.append(vals[pname])
    rc = getattr(lib, name)(*args)
    return [rc, lib.grpg_last_error().decode()]


def _null_args(sigs, name):
    return {pname: (None if t is ctypes.c_void_p else 0) for pname, t in sigs[name]}


# ---- the frames the cases start from ----

class HostFrame:
    """No device: every pointer is host memory that no call gets as far as reading."""

    def __init__(self):
        self.keep = ctypes.create_string_buffer(4096)
        ptr = ctypes.addressof(self.keep)
        self.real = False
        self.seg_arrays = [{f: ptr for f in SEG_ARRAYS} for _ in range(NSEG)]
        self.grad_arrays = [{f: ptr for f in SEG_ARRAYS} for _ in range(NSEG)]
        self.semantic_grads = [ptr] * NSEG
        self.rotation_grads = [ptr] * NSEG
        names = ("background viewmatrix projmatrix campos cam_pos radii alphas geom_buffer binning_buffer image_buffer "
                 "feature_buffer dL_dpix dL_dpix_depth dL_dalphas dL_dpix_features dL_dfeatures dL_dmean2D dL_dposes "
                 "alpha_object out_alpha_object workspace dL_dalpha_object eval_geom flat_geom flat_binning flat_image "
                 "flat_eval_geom flat_moved_geom flat_zero_geom means3D shs colors_precomp cov3D_precomp scales "
                 "rotations flat_alphas flat_radii semantics dL_dpix_semantic dL_dsemantic dL_dconic dL_dopacity "
                 "dL_dcolor dL_ddepth dL_dmean3D dL_dcov3D dL_dsh dL_dscale dL_drot").split()
        self.ptr = {n: ptr for n in names}
        self.R = self.flat_R = 100
        self.tan_fovx = self.tan_fovy = 0.5

    def prepare(self):
        pass

    def unwritten(self, names):
        return []


class DeviceFrame:
    """One composed training frame (feature planes, object-alpha workspace) and one flat training frame, made
    through the library under test; every tensor the backward entries read or write."""

    def __init__(self, lib, sigs):
        import torch
        from gaussianrpg_amd import harness as hz
        self.real, self.torch = True, torch
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(7)
        sc = hz.toy_scene(P, seed=21, sh_degree=D)
        cam = hz.trajectory_camera(0, W=W, H=H)
        self.tan_fovx, self.tan_fovy = cam.tanfovx, cam.tanfovy
        t = {}                                              # name -> device tensor (kept alive here)

        def put(name, x):
            t[name] = x.float().contiguous().to(dev) if x.is_floating_point() else x.contiguous().to(dev)
            return t[name]
        put("background", torch.tensor([0.2, 0.1, 0.3]))
        put("viewmatrix", cam.viewmatrix), put("projmatrix", cam.projmatrix), put("campos", cam.campos)
        t["cam_pos"] = t["campos"]
        # raw parameters of the two models: the second is an actor, posed by a small rigid motion
        opac = sc.opacity.clamp(1e-3, 1 - 1e-3)
        raw = dict(xyz=sc.means3D, scaling=sc.scales.log(), rotation=sc.rotations, opacity=(opac / (1 - opac)).log(),
                   features_dc=sc.shs[:, :1], features_rest=sc.shs[:, 1:])
        self.seg_arrays, self.grad_arrays, self.semantic_grads, self.rotation_grads, sem_in = [], [], [], [], []
        self.outputs = {}                                   # output name -> tensor, poisoned before every call
        for i in range(NSEG):
            rows = slice(i * COUNT, (i + 1) * COUNT)
            self.seg_arrays.append({f: put("seg%d_%s" % (i, f), raw[f][rows]).data_ptr() for f in SEG_ARRAYS})
            grads = {}
            for f in SEG_ARRAYS:
                grads[f] = self.outputs["grad%d_%s" % (i, f)] = torch.empty_like(t["seg%d_%s" % (i, f)])
            self.grad_arrays.append({f: x.data_ptr() for f, x in grads.items()})
            sem_in.append(put("seg%d_semantic" % i, torch.randn(COUNT, S, generator=g)).data_ptr())
            self.outputs["seg%d_dL_dsemantic" % i] = torch.empty(COUNT, S, device=dev)
            self.semantic_grads.append(self.outputs["seg%d_dL_dsemantic" % i].data_ptr())
            self.outputs["seg%d_dL_drotation" % i] = torch.empty(COUNT, 4, device=dev)
            self.rotation_grads.append(self.outputs["seg%d_dL_drotation" % i].data_ptr())
        for name, shape in (("dL_dmean2D", (P, 3)), ("dL_dposes", (NSEG, 8)), ("dL_dconic", (P, 4)),
                            ("dL_dopacity", (P, 1)), ("dL_dcolor", (P, 3)), ("dL_ddepth", (P,)),
                            ("dL_dmean3D", (P, 3)), ("dL_dcov3D", (P, 6)), ("dL_dsh", (P, M, 3)), ("dL_dscale", (P, 3)),
                            ("dL_drot", (P, 4)), ("out_alpha_object", (H, W))):
            self.outputs[name] = torch.empty(shape, device=dev)
        # scratch the blend backward ADDS to: zero-filled before every call
        self.zeroed = {"dL_dfeatures": torch.empty(P, F, device=dev), "dL_dsemantic": torch.empty(P, S, device=dev)}
        for name, shape in (("dL_dpix", (3, H, W)), ("dL_dpix_depth", (1, H, W)), ("dL_dalphas", (1, H, W)),
                            ("dL_dpix_features", (F, H, W)), ("dL_dalpha_object", (H, W)),
                            ("dL_dpix_semantic", (S, H, W)), ("semantics", (P, S)), ("colors_precomp", (P, 3))):
            put(name, torch.randn(shape, generator=g))
        put("cov3D_precomp", 0.01 * torch.eye(3)[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].repeat(P, 1))
        for f, x in (("means3D", sc.means3D), ("shs", sc.shs), ("scales", sc.scales), ("rotations", sc.rotations),
                     ("opacities", sc.opacity)):
            put(f, x)

        segs = _segments(self.seg_arrays, None)
        self.keep = [segs, (ctypes.c_void_p * NSEG)(*sem_in)]
        planes = {n: torch.empty(c, H, W, device=dev) for n, c in
                  (("out_color", 3), ("out_depth", 1), ("out_alpha", 1), ("out_features", F))}

        def forward(name, flags, **more):
            blobs = {k: [] for k in ("geometry", "binning", "image", "feature")}
            vals = dict(hip_stream=None, debug=0, flags=flags, scale_modifier=1.0, width=W, height=H, D=D, M=M,
                        tan_fovx=self.tan_fovx, tan_fovy=self.tan_fovy, prefiltered=0,
                        radii=torch.empty(P, dtype=torch.int32, device=dev))
            for k in ("background", "viewmatrix", "projmatrix", "cam_pos"):
                vals[k] = t[k].data_ptr()
            for k, lst in blobs.items():
                def alloc(nbytes, _user, lst=lst):
                    lst.append(torch.empty(int(nbytes), dtype=torch.uint8, device=dev))
                    return lst[-1].data_ptr()
                vals[k + "_alloc"], vals[k + "_user"] = ALLOC_FN(alloc), None
            vals.update({k: x.data_ptr() for k, x in planes.items()})
            vals.update(more)
            ptrs = {k: (x.data_ptr() if isinstance(x, torch.Tensor) else x) for k, x in vals.items()}
            rc, err = _invoke(lib, sigs, name, ptrs)
            torch.cuda.synchronize()
            assert rc >= 0, (name, rc, err)
            out = {k: lst[-1] for k, lst in blobs.items() if lst}     # (the binning blob is re-carved after an overflow)
            out.update(R=rc, radii=vals["radii"], alphas=planes["out_alpha"].clone())
            return out

        composed = dict(segments=ctypes.addressof(segs), num_segments=NSEG, seg_semantic=ctypes.addressof(self.keep[1]),
                        S=S, normals=NORMALS)
        fr = forward("grpg_forward_composed_features", 0, **composed)
        ev = forward("grpg_forward_composed_features", GRPG_FORWARD_NO_BACKWARD, **composed)
        flat = dict(P=P, S=0, semantics=None, out_semantic=None, colors_precomp=None, cov3D_precomp=None,
                    means3D=t["means3D"], shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
                    rotations=t["rotations"])
        ff = forward("grpg_forward_flags", 0, **flat)
        fe = forward("grpg_forward_flags", GRPG_FORWARD_NO_BACKWARD, **flat)
        assert fr["R"] > 0 and ff["R"] > 0
        self.R, self.flat_R = fr["R"], ff["R"]
        t.update(geom_buffer=fr["geometry"], binning_buffer=fr["binning"], image_buffer=fr["image"],
                 feature_buffer=fr["feature"], radii=fr["radii"], alphas=fr["alphas"], eval_geom=ev["geometry"],
                 flat_geom=ff["geometry"], flat_binning=ff["binning"], flat_image=ff["image"], flat_radii=ff["radii"],
                 flat_alphas=ff["alphas"], flat_eval_geom=fe["geometry"], flat_moved_geom=ff["geometry"].clone(),
                 flat_zero_geom=torch.zeros_like(ff["geometry"]))
        # the object-alpha plane of the composed frame and the workspace its backward reads (one spare byte behind it:
        # the misaligned case points there)
        nbytes = lib.grpg_object_alpha_workspace_bytes(W, H)
        t["workspace"] = torch.zeros(nbytes + 4, dtype=torch.uint8, device=dev)
        t["alpha_object"] = torch.empty(H, W, device=dev)
        rc, err = _invoke(lib, sigs, "grpg_object_alpha_forward", dict(
            P=P, width=W, height=H, layer_class=None, geom_buffer=t["geom_buffer"].data_ptr(),
            binning_buffer=t["binning_buffer"].data_ptr(), image_buffer=t["image_buffer"].data_ptr(),
            out_alpha_object=t["alpha_object"].data_ptr(), workspace=t["workspace"].data_ptr(), hip_stream=None))
        torch.cuda.synchronize()
        assert rc == OK, err
        self.tensors = t
        self.ptr = {k: x.data_ptr() for k, x in t.items()}
        self.ptr.update({k: x.data_ptr() for k, x in self.outputs.items()})
        self.ptr.update({k: x.data_ptr() for k, x in self.zeroed.items()})

    def prepare(self):
        for x in self.outputs.values():
            x.fill_(float("nan"))
        for x in self.zeroed.values():
            x.zero_()

    def unwritten(self, names):
        self.torch.cuda.synchronize()
        both = dict(self.outputs, **self.zeroed)
        return [n for n in names if not bool(self.torch.isfinite(both[n]).all())]


def _segments(arrays, spec):
    """the host segment array: `arrays` per segment, changed by spec (a list of per-segment field overrides)"""
    spec = spec if spec is not None else [{}] * NSEG
    segs = (Segment * max(len(spec), 1))()
    for i, (s, change) in enumerate(zip(segs, spec)):
        for f, x in arrays[min(i, NSEG - 1)].items():
            setattr(s, f, x)
        s.count, s.fourier_dim, s.rigid = COUNT, 1, int(i > 0)
        s.obj_rot[0], s.idft[0] = 1.0, 1.0
        if i > 0:
            s.obj_trans[0], s.obj_trans[2] = 0.25, 0.5
        for k, x in change.items():
            setattr(s, k, x)
    return segs


# ---- the cases: overrides of a passing call.  "seg" / "grad": per-segment field overrides of the segment / gradient
# tables; a string value names another pointer of the frame; "written": the outputs a passing call must leave finite
# (default: the entry's own list).  A case runs for the entries that have every parameter it overrides. ----

NULLABLE = ("dL_dpix", "dL_dpix_depth", "dL_dalphas", "alphas", "dL_dmean2D", "dL_dposes", "radii", "background",
            "viewmatrix", "projmatrix", "campos")
COMPOSED_CASES = {
    "valid": {},
    "zero_segments": dict(num_segments=0),
    "too_many_segments": dict(num_segments=GRPG_MAX_SEGMENTS + 1),
    "null_segments": dict(segments=None),
    "segment_count_zero": dict(seg=[{}, dict(count=0)]),
    "D_negative": dict(D=-1),
    "D_4": dict(D=4),
    "D_beyond_M": dict(D=2),
    "null_grads": dict(grads=None),
    "null_geom_buffer": dict(geom_buffer=None),
    "null_binning_buffer": dict(binning_buffer=None),
    "null_image_buffer": dict(image_buffer=None),
    "evaluation_blob": dict(geom_buffer="eval_geom"),
    "grad_null_xyz": dict(grad=[{}, dict(xyz=None)]),
    "grad_null_features_rest": dict(grad=[dict(features_rest=None), {}]),
    "M_1": dict(M=1, D=0, written_without="features_rest"),
    "M_1_grad_null_features_rest": dict(M=1, D=0, grad=[dict(features_rest=None), dict(features_rest=None)],
                                        written_without="features_rest"),
    "debug": dict(debug=1),
    "S_negative": dict(S=-1),
    "normals_2": dict(normals=2),
    "S_33": dict(S=33),
    "null_feature_buffer": dict(feature_buffer=None),
    "null_dL_dpix_features": dict(dL_dpix_features=None),
    "null_dL_dfeatures": dict(dL_dfeatures=None),
    "null_seg_dL_dsemantic": dict(seg_dL_dsemantic=None, written_without="dL_dsemantic"),
    "F_0_without_feature_pointers": dict(S=0, normals=0, feature_buffer=None, dL_dpix_features=None, dL_dfeatures=None,
                                         written_without=("dL_dsemantic", "dL_dfeatures")),
    "null_alpha_object": dict(alpha_object=None),
    "null_workspace": dict(workspace=None),
    "null_dL_dalpha_object": dict(dL_dalpha_object=None),
    "workspace_bit_0": dict(workspace=("workspace", 1)),
    "width_0": dict(width=0, only="grpg_backward_composed_objects"),
    # two things wrong at once: which check answers
    "null_grads_and_S_negative": dict(grads=None, S=-1),
    "null_grads_and_zero_segments": dict(grads=None, num_segments=0),
    "null_alpha_object_and_zero_segments": dict(alpha_object=None, num_segments=0),
    "null_alpha_object_and_S_negative": dict(alpha_object=None, S=-1),
    "evaluation_blob_and_null_dL_dpix": dict(geom_buffer="eval_geom", dL_dpix=None),
    "null_geom_buffer_and_null_dL_dpix": dict(geom_buffer=None, dL_dpix=None),
    "S_33_and_segment_count_zero": dict(S=33, seg=[{}, dict(count=0)]),
    "null_feature_buffer_and_D_4": dict(feature_buffer=None, D=4),
    "null_dL_dpix_and_grad_null_xyz": dict(dL_dpix=None, grad=[{}, dict(xyz=None)]),
}
COMPOSED_CASES.update({"null_" + n: {n: None} for n in NULLABLE})

FEATURE_BACKWARD_CASES = {
    "valid": {},
    "zero_segments": dict(num_segments=0),
    "too_many_segments": dict(num_segments=GRPG_MAX_SEGMENTS + 1),
    "segment_count_zero": dict(seg=[{}, dict(count=0)]),
    "S_negative": dict(S=-1),
    "normals_2": dict(normals=2),
    "null_cam_pos": dict(cam_pos=None),
    "null_cam_pos_without_normals": dict(cam_pos=None, normals=0),
    "F_0": dict(S=0, normals=0, written=()),
    "null_dL_dfeatures": dict(dL_dfeatures=None),
    "null_dL_dposes": dict(dL_dposes=None),
    "null_seg_arrays": dict(seg_dL_dsemantic=None, seg_dL_drotation=None, written=()),
    "null_dL_dfeatures_and_S_negative": dict(dL_dfeatures=None, S=-1),
}

OBJECT_ALPHA_CASES = {
    "valid": {},
    "P_negative": dict(P=-1),
    "P_0": dict(P=0),
    "P_0_without_blobs": dict(P=0, geom_buffer=None, binning_buffer=None, image_buffer=None),
    "width_0": dict(width=0),
    "height_negative": dict(height=-1),
    "null_out_alpha_object": dict(out_alpha_object=None),
    "null_workspace": dict(workspace=None),
    "workspace_bit_0": dict(workspace=("workspace", 1)),
    "null_geom_buffer": dict(geom_buffer=None),
    "null_binning_buffer": dict(binning_buffer=None),
    "null_image_buffer": dict(image_buffer=None),
    "evaluation_blob": dict(geom_buffer="eval_geom"),
    "evaluation_blob_and_null_out_alpha_object": dict(geom_buffer="eval_geom", out_alpha_object=None),
    "null_geom_buffer_and_width_0": dict(geom_buffer=None, width=0),
}

FLAT_OUT = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_ddepth", "dL_dmean3D", "dL_dcov3D", "dL_dsh",
            "dL_dscale", "dL_drot")
SEMANTIC = dict(S=S, semantics="semantics", dL_dpix_semantic="dL_dpix_semantic", dL_dsemantic="dL_dsemantic")
FLAT_CASES = {
    "valid": {},
    "P_0": dict(P=0, written=()),
    "P_negative": dict(P=-1, written=()),
    "null_geom_buffer": dict(geom_buffer=None),
    "null_binning_buffer": dict(binning_buffer=None),
    "null_image_buffer": dict(image_buffer=None),
    # the pairs tests/test_gpu_cabi_backward.py looks at
    "null_dL_dsh": dict(dL_dsh=None),
    "null_dL_dscale": dict(dL_dscale=None),
    "null_dL_drot": dict(dL_drot=None),
    "null_dL_dmean3D": dict(dL_dmean3D=None),
    "evaluation_blob": dict(geom_buffer="flat_eval_geom"),
    "moved_blob": dict(geom_buffer="flat_moved_geom"),
    "no_blob": dict(geom_buffer="flat_zero_geom"),
    "cov3D_precomp_without_dL_dcov3D": dict(cov3D_precomp="cov3D_precomp", dL_dcov3D=None),
    # colors_precomp / cov3D_precomp
    "optional_outputs_null": dict(dL_dconic=None, dL_ddepth=None, dL_dcolor=None, dL_dcov3D=None,
                                  written_without=("dL_dconic", "dL_ddepth", "dL_dcolor", "dL_dcov3D")),
    "colors_precomp": dict(colors_precomp="colors_precomp", written_without="dL_dsh"),
    "colors_precomp_without_shs": dict(colors_precomp="colors_precomp", shs=None, dL_dsh=None, written_without="dL_dsh"),
    "colors_precomp_without_dL_dcolor": dict(colors_precomp="colors_precomp", dL_dcolor=None),
    "cov3D_precomp": dict(cov3D_precomp="cov3D_precomp", written_without=("dL_dscale", "dL_drot")),
    "cov3D_precomp_without_scales": dict(cov3D_precomp="cov3D_precomp", scales=None, rotations=None, dL_dscale=None,
                                         dL_drot=None, written_without=("dL_dscale", "dL_drot")),
    "both_precomp_without_their_gradients": dict(colors_precomp="colors_precomp", cov3D_precomp="cov3D_precomp",
                                                 dL_dcolor=None, dL_dcov3D=None),
    "null_shs": dict(shs=None),
    "null_scales": dict(scales=None),
    "null_rotations": dict(rotations=None),
    "null_means3D": dict(means3D=None),
    "null_campos": dict(campos=None),
    "null_dL_dpix": dict(dL_dpix=None),
    "null_alphas": dict(alphas=None),
    "null_dL_dopacity": dict(dL_dopacity=None),
    "null_radii": dict(radii=None),                       # allowed: the geometry blob keeps its own copy
    # semantics
    "S_2": dict(SEMANTIC),
    "S_33": dict(SEMANTIC, S=33),
    "S_2_null_semantics": dict(SEMANTIC, semantics=None),
    "S_2_null_dL_dpix_semantic": dict(SEMANTIC, dL_dpix_semantic=None),
    "S_2_null_dL_dsemantic": dict(SEMANTIC, dL_dsemantic=None),
    "S_33_null_semantics": dict(SEMANTIC, S=33, semantics=None),
    # debug = 1 reads the three headers back
    "debug": dict(debug=1),
    "debug_R_plus_1": dict(debug=1, R=("R", 1)),
    "debug_R_minus_1": dict(debug=1, R=("R", -1)),
    "debug_null_dL_dpix": dict(debug=1, dL_dpix=None),
    "null_dL_dsh_and_null_means3D": dict(dL_dsh=None, means3D=None),
    "evaluation_blob_and_null_dL_dpix": dict(geom_buffer="flat_eval_geom", dL_dpix=None),
}

CASES = {"grpg_backward": FLAT_CASES, "grpg_compose_features_backward": FEATURE_BACKWARD_CASES,
         "grpg_object_alpha_forward": OBJECT_ALPHA_CASES}
SPECIAL = ("seg", "grad", "written", "written_without", "only")


def _base(fr, name):
    """the arguments of a call of `name` that passes; the outputs it must write"""
    p = fr.ptr
    v = dict(num_segments=NSEG, S=S, normals=NORMALS, D=D, M=M, R=fr.R, width=W, height=H, scale_modifier=1.0,
             tan_fovx=fr.tan_fovx, tan_fovy=fr.tan_fovy, debug=0, hip_stream=None, P=P, layer_class=None)
    for n in ("background viewmatrix projmatrix campos cam_pos radii alphas geom_buffer binning_buffer image_buffer "
              "feature_buffer dL_dpix dL_dpix_depth dL_dalphas dL_dpix_features dL_dfeatures dL_dmean2D dL_dposes "
              "alpha_object out_alpha_object workspace dL_dalpha_object").split():
        v[n] = p[n]
    seg_grads = ["grad%d_%s" % (i, f) for i in range(NSEG) for f in SEG_ARRAYS]
    sem_grads = ["seg%d_dL_dsemantic" % i for i in range(NSEG)]
    if name == "grpg_backward":
        v.update(S=0, R=fr.flat_R, semantics=None, dL_dpix_semantic=None, dL_dsemantic=None, colors_precomp=None,
                 cov3D_precomp=None, geom_buffer=p["flat_geom"], binning_buffer=p["flat_binning"],
                 image_buffer=p["flat_image"], alphas=p["flat_alphas"], radii=p["flat_radii"])
        for n in ("means3D", "shs", "scales", "rotations") + FLAT_OUT[1:]:
            v[n] = p[n]
        return v, list(FLAT_OUT)
    if name == "grpg_backward_composed":
        return v, seg_grads + ["dL_dmean2D", "dL_dposes"]
    if name in COMPOSED:
        return v, seg_grads + sem_grads + ["dL_dmean2D", "dL_dposes", "dL_dfeatures"]
    if name == "grpg_compose_features_backward":
        # (dL_dfeatures is an input here: the zero-filled scratch serves; dL_dposes and the rotation gradients are
        # ADDED to, so they arrive as zeros a caller would hand in)
        return v, sem_grads
    return v, ["out_alpha_object"]


def _run_case(lib, sigs, fr, name, case):
    vals, written = _base(fr, name)
    keep = []
    params = {pname for pname, _ in sigs[name]}
    if "segments" in params:
        segs = _segments(fr.seg_arrays, case.get("seg"))
        grads = (SegmentGrad * NSEG)()
        for i, g in enumerate(grads):
            for f, x in fr.grad_arrays[i].items():
                setattr(g, f, x)
            for k, x in (case.get("grad") or [{}] * NSEG)[i].items():
                setattr(g, k, x)
        sem = (ctypes.c_void_p * NSEG)(*fr.semantic_grads)
        rot = (ctypes.c_void_p * NSEG)(*fr.rotation_grads)
        keep += [segs, grads, sem, rot]
        vals.update(segments=ctypes.addressof(segs), grads=ctypes.addressof(grads),
                    seg_dL_dsemantic=ctypes.addressof(sem), seg_dL_drotation=ctypes.addressof(rot))
    for k, x in case.items():
        if k in SPECIAL:
            continue
        if isinstance(x, tuple):                            # (name, offset): a neighbour of a value of the passing call
            x = vals[x[0]] + x[1]
        elif isinstance(x, str):
            x = fr.ptr[x]
        vals[k] = x
    fr.prepare()
    if fr.real and name == "grpg_compose_features_backward":
        for i in range(NSEG):                               # accumulated into: zeros, as a caller hands them in
            fr.outputs["seg%d_dL_drotation" % i].zero_()
        fr.outputs["dL_dposes"].zero_()
    got = _invoke(lib, sigs, name, vals)
    if got[0] == OK and fr.real:
        if "written" in case:
            written = list(case["written"])
        drop = case.get("written_without", ())
        drop = (drop,) if isinstance(drop, str) else drop
        written = [n for n in written if not any(d in n for d in drop)]
        bad = fr.unwritten(written)
        assert not bad, "%s / %s returned GRPG_OK but left NaN in %s" % (name, case, bad)
    return got


def _cases(sigs, name):
    """case id -> overrides, for the cases whose overridden parameters `name` has"""
    table = COMPOSED_CASES if name in COMPOSED else CASES[name]
    params = {pname for pname, _ in sigs[name]}
    return {cid: c for cid, c in table.items()
            if all(k in params or k in SPECIAL for k in c) and c.get("only", name) == name}


def _mode():
    import torch
    return "device" if torch.cuda.is_available() else "no_device"


@functools.lru_cache(maxsize=None)
def run_all(lib_path):
    lib, sigs = _load(lib_path)
    fr = DeviceFrame(lib, sigs) if _mode() == "device" else HostFrame()
    table = {}
    for name in ENTRIES:
        table[name] = {"all_null": _invoke(lib, sigs, name, _null_args(sigs, name))}
        for cid, case in _cases(sigs, name).items():
            table[name][cid] = _run_case(lib, sigs, fr, name, case)
    if fr.real:
        fr.torch.cuda.synchronize()
    return table


def _check(mode):
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    want = json.load(open(GOLDEN))[mode]
    got = run_all(LIB)
    assert sorted(got) == sorted(want) == sorted(ENTRIES)
    bad = []
    for name in ENTRIES:
        assert sorted(got[name]) == sorted(want[name]), name
        for cid in got[name]:
            if got[name][cid] != want[name][cid]:
                bad.append((name, cid, got[name][cid], want[name][cid]))
    assert not bad, "(entry, case, got, recorded before the move):\n" + "\n".join(map(repr, bad))
    for name in ENTRIES:
        for cid, (rc, msg) in got[name].items():
            assert (rc == OK and msg == "") or (rc < 0 and msg), (name, cid, rc, msg)
            if mode == "no_device":
                assert rc == NO_DEVICE, (name, cid, rc, msg)
    return got


def test_backward_entries_report_the_recorded_errors():
    """Without a device: the "no_device" pairs, GRPG_ERR_NO_DEVICE every one; with one: the "device" pairs."""
    _check(_mode())


def test_a_refused_composed_backward_consumes_the_pose_binding_and_a_refused_flat_one_does_not():
    lib, sigs = _load(LIB)
    rows = (ctypes.c_int * NSEG)(-1, -1)
    for name in COMPOSED + ["grpg_compose_features_backward"]:
        assert lib.grpg_bind_device_poses(None, None, rows, NSEG) == OK and lib.grpg_device_poses_bound() == 1
        rc, msg = _invoke(lib, sigs, name, _null_args(sigs, name))
        assert rc < 0 and msg, (name, rc, msg)              # no device, or no segments
        assert lib.grpg_device_poses_bound() == 0, name
    # grpg_backward and grpg_object_alpha_forward take no segments: the binding waits for a call that does
    assert lib.grpg_bind_device_poses(None, None, rows, NSEG) == OK and lib.grpg_device_poses_bound() == 1
    for name in ("grpg_backward", "grpg_object_alpha_forward"):
        rc, msg = _invoke(lib, sigs, name, dict(_null_args(sigs, name), P=P, width=W, height=H))
        assert rc < 0 and msg, (name, rc, msg)              # no device, or NULL state buffers / outputs
        assert lib.grpg_device_poses_bound() == 1, name
    name = COMPOSED[0]
    assert _invoke(lib, sigs, name, _null_args(sigs, name))[0] < 0 and lib.grpg_device_poses_bound() == 0


@pytest.mark.gpu
def test_backward_entries_validate_arguments_on_device():
    """The argument checks proper, in their recorded order -- reached only behind ensure_device -- and the calls that
    pass: GRPG_OK with every output written."""
    got = _check("device")
    for name in ENTRIES:
        assert got[name]["valid"] == [OK, ""], (name, got[name]["valid"])


if __name__ == "__main__":      # recorder: <library> <json>; merges this machine's mode into the file
    lib_path, out = sys.argv[1], sys.argv[2]
    table = json.load(open(out)) if os.path.exists(out) else {}
    table[_mode()] = run_all(os.path.abspath(lib_path))
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %s: %s cases" % (_mode(), {n: len(c) for n, c in table[_mode()].items()}))
