"""The eight forward bindings of csrc/torch_binding.cpp answer like they did before they were rebuilt from
shared helpers: the same exception class and text for a bad call -- and, where several arguments are wrong,
the same one of them -- and the same layout (dtype, shape, device of every returned element) for a good one.

No plane is compared numerically here: the rest of the suite compares every plane with the oracle and with
the unfused chains.  tests/golden/binding_forward_contract.json holds two tables,
    errors  : entry -> case -> [exception class name, first line of str(e)]   (later lines may carry source
              locations)
    layouts : entry -> combination -> [[dtype, shape, device type] per tensor, [type name] per other value]
recorded from the `_C` of the commit BEFORE the bindings were rebuilt, with this file run as a script on an
MI355X:
    python tests/test_binding_forward_contract.py <package dir of that build> <json>
The cases whose first failing check comes before the device check are made of CPU tensors and run without a
device; the rest carry the gpu marker.
"""
import glob
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_forward_contract.json")

P0, H, W, DEGREE, M = 64, 48, 64, 1, 4       # 64 Gaussians / two models of 32, a 64x48 image, degree 1
FLAT = ("rasterize_gaussians", "rasterize_gaussians_eval", "rasterize_gaussians_eval_deferred")
LAYERS, FRAME = "rasterize_gaussians_layers", "rasterize_gaussians_frame"
COMPOSED, COMPOSED_LAYERS = "rasterize_gaussians_composed", "rasterize_gaussians_composed_layers"
COMPOSED_FRAME = "rasterize_gaussians_composed_frame"
ALL_COMPOSED = (COMPOSED, COMPOSED_LAYERS, COMPOSED_FRAME)
ENTRIES = FLAT + (LAYERS, FRAME) + ALL_COMPOSED
LISTS = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest", "flip")


def _empty():
    return torch.Tensor([])


def _camera(dev):
    """view = identity (the Gaussians sit in front of it), a perspective projection with tan(fov/2) = 0.5."""
    zn, zf = 0.01, 100.0
    proj = torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, zf / (zf - zn), -(zf * zn) / (zf - zn)],
                         [0, 0, 1.0, 0]])
    return dict(viewmatrix=torch.eye(4, device=dev), projmatrix=proj.t().contiguous().to(dev),
                tan_fovx=0.5, tan_fovy=0.5, image_height=H, image_width=W, campos=torch.zeros(3, device=dev))


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * torch.tensor([2.0, 1.5, 4.0]) + torch.tensor([-1.0, -0.75, 2.0])
    return xyz, g


def _sky(dev):
    g = torch.Generator().manual_seed(7)
    return dict(sky_cube=torch.rand(6, 8, 8, 3, generator=g).to(dev), ray_matrix=torch.eye(3).reshape(9),
                sky_fill=0.0, clamp=True, want_planes=True, want_rgb8=True, truncate=True, out_rgb8=None)


def flat_args(dev, entry, P=P0, S=0, layered=False):
    """Arguments of a valid call of a flat binding, by name, in the binding's positional order."""
    cam = _camera(dev)
    xyz, g = _points(P, 1)
    t = dict(background=torch.tensor([0.1, 0.2, 0.3], device=dev), means3D=xyz.to(dev), colors=_empty(),
             semantics=torch.rand(P, S, generator=g).to(dev), opacity=torch.full((P, 1), 0.5, device=dev),
             scales=torch.full((P, 3), 0.05, device=dev),
             rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1).to(dev), scale_modifier=1.0,
             cov3D_precomp=_empty(), sh=(torch.rand(P, M, 3, generator=g) - 0.5).to(dev), degree=DEGREE,
             prefiltered=False, debug=False, **cam)
    if entry in FLAT:
        order = ("background means3D colors semantics opacity scales rotations scale_modifier cov3D_precomp "
                 "viewmatrix projmatrix tan_fovx tan_fovy image_height image_width sh degree campos prefiltered debug")
        return {k: t[k] for k in order.split()}
    on = layered or entry == LAYERS
    t["layer_background"] = torch.ones(3, device=dev) if on else _empty()
    t["layer_class"] = (torch.arange(P) % 2).to(torch.uint8).to(dev) if on else _empty()
    order = ("background layer_background layer_class means3D colors opacity scales rotations scale_modifier "
             "cov3D_precomp viewmatrix projmatrix tan_fovx tan_fovy image_height image_width sh degree campos debug")
    a = {k: t[k] for k in order.split()}
    if entry == FRAME:
        a.update(_sky(dev))
    return a


def composed_args(dev, entry, layered=False):
    """Two models of 32: a static one, and a rigid actor with fourier_dim 2 and a flip mask."""
    cam = _camera(dev)
    a = dict(background=torch.tensor([0.1, 0.2, 0.3], device=dev))
    if entry != COMPOSED:
        on = layered or entry == COMPOSED_LAYERS
        a["layer_background"] = torch.ones(3, device=dev) if on else _empty()
        a["object_model"] = torch.empty(0, dtype=torch.uint8)
    if entry == COMPOSED_FRAME:
        a["layered"] = layered
    for name in LISTS:
        a[name] = []
    for i, F in enumerate((1, 2)):
        xyz, g = _points(32, 10 + i)
        a["xyz"].append(xyz.to(dev))
        a["scaling"].append(torch.full((32, 3), -3.0, device=dev))
        a["rotation"].append(torch.tensor([[1.0, 0, 0, 0]]).repeat(32, 1).to(dev))
        a["opacity"].append(torch.zeros(32, 1, device=dev))
        a["features_dc"].append((torch.rand(32, F, 3, generator=g) - 0.5).to(dev))
        a["features_rest"].append((torch.rand(32, M - 1, 3, generator=g) - 0.5).to(dev))
        a["flip"].append((torch.arange(32) % 3 == 0).to(dev) if i else torch.empty(0, dtype=torch.bool))
    a["poses"] = torch.tensor([[0.0] * 8, [1.0, 1, 0, 0, 0, 0.1, 0, 0.2]])
    a["idft"] = torch.tensor([[1.0] + [0.0] * 7, [1.0, 0.5] + [0.0] * 6])
    a["scale_modifier"] = 1.0
    for k in ("viewmatrix", "projmatrix", "tan_fovx", "tan_fovy", "image_height", "image_width"):
        a[k] = cam[k]
    a.update(degree=DEGREE, campos=cam["campos"], debug=False)
    if entry == COMPOSED:
        a["for_backward"] = False
    if entry == COMPOSED_FRAME:
        a.update(_sky(dev))
    return a


def base_args(dev, entry, **kw):
    return composed_args(dev, entry, **kw) if entry in ALL_COMPOSED else flat_args(dev, entry, **kw)


# ---- a. errors ------------------------------------------------------------------------------------------------
def _set(**values):
    """A case that replaces arguments; a callable value is given the argument dict (for device placement)."""
    def mutate(a):
        for k, v in values.items():
            a[k] = v(a) if callable(v) else v
    return mutate


def _f64(name):
    return lambda a: a[name].double()


def _no_frame():
    return dict(want_planes=False, want_rgb8=False)


def _bad_cube(a):
    return a["sky_cube"][:, :, :4]                                   # [6,8,4,3]: not square


def _shorter(name):
    return lambda a: a[name][:-1]


def _model1(name, fn):
    return lambda a: [a[name][0], fn(a[name][1])]


# case -> (entries, keyword arguments of base_args, mutation).  CPU_CASES are built from CPU tensors and stop at or
# before the device check; GPU_CASES are built on the device.  "double_*": two arguments are wrong, the text
# says which check comes first.
CPU_CASES = {
    "cpu_means3D": (FLAT + (LAYERS, FRAME), {}, _set()),
    "double_cpu_means3D_wrong_shape": (FLAT + (LAYERS, FRAME), {}, _set(means3D=torch.zeros(P0, 4))),
    "double_cpu_means3D_float64": (FLAT + (LAYERS, FRAME), {}, _set(means3D=_f64("means3D"))),
    "double_cpu_means3D_and_no_frame": ((FRAME,), {}, _set(**_no_frame())),
    "flip_list_short": (ALL_COMPOSED, {}, _set(flip=_shorter("flip"))),
    "no_models": (ALL_COMPOSED, {}, _set(**{k: [] for k in LISTS})),
    "scaling_list_short": (ALL_COMPOSED, {}, _set(scaling=_shorter("scaling"))),
    "poses_wrong_shape": (ALL_COMPOSED, {}, _set(poses=torch.zeros(2, 7))),
    "poses_float64": (ALL_COMPOSED, {}, _set(poses=_f64("poses"))),
    "idft_wrong_shape": (ALL_COMPOSED, {}, _set(idft=torch.zeros(2, 4))),
    "cpu_models": (ALL_COMPOSED, {}, _set()),
    "double_list_lengths_and_bad_poses": (ALL_COMPOSED, {}, _set(opacity=_shorter("opacity"),
                                                                  poses=torch.zeros(3, 8))),
    "double_bad_idft_and_no_frame": ((COMPOSED_FRAME,), {}, _set(idft=torch.zeros(2, 4), **_no_frame())),
}
_FLAT_ALL = FLAT + (LAYERS, FRAME)
_EVERY = ENTRIES
_LAYERED = (LAYERS, FRAME)
_C_LAYERED = (COMPOSED_LAYERS, COMPOSED_FRAME)
_FRAMES = (FRAME, COMPOSED_FRAME)
GPU_CASES = {
    "means3D_wrong_shape": (_FLAT_ALL, {}, _set(means3D=lambda a: a["means3D"][:, :2])),
    "means3D_float64": (_FLAT_ALL, {}, _set(means3D=_f64("means3D"))),
    "semantics_1d": (FLAT, {}, _set(semantics=lambda a: a["means3D"][:, 0])),
    "double_means3D_float64_and_semantics_1d": (FLAT, {}, _set(means3D=_f64("means3D"),
                                                               semantics=lambda a: a["means3D"][:, 0])),
    "background_float64": (_EVERY, {}, _set(background=_f64("background"))),
    "opacity_on_host": (_FLAT_ALL, {}, _set(opacity=lambda a: a["opacity"].cpu())),
    "projmatrix_on_host": (_EVERY, {}, _set(projmatrix=lambda a: a["projmatrix"].cpu())),
    "empty_viewmatrix": (_EVERY, {}, _set(viewmatrix=_empty())),
    "empty_background": (_EVERY, {}, _set(background=_empty())),
    "image_width_0": (_EVERY, {}, _set(image_width=0)),
    "sh_degree_beyond_M": (_EVERY, {}, _set(degree=3)),
    "double_float64_background_and_campos": (_EVERY, {}, _set(background=_f64("background"), campos=_f64("campos"))),
    "double_float64_scales_and_empty_campos": (_FLAT_ALL, {}, _set(scales=_f64("scales"), campos=_empty())),
    # layered: the per-Gaussian class (flat) / the per-model class (composed) and the layers' background
    "layer_class_wrong_size": (_LAYERED, dict(layered=True), _set(layer_class=lambda a: a["layer_class"][:-1])),
    "layer_class_float": (_LAYERED, dict(layered=True), _set(layer_class=lambda a: a["layer_class"].float())),
    "layer_class_on_host": (_LAYERED, dict(layered=True), _set(layer_class=lambda a: a["layer_class"].cpu())),
    "empty_layer_background": (_LAYERED + _C_LAYERED, dict(layered=True), _set(layer_background=_empty())),
    "layer_background_float64": (_LAYERED + _C_LAYERED, dict(layered=True),
                                 _set(layer_background=_f64("layer_background"))),
    "double_layer_class_wrong_size_and_empty_layer_background": (
        _LAYERED, dict(layered=True), _set(layer_class=lambda a: a["layer_class"][:-1], layer_background=_empty())),
    "double_layer_class_wrong_size_and_float64_opacity": (
        _LAYERED, dict(layered=True), _set(layer_class=lambda a: a["layer_class"][:-1], opacity=_f64("opacity"))),
    "object_model_wrong_size": (_C_LAYERED, dict(layered=True), _set(object_model=torch.ones(3, dtype=torch.uint8))),
    "object_model_float": (_C_LAYERED, dict(layered=True), _set(object_model=torch.ones(2))),
    "object_model_on_device": (_C_LAYERED, dict(layered=True),
                               _set(object_model=lambda a: torch.ones(2, dtype=torch.uint8).to(a["background"].device))),
    "double_object_model_wrong_size_and_empty_layer_background": (
        _C_LAYERED, dict(layered=True), _set(object_model=torch.ones(3, dtype=torch.uint8), layer_background=_empty())),
    "double_object_model_wrong_size_and_float64_campos": (
        _C_LAYERED, dict(layered=True), _set(object_model=torch.ones(3, dtype=torch.uint8), campos=_f64("campos"))),
    # the frame epilogue
    "no_planes_no_rgb8": (_FRAMES, {}, _set(**_no_frame())),
    "sky_cube_malformed": (_FRAMES, {}, _set(sky_cube=_bad_cube)),
    "sky_cube_on_host": (_FRAMES, {}, _set(sky_cube=lambda a: a["sky_cube"].cpu())),
    "ray_matrix_8_values": (_FRAMES, {}, _set(ray_matrix=torch.zeros(8))),
    "ray_matrix_float64": (_FRAMES, {}, _set(ray_matrix=_f64("ray_matrix"))),
    "out_wrong_size": (_FRAMES, {}, _set(out_rgb8=lambda a: torch.empty(H, W, 4, dtype=torch.uint8,
                                                                        device=a["background"].device))),
    "out_float": (_FRAMES, {}, _set(out_rgb8=lambda a: torch.empty(H, W, 3, device=a["background"].device))),
    "out_pageable_host": (_FRAMES, {}, _set(out_rgb8=torch.empty(H, W, 3, dtype=torch.uint8))),
    "out_without_rgb8_is_ignored_then_width_0": (_FRAMES, {}, _set(out_rgb8=torch.empty(5), want_rgb8=False,
                                                                   image_width=0)),
    "double_no_frame_and_malformed_sky_cube": (_FRAMES, {}, _set(sky_cube=_bad_cube, **_no_frame())),
    "double_out_wrong_size_and_bad_ray_matrix": (
        _FRAMES, {}, _set(ray_matrix=torch.zeros(8),
                          out_rgb8=lambda a: torch.empty(H, W, 4, dtype=torch.uint8, device=a["background"].device))),
    "double_malformed_sky_cube_and_empty_campos": (_FRAMES, {}, _set(sky_cube=_bad_cube, campos=_empty())),
    "double_empty_layer_background_and_empty_campos": (_FRAMES, dict(layered=True),
                                                       _set(layer_background=_empty(), campos=_empty())),
    "double_means3D_float64_and_no_frame": ((FRAME,), {}, _set(means3D=_f64("means3D"), **_no_frame())),
    "double_no_frame_and_layer_class_wrong_size": (
        (FRAME,), dict(layered=True), _set(layer_class=lambda a: a["layer_class"][:-1], **_no_frame())),
    "double_no_frame_and_object_model_wrong_size": (
        (COMPOSED_FRAME,), dict(layered=True), _set(object_model=torch.ones(3, dtype=torch.uint8), **_no_frame())),
    "object_model_unchecked_when_not_layered": (
        (COMPOSED_FRAME,), {}, _set(object_model=torch.ones(3, dtype=torch.uint8), image_width=0)),
    # the composition's own checks (pack_segments), behind the device check
    "poses_on_device": (ALL_COMPOSED, {}, _set(poses=lambda a: a["poses"].to(a["background"].device))),
    "model_empty": (ALL_COMPOSED, {}, _set(xyz=_model1("xyz", lambda t: t[:0]))),
    "model_scaling_wrong_shape": (ALL_COMPOSED, {}, _set(scaling=_model1("scaling", lambda t: t[:, :2]))),
    "features_dc_2d": (ALL_COMPOSED, {}, _set(features_dc=_model1("features_dc", lambda t: t[:, 0]))),
    "sh_count_mismatch": (ALL_COMPOSED, {}, _set(features_rest=_model1("features_rest", lambda t: t[:, :1]))),
    "xyz_float64": (ALL_COMPOSED, {}, _set(xyz=_model1("xyz", lambda t: t.double()))),
    "rotation_on_host": (ALL_COMPOSED, {}, _set(rotation=_model1("rotation", lambda t: t.cpu()))),
    "flip_wrong_size": (ALL_COMPOSED, {}, _set(flip=_model1("flip", lambda t: t[:-1]))),
    "flip_on_host": (ALL_COMPOSED, {}, _set(flip=_model1("flip", lambda t: t.cpu()))),
    "double_model_empty_and_float64_background": (ALL_COMPOSED, {}, _set(xyz=_model1("xyz", lambda t: t[:0]),
                                                                          background=_f64("background"))),
    "double_flip_wrong_size_and_no_frame": ((COMPOSED_FRAME,), {}, _set(flip=_model1("flip", lambda t: t[:-1]),
                                                                        **_no_frame())),
}


def _cases_of(table, entry):
    return sorted(c for c, (entries, _, _) in table.items() if entry in entries)


def run_error_cases(_C, table, entry, dev):
    got = {}
    for case in _cases_of(table, entry):
        _, kw, mutate = table[case]
        a = base_args(dev, entry, **kw)
        mutate(a)
        try:
            getattr(_C, entry)(*a.values())
            got[case] = ["no error", ""]
        except Exception as e:   # noqa: BLE001  (the class is what is recorded)
            got[case] = [type(e).__name__, str(e).split("\n")[0]]
    return got


# ---- b. return layouts ------------------------------------------------------------------------------------------
def _frame_combos():
    combos = {}
    for planes in (False, True):
        for layered in (False, True):
            for rgb8 in (False, True):
                if planes or rgb8:
                    combos["planes%d_layered%d_rgb8%d" % (planes, layered, rgb8)] = (
                        dict(layered=layered), dict(want_planes=planes, want_rgb8=rgb8))
    dev_out = lambda a: torch.empty(H, W, 3, dtype=torch.uint8, device=a["background"].device)   # noqa: E731
    pinned = lambda a: torch.empty(H, W, 3, dtype=torch.uint8).pin_memory()                      # noqa: E731
    combos["out_device"] = ({}, dict(want_planes=False, out_rgb8=dev_out))
    combos["out_pinned_host"] = ({}, dict(want_planes=False, out_rgb8=pinned))
    combos["out_device_unused_without_rgb8"] = ({}, dict(want_rgb8=False, out_rgb8=dev_out))
    combos["no_sky"] = ({}, dict(sky_cube=_empty(), ray_matrix=_empty()))
    return combos


def layout_combos(entry):
    """combination -> (keyword arguments of base_args, replaced arguments)."""
    if entry in FLAT:
        return {"P%d_S%d" % (P, S): (dict(P=P, S=S), {}) for P in (0, P0) for S in (0, 2)}
    if entry == LAYERS:
        return {"P%d" % P: (dict(P=P), {}) for P in (0, P0)}
    if entry == FRAME:
        combos = _frame_combos()
        combos["P0_planes1_layered1_rgb81"] = (dict(P=0, layered=True), {})
        combos["P0_planes1_layered0_rgb81"] = (dict(P=0), {})
        return combos
    if entry == COMPOSED:
        return {"for_backward%d" % fb: ({}, dict(for_backward=fb)) for fb in (False, True)}
    if entry == COMPOSED_LAYERS:
        return {"actors_are_objects": ({}, {}),
                "object_model_given": ({}, dict(object_model=torch.tensor([1, 0], dtype=torch.uint8)))}
    combos = _frame_combos()
    combos["layered_object_model_given"] = (dict(layered=True), dict(object_model=torch.tensor([0, 1]).bool()))
    return combos


def _describe(x):
    if isinstance(x, torch.Tensor):
        return [str(x.dtype), list(x.shape), x.device.type]
    return [type(x).__name__]


def run_layouts(_C, entry, dev):
    got = {}
    for combo, (kw, values) in sorted(layout_combos(entry).items()):
        a = base_args(dev, entry, **kw)
        _set(**values)(a)
        _C.reset_capacity_hints()        # the blobs' sizes then depend on this call alone, not on the calls before it
        out = getattr(_C, entry)(*a.values())
        if entry == "rasterize_gaussians_eval_deferred":
            _C.frame_status(out[0], True)
        torch.cuda.synchronize()
        got[combo] = [_describe(x) for x in out]
    return got


# ---- the tests ----------------------------------------------------------------------------------------------------
def _compare(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    bad = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not bad, "%s (case, got, recorded from the parent):\n%s" % (what, "\n".join(map(repr, bad)))


def _binding():
    from gaussianrpg_amd.rasterizer import _C
    return _C


@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_before_the_device_check(entry):
    want = json.load(open(GOLDEN))["errors"][entry]
    got = run_error_cases(_binding(), CPU_CASES, entry, "cpu")
    assert got and all(v[0] != "no error" for v in got.values()), got
    _compare(got, {c: want[c] for c in _cases_of(CPU_CASES, entry)}, entry)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_on_the_device(entry):
    want = json.load(open(GOLDEN))["errors"][entry]
    got = run_error_cases(_binding(), GPU_CASES, entry, "cuda")
    assert got and all(v[0] != "no error" for v in got.values()), got
    _compare(got, {c: want[c] for c in _cases_of(GPU_CASES, entry)}, entry)
    assert sorted(want) == sorted(_cases_of(GPU_CASES, entry) + _cases_of(CPU_CASES, entry))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_return_layouts(entry):
    _compare(run_layouts(_binding(), entry, "cuda"), json.load(open(GOLDEN))["layouts"][entry], entry)


if __name__ == "__main__":      # recorder: <package dir of the parent build> <json>, on a machine with a device
    pkg, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    spec = importlib.util.spec_from_file_location("_C", glob.glob(os.path.join(pkg, "_C*.so"))[0])
    parent_C = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parent_C)
    assert torch.cuda.is_available(), "the device cases and the layouts need a device"
    table = {"errors": {}, "layouts": {}}
    for name in ENTRIES:
        table["errors"][name] = run_error_cases(parent_C, CPU_CASES, name, "cpu")
        table["errors"][name].update(run_error_cases(parent_C, GPU_CASES, name, "cuda"))
        table["layouts"][name] = run_layouts(parent_C, name, "cuda")
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d error cases and %d layouts from %s" % (
        sum(len(v) for v in table["errors"].values()), sum(len(v) for v in table["layouts"].values()), spec.origin))
