"""-m gpu: the sky cube map's backward (csrc/sky.hip sky_backward_kernel), texel by texel and pixel by pixel against
the float64 truth of tests/sky_truth.py -- at the kernel (`_C.sky_backward`, with the float32 ray matrix the truth also
gets), through gaussianrpg_amd.sky.SkyCubeMap (both training paths, train mode, white background, a non-contiguous
upstream gradient) and through the C ABI (grpg_sky_backward_ex).  The bars are derived in sky_truth.py's docstring and
shown on the CPU to hold float32 arithmetic with a factor two to spare (tests/test_sky_truth_host.py); every case
records its worst err / tol in helpers.PARITY_STATS."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import sky_truth as T
from test_sky import _RefLikeCamera, _camera

pytestmark = pytest.mark.gpu
GRPG_ERR_INVALID_ARGUMENT = -1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _to(t, dev):
    return None if t is None else t.to(dev)


def _record(plane, **kw):
    test_id = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    helpers.PARITY_STATS.append(dict(test=test_id, plane=plane, **kw))


def _check(plane, t, grad_cube=None, grad_acc=None, **extra):
    """grad_cube / grad_acc (device tensors) against the truth t; prints and records the worst err / tol first."""
    rec = {}
    if grad_cube is not None:
        rec["cube_ratio"], rec["cube_unhit_zero"] = T.cube_ratio(_np(grad_cube), t)
    if grad_acc is not None:
        rec["acc_ratio"] = T.acc_ratio(_np(grad_acc), t)
    print(plane, rec)
    _record(plane, **rec, **extra)
    if grad_cube is not None:
        assert rec["cube_unhit_zero"], "%s: a texel nothing hits is not exactly 0.0" % plane
        assert rec["cube_ratio"] <= 1.0, "%s: grad_cube err / tol = %.3g" % (plane, rec["cube_ratio"])
    if grad_acc is not None:
        assert rec["acc_ratio"] <= 1.0, "%s: grad_acc err / tol = %.3g" % (plane, rec["acc_ratio"])


# ---------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_kernel_matches_float64_truth(dev, name):
    from gaussianrpg_amd.rasterizer import _C
    case = T.CASES[T.CASE_NAMES.index(name)]
    i, t = T.case_truth(name)
    shares = T.check_case_conditions(case, t)
    cube, g, acc, mask, jit = (_to(i[k], dev) for k in ("cube", "g", "acc", "mask", "jitter"))
    rm = i["M"].to(dev) if case.mdev else i["M"]
    runs = []
    for rep in range(2):
        gc, ga = _C.sky_backward(cube, rm, case.fill, acc, g, mask, jit)
        torch.cuda.synchronize()
        assert gc.shape == cube.shape and ga.shape == (1, case.H, case.W)
        _check("sky_backward/%s/run%d" % (name, rep), t, gc, ga, **shares)
        runs.append((gc, ga))
    assert torch.equal(runs[0][1], runs[1][1]), "grad_acc differs between two runs"
    if case.mode == "acc_edge":       # acc 1.0, float32(0.999), 1.0005 and NaN: no fetch, grad_acc = -fill sum g
        off = torch.from_numpy(~t["fetch"]).to(dev)
        assert int(off.sum()) >= 3 * case.W + 10
        assert bool(torch.isfinite(runs[0][1]).all())


# ---------------------------------------------------------------------------------------------------------------
# module level: gaussianrpg_amd.sky.SkyCubeMap
# ---------------------------------------------------------------------------------------------------------------
RES, HM, WM = 16, 61, 67


def _module_inputs(seed):
    """cube, acc (values on both sides of the 1e-3 fetch threshold), rgb, g: CPU float32."""
    gen = torch.Generator().manual_seed(seed)
    cube = torch.rand(6, RES, RES, 3, generator=gen) * 1.6 - 0.3
    acc = torch.rand(1, HM, WM, generator=gen) * 0.95
    # float32(0.999) = 1 - 16777 * 2^-24 does not fetch, its float32 neighbour below (row 19) does
    for row, v in ((4, float(np.float32(0.999))), (9, 1.0), (14, 0.9985), (19, 1.0 - 16778 * 2.0 ** -24), (24, 0.99905),
                   (29, 0.0)):
        acc[0, row] = v
    acc[0, 33:36, ::3] = float(np.float32(0.999))
    rgb = torch.rand(3, HM, WM, generator=gen)
    g = torch.randn(3, HM, WM, generator=gen)
    return cube, acc, rgb, g


def _sky_module(dev, cube, **kw):
    from gaussianrpg_amd.sky import SkyCubeMap
    sky = SkyCubeMap(RES, **kw).to(dev)
    with torch.no_grad():
        sky.sky_cube_map.copy_(cube.to(dev))
    return sky


@pytest.mark.parametrize("path", ["lookup_then_torch", "fused_composite"])
@pytest.mark.parametrize("white", [False, True])
def test_module_training_paths(dev, path, white):
    from gaussianrpg_amd.sky import ray_matrix
    K, w2c = _camera(WM, HM, *T.CORNER, 0.55)
    cube, acc, rgb, g = _module_inputs(21)
    fill = 1.0 if white else 0.0
    t = T.backward64(cube.numpy(), ray_matrix(K, w2c).numpy(), HM, WM, g.numpy(), acc=acc.numpy(), fill=fill)
    off = ~t["fetch"]
    assert off[4].all() and off[9].all() and t["fetch"][14].all() and t["fetch"][19].all() and off[24].all()
    assert int(t["corner"].sum()) > 0 and int(t["clamped"].sum()) >= 50
    sky = _sky_module(dev, cube, white_background=white)
    a = acc.to(dev).requires_grad_(True)
    r = rgb.to(dev).requires_grad_(True)
    gd = g.to(dev)
    if path == "lookup_then_torch":
        # forward() itself hands acc no gradient (the reference detaches nothing, but its mask is not differentiable
        # either: the only way to acc is the composite's (1 - acc))
        s_only = sky(K, w2c, HM, WM, a)
        s_only.backward(gd)
        assert a.grad is None and sky.sky_cube_map.grad is not None
        sky.sky_cube_map.grad = None
        out = r + sky(K, w2c, HM, WM, a) * (1.0 - a)
    else:
        out = sky.composite(r, a, K, w2c, train=True)
    out.backward(gd)
    torch.cuda.synchronize()
    assert torch.equal(r.grad, gd)
    _check("sky_module/%s/fill%d" % (path, fill), t, sky.sky_cube_map.grad, a.grad)
    if white:      # where nothing is fetched: -(g0 + g1 + g2), two float32 additions
        ga = a.grad.detach().cpu().numpy().astype(np.float64)[0]
        g64 = g.double().numpy()
        err = np.abs(ga + g64.sum(axis=0))[off]
        assert (err <= 2 * T.EPS * np.abs(g64).sum(axis=0)[off]).all(), float(err.max())


def test_module_train_mode_through_the_camera_form(dev):
    from gaussianrpg_amd.sky import ray_matrix, train_sky_mask
    K, w2c = _camera(WM, HM, 0.9, -0.4, 0.3)
    cube, acc, _, g = _module_inputs(22)
    gen = torch.Generator().manual_seed(23)
    sky_mask = torch.rand(1, HM, WM, generator=gen) > 0.6
    jitter = torch.rand(2, HM, WM, generator=gen)
    cam = _RefLikeCamera(K.to(dev), w2c.to(dev), HM, WM, sky_mask.to(dev))
    before = cam.original_sky_mask.clone()
    m = train_sky_mask(sky_mask)
    assert m[:50].all() and not m[50:].all() and m[50:].any()
    # the matrix forward() forms, on the device like the camera's tensors
    M32 = ray_matrix(cam.K, cam.world_view_transform.transpose(0, 1)).cpu().numpy()
    t = T.backward64(cube.numpy(), M32, HM, WM, g.numpy(), acc=None, mask=m.numpy(), jitter=jitter.numpy(), fill=0.0)
    sky = _sky_module(dev, cube, mode="train")
    a = acc.to(dev).requires_grad_(True)
    out = sky(cam, a, jitter=jitter.to(dev))
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    _check("sky_module/train_camera", t, sky.sky_cube_map.grad)
    assert a.grad is None
    assert torch.equal(cam.original_sky_mask, before)


def test_module_non_contiguous_upstream_gradient(dev):
    from gaussianrpg_amd.sky import ray_matrix
    K, w2c = _camera(WM, HM, *T.FACE, 0.55)
    cube, acc, rgb, g = _module_inputs(24)
    t = T.backward64(cube.numpy(), ray_matrix(K, w2c).numpy(), HM, WM, g.numpy(), acc=acc.numpy())
    sky = _sky_module(dev, cube)
    got = {}
    for kind in ("contiguous", "permuted"):
        sky.sky_cube_map.grad = None
        a = acc.to(dev).requires_grad_(True)
        r = rgb.to(dev).requires_grad_(True)
        out = sky.composite(r, a, K, w2c, train=True)
        seen = []
        out.register_hook(lambda gr: seen.append(gr.is_contiguous()))
        if kind == "contiguous":
            (out * g.to(dev)).sum().backward()
        else:
            (out.permute(1, 2, 0) * g.permute(1, 2, 0).contiguous().to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert seen == [kind == "contiguous"], (kind, seen)
        _check("sky_module/upstream_%s" % kind, t, sky.sky_cube_map.grad, a.grad)
        got[kind] = (sky.sky_cube_map.grad.clone(), a.grad.clone(), r.grad.clone())
    assert torch.equal(got["contiguous"][1], got["permuted"][1])
    assert torch.equal(got["contiguous"][2], got["permuted"][2])
    diff = (got["contiguous"][0].double() - got["permuted"][0].double()).abs().cpu().numpy()
    assert (diff <= t["tol_cube"]).all()


def test_a_loss_that_ignores_the_sky_leaves_its_gradient_unset(dev):
    K, w2c = _camera(WM, HM, *T.FACE, 0.55)
    cube, acc, rgb, g = _module_inputs(25)
    sky = _sky_module(dev, cube)
    a = acc.to(dev).requires_grad_(True)
    r = rgb.to(dev).requires_grad_(True)
    sky.composite(r, a, K, w2c, train=True)
    sky(K, w2c, HM, WM, a)
    ((r * g.to(dev)).sum() + a.sum()).backward()
    assert sky.sky_cube_map.grad is None
    assert torch.equal(r.grad, g.to(dev))


# ---------------------------------------------------------------------------------------------------------------
# C ABI: grpg_sky_backward_ex, the library loaded as tests/test_gpu_cabi_backward.py loads it
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gaussianrpg_amd.build import LIB_PATH
    lb = ctypes.CDLL(LIB_PATH)
    lb.grpg_sky_backward_ex.restype = ctypes.c_int
    lb.grpg_last_error.restype = ctypes.c_char_p
    return lb


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Abi:
    CASE = "r16_61x67_face_f0.55_acc_edge_fill1_host"

    def __init__(self, lib, dev):
        self.lib, self.dev = lib, dev
        self.case = T.CASES[T.CASE_NAMES.index(self.CASE)]
        i, self.t = T.case_truth(self.CASE)
        self.cube, self.g, self.acc = (i[k].to(dev).contiguous() for k in ("cube", "g", "acc"))
        self.M = i["M"].contiguous()          # host float[9]

    def call(self, grad_cube, grad_acc, cube="own", res=None, grad_rgb="own"):
        c = self.case
        rc = self.lib.grpg_sky_backward_ex(
            _p(self.cube if cube == "own" else cube), c.res if res is None else res, _p(self.M), 0,
            ctypes.c_float(c.fill), c.W, c.H, _p(self.acc), None, None, _p(self.g if grad_rgb == "own" else grad_rgb),
            _p(grad_cube), _p(grad_acc), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def buffers(self, value=0.0):
        c = self.case
        return (torch.full((6, c.res, c.res, 3), value, device=self.dev),
                torch.full((c.H, c.W), float("nan"), device=self.dev))


def test_cabi_optional_outputs_and_accumulation(dev, lib):
    f = _Abi(lib, dev)
    gc, ga = f.buffers()
    assert f.call(gc, ga) == 0, lib.grpg_last_error()
    _check("sky_cabi/full", f.t, gc, ga)
    # grad_cube = NULL: the same grad_acc bits
    _, ga2 = f.buffers()
    assert f.call(None, ga2) == 0, lib.grpg_last_error()
    assert torch.equal(ga2, ga)
    # grad_acc = NULL
    gc3, _ = f.buffers()
    assert f.call(gc3, None) == 0, lib.grpg_last_error()
    _check("sky_cabi/no_grad_acc", f.t, gc3)
    # the header: grad_cube is accumulated into -> 0.5 + gradient; the sum now rounds at 0.5 + |G|
    gc4, _ = f.buffers(0.5)
    assert f.call(gc4, None) == 0, lib.grpg_last_error()
    untouched = torch.from_numpy((f.t["n"] == 0) & (f.t["F"] == 0)).to(dev)
    assert bool((gc4[untouched] == 0.5).all())
    widen = T.EPS * (0.5 + np.abs(f.t["grad_cube"]))
    hit = f.t["n"] > 0
    err = np.abs(gc4.double().cpu().numpy() - 0.5 - f.t["grad_cube"])
    tol = f.t["tol_cube"] + widen
    ratio = float((err[hit] / tol[hit]).max())
    print("sky_cabi/prefilled", ratio)
    helpers.PARITY_STATS.append(dict(test="test_cabi_optional_outputs_and_accumulation", plane="sky_cabi/prefilled",
                                     cube_ratio=ratio))
    assert ratio <= 1.0


def test_cabi_argument_errors_leave_the_library_usable(dev, lib):
    f = _Abi(lib, dev)
    gc, ga = f.buffers()
    assert f.call(gc, ga) == 0
    want_acc = ga.clone()
    for kw, what in ((dict(res=0), "res = 0"), (dict(cube=None), "NULL cube"), (dict(grad_rgb=None), "NULL grad_rgb")):
        gcx, gax = f.buffers()
        assert f.call(gcx, gax, **kw) == GRPG_ERR_INVALID_ARGUMENT, what
        assert lib.grpg_last_error()
        assert float(gcx.abs().max()) == 0.0 and bool(torch.isnan(gax).all()), "%s: an output was written" % what
        gc2, ga2 = f.buffers()
        assert f.call(gc2, ga2) == 0, lib.grpg_last_error()
        assert torch.equal(ga2, want_acc)
        _check("sky_cabi/after_%s" % what.replace(" ", "_"), f.t, gc2)
