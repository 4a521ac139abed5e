"""CPU tests (-m "not gpu") of the fused lidar-depth / sky / object-alpha losses (gaussianrpg_amd/loss.py,
csrc/aux_loss.hip): the tests' float64 statement (tests/aux_loss_truth.py) against the train.py formulas run in
float64 PyTorch with autograd, the device's k = floor(0.95 * (double)N) against Python's int(0.95 * N), the C
entries' loud failure without a device, and the wrapper's rejections."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import aux_loss_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")


def _formula_lidar(depth, acc, lidar, mask=None):
    """train.py:164-176 as written there, in float64 (selection by the float64 error)."""
    depth_mask = lidar > 0.0
    if mask is not None:
        depth_mask = torch.logical_and(depth_mask, mask)
    if torch.nonzero(depth_mask).any():
        expected = depth / (acc + truth.EPS)
        err = torch.abs(expected[depth_mask] - lidar[depth_mask])
        err, _ = torch.topk(err, int(0.95 * err.size(0)), largest=False)
        return err.mean()
    return (depth * 0).sum() + (acc * 0).sum()


def _formula_sky(acc, sky, scale=1.0):
    a = torch.clamp(acc, min=truth.LO, max=truth.HI)
    return torch.where(sky, -torch.log(1 - a), -torch.log(a)).mean() * scale


def _formula_obj(acc_obj, bound):
    a = torch.clamp(acc_obj, min=truth.LO, max=truth.HI)
    return torch.where(bound, -(a * torch.log(a) + (1. - a) * torch.log(1. - a)), -torch.log(1. - a)).mean()


def _planes(shape, seed, coverage=0.5):
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(shape, generator=g) * 60 + 1
    acc = torch.rand(shape, generator=g) * 0.9 + 0.05
    lidar = torch.rand(shape, generator=g) * 80
    lidar[torch.rand(shape, generator=g) > coverage] = 0
    mask = torch.rand(shape, generator=g) > 0.2
    return depth, acc, lidar, mask


def _grads(fn, *leaves):
    ts = [t.clone().requires_grad_(True) for t in leaves]
    v = fn(*ts)
    v.backward()
    return v.detach(), [t.grad for t in ts]


@pytest.mark.parametrize("shape", [(1, 37, 53), (29, 41), (1, 5, 7), (1, 64, 96)])
def test_truth_lidar_matches_formula(shape):
    depth, acc, lidar, mask = _planes(shape, sum(shape))
    d, a = depth.double(), acc.double()
    for m in (None, mask):
        v, (gd, ga) = _grads(lambda x, y: truth.lidar(x, y, lidar.double(), m), d, a)
        v2, (gd2, ga2) = _grads(lambda x, y: _formula_lidar(x, y, lidar.double(), m), d, a)
        assert abs(float(v) - float(v2)) <= 1e-12 * abs(float(v2))
        assert torch.allclose(gd, gd2, rtol=1e-12, atol=0) and torch.allclose(ga, ga2, rtol=1e-12, atol=0)


def test_truth_lidar_ties():
    # errors 0..9 with the k-th value (k = int(0.95 * 40) = 38) tied across many pixels
    e = torch.tensor([float(i // 4) for i in range(40)], dtype=torch.float64)
    lidar = torch.full((1, 5, 8), 10.0, dtype=torch.float64)
    depth = (lidar.reshape(-1) + e).reshape(1, 5, 8)
    acc = torch.ones_like(depth)
    w, N, k, t, c_lt, c_eq, zero = truth.lidar_weights(depth, acc, lidar)
    assert (N, k, t, c_lt, c_eq, zero) == (40, 38, 9.0, 36, 4, False)
    assert abs(float(w.sum()) - 1.0) < 1e-15
    assert torch.allclose(w[w > 0].unique(), torch.tensor([2 / 4 / 38, 1 / 38], dtype=torch.float64))
    v = truth.lidar(depth, acc, lidar)
    topk = torch.topk(e, k, largest=False).values.mean()
    assert abs(float(v) - float(topk)) < 1e-8     # acc + 1e-10 in float64 is not 1


def test_truth_lidar_zero_term_and_nan():
    z = torch.zeros(1, 4, 6, dtype=torch.float64)
    depth, acc = torch.rand(1, 4, 6, dtype=torch.float64) + 1, torch.rand(1, 4, 6, dtype=torch.float64) + 0.1
    # N == 0
    v, (gd, ga) = _grads(lambda x, y: truth.lidar(x, y, z), depth, acc)
    assert float(v) == 0.0 and float(gd.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0
    # N == 1 at flat index 0: the reference's nonzero guard is false
    l0 = z.clone()
    l0[0, 0, 0] = 5.0
    v, (gd, ga) = _grads(lambda x, y: truth.lidar(x, y, l0), depth, acc)
    assert float(v) == 0.0 and float(gd.abs().max()) == 0.0
    v2 = _formula_lidar(depth, acc, l0)
    assert float(v2) == 0.0
    # N == 1 elsewhere: k == 0, mean of nothing
    l1 = z.clone()
    l1[0, 2, 3] = 5.0
    v, (gd, ga) = _grads(lambda x, y: truth.lidar(x, y, l1), depth, acc)
    assert math.isnan(float(v)) and float(gd.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0
    assert math.isnan(float(_formula_lidar(depth, acc, l1)))
    # [H,W] planes follow the same rule
    v = truth.lidar(depth[0], acc[0], l0[0])
    assert float(v) == 0.0


def test_truth_lidar_nan_depth():
    depth, acc, lidar, mask = _planes((1, 20, 30), 3, coverage=0.9)
    d = depth.double()
    sel = truth.selection(lidar, mask)
    idx = int(torch.nonzero(sel.reshape(-1))[5])
    d.view(-1)[idx] = float("nan")          # one NaN error: sorts last, outside the smallest 95 %
    v, (gd, _) = _grads(lambda x, y: truth.lidar(x, y, lidar.double(), mask), d, acc.double())
    v2 = _formula_lidar(d, acc.double(), lidar.double(), mask)
    assert abs(float(v) - float(v2)) < 1e-12 and float(gd.view(-1)[idx]) == 0.0
    dn = d.clone()
    dn[sel] = float("nan")                  # every selected error NaN: NaN
    assert math.isnan(float(truth.lidar(dn, acc.double(), lidar.double(), mask)))
    assert math.isnan(float(_formula_lidar(dn, acc.double(), lidar.double(), mask)))


@pytest.mark.parametrize("shape", [(1, 37, 53), (48, 31), (1, 1, 1)])
def test_truth_sky_and_obj_match_formula(shape):
    g = torch.Generator().manual_seed(sum(shape))
    acc = torch.rand(shape, generator=g, dtype=torch.float64)
    flat = acc.view(-1)
    flat[: min(4, flat.numel())] = torch.tensor([0.0, truth.LO, truth.HI, 1.0], dtype=torch.float64)[: min(4, flat.numel())]
    sky = torch.rand(shape, generator=g) < 0.3
    for scale in (0.0, 0.5, 1.0):
        v, (ga,) = _grads(lambda x: truth.sky(x, sky, scale), acc)
        v2, (ga2,) = _grads(lambda x: _formula_sky(x, sky, scale), acc)
        assert abs(float(v) - float(v2)) <= 1e-14 and torch.allclose(ga, ga2, rtol=1e-14, atol=0)
    v, (go,) = _grads(lambda x: truth.obj(x, sky), acc)
    v2, (go2,) = _grads(lambda x: _formula_obj(x, sky), acc)
    assert abs(float(v) - float(v2)) <= 1e-14 and torch.allclose(go, go2, rtol=1e-14, atol=0)
    if flat.numel() >= 4:     # clamp backward: inclusive bounds
        assert float(ga.view(-1)[0]) == 0.0 and float(ga.view(-1)[3]) == 0.0
        assert float(ga.view(-1)[1]) != 0.0 and float(ga.view(-1)[2]) != 0.0


def test_truth_sky_nan_propagates():
    acc = torch.full((1, 3, 3), 0.5, dtype=torch.float64)
    acc[0, 1, 1] = float("nan")
    sky = torch.zeros(1, 3, 3, dtype=torch.bool)
    v, (ga,) = _grads(lambda x: truth.sky(x, sky, 0.0), acc)
    assert math.isnan(float(v))           # a scale of 0 still evaluates the term: NaN * 0
    v, (go,) = _grads(lambda x: truth.obj(x, sky), acc)
    assert math.isnan(float(v)) and float(go[0, 1, 1]) == 0.0


def test_k_in_float64_equals_python_int():
    N = np.arange(0, (1 << 22) + 1, dtype=np.int64)
    k_dev = np.floor(0.95 * N.astype(np.float64)).astype(np.int64)   # the device's floor(0.95 * (double)N)
    k_py = np.array([int(0.95 * int(n)) for n in N], dtype=np.int64)
    assert np.array_equal(k_dev, k_py)


def test_loss_module_imports():
    from gaussianrpg_amd import loss
    for name in ("aux_loss", "lidar_depth_loss", "sky_loss", "obj_acc_loss", "lidar_selection"):
        assert callable(getattr(loss, name))
    from gaussianrpg_amd.rasterizer import _C
    assert hasattr(_C, "aux_loss_forward") and hasattr(_C, "aux_loss_backward")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    return ctypes.CDLL(LIB)


def test_c_entries_fail_loudly_without_a_device(lib):
    lib.grpg_aux_loss_workspace_bytes.restype = ctypes.c_size_t
    assert lib.grpg_aux_loss_workspace_bytes(1280, 1920) >= 4 * 1280 * 1920     # pure size query
    assert lib.grpg_aux_loss_workspace_bytes(0, 1920) == 0
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib.grpg_aux_loss_forward.restype = ctypes.c_int
    lib.grpg_aux_loss_backward.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    f = ctypes.c_float
    assert lib.grpg_aux_loss_forward(8, 8, None, None, None, None, None, None, None, f(1.0), f(0.1), f(0.05),
                                     f(0.1), None, None, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_aux_loss_backward(8, 8, None, None, None, None, None, None, None, f(1.0), f(0.1), f(0.05),
                                      f(0.1), None, None, None, None, None, None) == -2


def test_wrapper_rejects_unsupported_inputs():
    from gaussianrpg_amd import loss
    depth, acc, lidar, mask = _planes((1, 8, 9), 1)
    sky = mask.clone()
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.lidar_depth_loss(depth, acc, lidar, mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.sky_loss(acc, sky)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.obj_acc_loss(acc, sky)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.aux_loss(depth, acc, lidar_depth=lidar, lambda_depth_lidar=0.1)
    with pytest.raises(TypeError, match="float32"):
        loss.lidar_depth_loss(depth.double(), acc, lidar)
    with pytest.raises(TypeError, match="float32"):
        loss.sky_loss(acc.half(), sky)
    with pytest.raises(TypeError, match="bool"):
        loss.sky_loss(acc, sky.float())
    with pytest.raises(ValueError, match=r"\[H,W\] or \[1,H,W\]"):
        loss.sky_loss(acc.expand(3, 8, 9), sky)
    with pytest.raises(ValueError, match="another plane"):
        loss.lidar_depth_loss(depth, acc[:, :, :8], lidar)
    with pytest.raises(ValueError, match="lidar_depth requires a gradient"):
        loss.lidar_depth_loss(depth, acc, lidar.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no auxiliary term is on"):
        loss.aux_loss(depth, acc, lidar_depth=lidar)
    with pytest.raises(ValueError, match="needs depth and acc"):
        loss.aux_loss(None, acc, lidar_depth=lidar, lambda_depth_lidar=0.1)
