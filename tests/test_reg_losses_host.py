"""CPU tests (-m "not gpu") of the fused mono-normal loss, the scale-flatten / opacity-sparse regularisers and PSNR:
the float64 statements the GPU tests compare against (tests/normal_loss_truth.py, tests/reg_loss_truth.py) equal the
reference's expressions on small inputs, the Python surface rejects what it cannot run (there is no CPU or PyTorch
fallback), and the C ABI answers its size queries and fails loudly without a device."""
import ctypes
import inspect
import math
import os

import pytest
import torch

import normal_loss_truth as ntruth
import reg_loss_truth as rtruth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
NEW_NAMES = ("normal_loss", "normal_loss_terms", "scale_flatten_loss", "opacity_sparse_loss", "gaussian_reg_loss",
             "psnr")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    return ctypes.CDLL(LIB)


def _normal_inputs(H=7, W=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    normals = torch.randn(3, H, W, generator=g)
    mono = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    wvt = torch.eye(4)
    wvt[:3, :3] = q
    wvt[3, :3] = torch.randn(3, generator=g)
    mask = torch.rand(1, H, W, generator=g) < 0.8
    sky = torch.rand(1, H, W, generator=g) < 0.3
    return normals, mono, wvt, mask, sky


def _reg_inputs(N=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    scaling = torch.randn(N, 3, generator=g) * 1.5 - 3
    opacity = torch.randn(N, 1, generator=g) * 4
    radii = (torch.rand(N, generator=g) < 0.6).int() * 5
    return scaling, opacity, radii


# ---- the truth modules state the reference's lines ----

def test_normal_truth_is_the_reference_expression():
    normals, mono, wvt, mask, sky = _normal_inputs()
    l1, cos, n = ntruth.terms64(normals, mono, wvt, mask, sky, normalize=True, top_rows=2)
    # train.py:206-225 by hand, per pixel
    x = torch.nn.functional.normalize(normals.double(), dim=0)
    R = wvt.double()[:3, :3]
    sel = (mask & ~sky)[0].clone()
    sel[:2] = False
    a = b = 0.0
    for y, xx in sel.nonzero().tolist():
        gt = R @ mono.double()[:, y, xx]          # (m @ R.T)_j = sum_k m_k R[j][k]
        p = x[:, y, xx]
        a += float((p - gt).abs().sum())
        b += 1.0 - float((p * gt).sum())
    assert n == int(sel.sum()) and n > 0
    assert abs(float(l1) - a / (3 * n)) <= 1e-13 and abs(float(cos) - b / n) <= 1e-13
    assert float(ntruth.loss64(normals, mono, wvt, mask, sky, normalize=True, top_rows=2)) == float(l1 + cos)
    # no sky mask: the mask alone, no row cut; no mask at all: every pixel
    assert ntruth.terms64(normals, mono, wvt, mask, None)[2] == int(mask.sum())
    assert ntruth.terms64(normals, mono, wvt, None, None)[2] == 7 * 9
    assert ntruth.terms64(normals, mono, wvt, None, sky, top_rows=3)[2] == int((~sky[0, 3:]).sum())
    # normalize=False takes the planes as given
    unit = torch.nn.functional.normalize(normals, dim=0)
    l1n, _, _ = ntruth.terms64(unit, mono, wvt, mask, sky, normalize=False, top_rows=2)
    assert abs(float(l1n) - float(l1)) <= 1e-6
    # float32: the reference's own arithmetic, a few ulp from float64
    v32 = float(ntruth.loss32(normals, mono, wvt, mask, sky, top_rows=2))
    assert abs(v32 - float(l1 + cos)) <= 1e-6 * abs(float(l1 + cos))


def test_normal_truth_empty_selection_is_nan_with_a_zero_gradient():
    normals, mono, wvt, mask, sky = _normal_inputs()
    x = normals.double().requires_grad_(True)
    v = ntruth.loss64(x, mono, wvt, mask, sky, top_rows=50)        # 7 rows: the cut removes every pixel
    v.backward()
    assert math.isnan(float(v.detach())) and float(x.grad.abs().max()) == 0.0


def test_scale_flatten_truth_is_the_reference_expression():
    scaling, _, _ = _reg_inputs()
    scaling[3] = torch.tensor([4.0, -20.0, 0.0])
    scaling[4] = torch.tensor([-13.0, -12.0, -14.0])
    v = rtruth.scale_flatten64(scaling)
    t = 0.0
    for row in scaling.double().exp().tolist():
        s1, s2, s3 = sorted(row)
        s1, s2, s3 = min(max(s1, 0.0), 30.0), min(max(s2, 1e-5), 30.0), min(max(s3, 1e-5), 30.0)
        t += abs(s1) + abs(s2 / s3 + s3 / s2 - 2.0)
    assert abs(float(v) - t / scaling.shape[0]) <= 1e-12 * abs(float(v))
    assert float(rtruth.scale_flatten64(scaling.double().exp(), activated=True)) == pytest.approx(float(v), rel=1e-12)
    assert abs(float(rtruth.scale_flatten32(scaling)) - float(v)) <= 1e-6 * abs(float(v))
    assert math.isnan(float(rtruth.scale_flatten64(scaling[:0])))
    # a tie keeps index order: the gradient of |s1| lands on the first of two equal values
    tie = torch.tensor([[0.5, 0.5, 2.0]], dtype=torch.float64, requires_grad=True)
    rtruth.scale_flatten64(tie, activated=True).backward()
    assert float(tie.grad[0, 0]) == 1.0 and float(tie.grad[0, 1]) != 1.0


def test_opacity_sparse_truth_is_the_reference_expression():
    _, opacity, radii = _reg_inputs()
    opacity[2], opacity[5] = 20.0, -20.0
    radii[2], radii[5] = 3, 3
    v = rtruth.opacity_sparse64(opacity, radii)
    t, n = 0.0, 0
    for x, r in zip(opacity.double().reshape(-1).tolist(), radii.tolist()):
        if r > 0:
            o = min(max(1.0 / (1.0 + math.exp(-x)), 1e-6), 1 - 1e-6)
            t -= o * math.log(o) + (1 - o) * math.log(1 - o)
            n += 1
    assert abs(float(v) - t / n) <= 1e-12 * abs(float(v))
    # a list of models is the concatenation
    parts = [opacity[:4], opacity[4:4], opacity[4:]]
    assert float(rtruth.opacity_sparse64(parts, radii)) == float(v)
    assert abs(float(rtruth.opacity_sparse32(opacity, radii)) - float(v)) <= 1e-6 * abs(float(v))
    x = opacity.double().requires_grad_(True)
    w = rtruth.opacity_sparse64(x, torch.zeros_like(radii))
    w.backward()
    assert math.isnan(float(w.detach())) and float(x.grad.abs().max()) == 0.0
    # the planted +-20 are clamped: zero gradient
    x = opacity.double().requires_grad_(True)
    rtruth.opacity_sparse64(x, radii).backward()
    assert float(x.grad[2]) == 0.0 and float(x.grad[5]) == 0.0


def test_psnr_truth_is_the_reference_expression():
    g = torch.Generator().manual_seed(2)
    a, b = torch.rand(3, 5, 6, generator=g), torch.rand(3, 5, 6, generator=g)
    m = torch.rand(1, 5, 6, generator=g) < 0.5
    mse = float(((a.double() - b.double()) ** 2)[:, m[0]].mean())
    assert abs(float(rtruth.psnr64(a, b, m)) - 20 * math.log10(1 / math.sqrt(mse))) <= 1e-12
    assert abs(float(rtruth.psnr64(a, b)) - 20 * math.log10(1 / math.sqrt(float(((a.double() - b.double()) ** 2).mean())))) <= 1e-12
    assert math.isnan(float(rtruth.psnr64(a, b, torch.zeros_like(m))))
    assert math.isinf(float(rtruth.psnr64(a, a)))


# ---- the Python surface ----

def test_new_names_are_public():
    from gaussianrpg_amd import loss
    for name in NEW_NAMES:
        assert name in loss.__all__ and callable(getattr(loss, name)), name
        assert name in loss.__doc__, name
    assert "no gradient" in loss.psnr.__doc__.lower()


def test_normal_loss_rejects_what_it_cannot_run():
    from gaussianrpg_amd import loss
    normals, mono, wvt, mask, sky = _normal_inputs()
    for fn in (loss.normal_loss, loss.normal_loss_terms):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(normals, mono, wvt)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(normals, mono, wvt, mask, sky, normalize=False, top_rows=3)
        with pytest.raises(TypeError, match="float32"):
            fn(normals.double(), mono, wvt)
        with pytest.raises(TypeError, match="float32"):
            fn(normals, mono.half(), wvt)
        with pytest.raises(TypeError, match="float32"):
            fn(normals, mono, wvt.double())
        with pytest.raises(TypeError, match="bool"):
            fn(normals, mono, wvt, mask.float())
        with pytest.raises(TypeError, match="bool"):
            fn(normals, mono, wvt, mask, sky.long())
        with pytest.raises(ValueError):
            fn(normals, mono[:, :-1], wvt)                       # mismatched H x W
        with pytest.raises(ValueError):
            fn(normals[:2], mono[:2], wvt)                       # not three planes
        with pytest.raises(ValueError):
            fn(normals, mono, wvt[:3, :3])                       # the camera's [4,4] is expected
        with pytest.raises(ValueError):
            fn(normals, mono, wvt, mask[:, :, :-1])
        with pytest.raises(ValueError):
            fn(normals, mono, wvt, mask, sky[:, 1:])
        with pytest.raises(ValueError, match="top_rows"):
            fn(normals, mono, wvt, mask, sky, top_rows=-1)
        with pytest.raises(ValueError, match="requires a gradient"):
            fn(normals, mono.clone().requires_grad_(True), wvt)


def test_regularisers_reject_what_they_cannot_run():
    from gaussianrpg_amd import loss
    scaling, opacity, radii = _reg_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.scale_flatten_loss(scaling)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.opacity_sparse_loss(opacity, radii)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.opacity_sparse_loss([opacity[:4], opacity[4:].reshape(-1)], radii, activated=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.gaussian_reg_loss(scaling=scaling, opacities=[opacity], radii=radii, lambda_scale_flatten=0.1,
                               lambda_opacity_sparse=0.2)
    with pytest.raises(TypeError, match="float32"):
        loss.scale_flatten_loss(scaling.double())
    with pytest.raises(TypeError, match="float32"):
        loss.opacity_sparse_loss(opacity.double(), radii)
    with pytest.raises(TypeError, match="int32"):
        loss.opacity_sparse_loss(opacity, radii.long())
    with pytest.raises(TypeError, match="int32"):
        loss.opacity_sparse_loss(opacity, radii > 0)
    with pytest.raises(ValueError):
        loss.scale_flatten_loss(scaling[:, :2])
    with pytest.raises(ValueError):
        loss.scale_flatten_loss(scaling.reshape(-1))
    with pytest.raises(ValueError):
        loss.opacity_sparse_loss(opacity.reshape(1, -1), radii)
    with pytest.raises(ValueError, match="radii"):
        loss.opacity_sparse_loss(opacity, radii[:-1])                         # radii / sum N_i mismatch
    with pytest.raises(ValueError, match="radii"):
        loss.opacity_sparse_loss([opacity, opacity[:3]], radii)
    with pytest.raises(ValueError, match="no regulariser is on"):
        loss.gaussian_reg_loss(scaling=scaling, opacities=opacity, radii=radii)
    with pytest.raises(ValueError, match="no regulariser is on"):
        loss.gaussian_reg_loss(lambda_scale_flatten=0.1, lambda_opacity_sparse=0.1)


def test_psnr_rejects_what_it_cannot_run():
    from gaussianrpg_amd import loss
    g = torch.Generator().manual_seed(2)
    a, b = torch.rand(3, 5, 6, generator=g), torch.rand(3, 5, 6, generator=g)
    m = torch.rand(1, 5, 6, generator=g) < 0.5
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.psnr(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.psnr(a, b, m)
    with pytest.raises(TypeError, match="float32"):
        loss.psnr(a.double(), b)
    with pytest.raises(TypeError, match="bool"):
        loss.psnr(a, b, m.float())
    with pytest.raises(ValueError):
        loss.psnr(a, b[:, :-1])
    with pytest.raises(ValueError):
        loss.psnr(a[0], b[0])
    with pytest.raises(ValueError):
        loss.psnr(a, b, m[:, :, 1:])


def test_binding_exposes_the_entry_points():
    from gaussianrpg_amd.rasterizer import _C
    for name in ("normal_loss_forward", "normal_loss_backward", "reg_loss_forward", "reg_loss_backward",
                 "psnr_forward"):
        assert hasattr(_C, name), name
    normals, mono, wvt, _, _ = _normal_inputs()
    e = torch.empty(0, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.normal_loss_forward(normals, mono, wvt, e, e, True, 50)
    scaling, opacity, radii = _reg_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.reg_loss_forward(scaling, False, [opacity], False, radii, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.psnr_forward(normals, mono, e)


# ---- the C ABI ----

def test_workspace_size_queries_need_no_device(lib):
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7                                   # additive exports only
    for fn in (lib.grpg_normal_loss_workspace_bytes, lib.grpg_reg_loss_workspace_bytes, lib.grpg_psnr_workspace_bytes):
        fn.restype = ctypes.c_size_t
    n = lib.grpg_normal_loss_workspace_bytes(37, 53)
    assert 8 <= n < (1 << 16) and n % 16 == 0                            # a header and the partials, no plane
    assert lib.grpg_normal_loss_workspace_bytes(1280, 1920) == n
    assert lib.grpg_normal_loss_workspace_bytes(0, 53) == 0
    assert lib.grpg_normal_loss_workspace_bytes(65536, 65536) == 0       # H*W >= 2^31
    r1, r11 = lib.grpg_reg_loss_workspace_bytes(1), lib.grpg_reg_loss_workspace_bytes(11)
    assert 8 <= r1 <= r11 < (1 << 17)
    assert lib.grpg_reg_loss_workspace_bytes(1000) >= 2 * 32 * 1000      # a forward and a backward segment table
    assert lib.grpg_reg_loss_workspace_bytes(0) > 0 and lib.grpg_reg_loss_workspace_bytes(-1) == 0
    assert 8 <= lib.grpg_psnr_workspace_bytes() < (1 << 16)


def test_entry_points_fail_loudly_without_a_device(lib):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib.grpg_last_error.restype = ctypes.c_char_p
    f, ll = ctypes.c_float, ctypes.c_longlong
    for name in ("grpg_normal_loss_forward", "grpg_normal_loss_backward", "grpg_reg_loss_forward",
                 "grpg_reg_loss_backward", "grpg_psnr_forward"):
        getattr(lib, name).restype = ctypes.c_int
    assert lib.grpg_normal_loss_forward(4, 4, None, None, None, 4, 1, None, None, 1, 50, None, None, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_normal_loss_backward(4, 4, None, None, None, 4, 1, None, None, 1, 50, None, None, None, None) == -2
    assert lib.grpg_reg_loss_forward(None, ll(0), 0, None, 0, 0, None, ll(0), f(1.0), f(1.0), None, None, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_reg_loss_backward(None, ll(0), 0, None, 0, 0, None, ll(0), f(1.0), f(1.0), None, None, None,
                                      None) == -2
    assert lib.grpg_psnr_forward(3, 4, 4, None, None, None, None, None, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()


# ---- harness.train_loss ----

def test_train_loss_accepts_the_new_keywords():
    from gaussianrpg_amd import harness as hz
    p = inspect.signature(hz.train_loss).parameters
    for name, default in (("mono_normal", None), ("world_view_transform", None), ("lambda_normal_mono", 0.0),
                          ("scaling", None), ("opacities", None), ("lambda_scale_flatten", 0.0),
                          ("lambda_opacity_sparse", 0.0)):
        assert p[name].default == default and p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    g = torch.Generator().manual_seed(1)
    normals, mono, wvt, mask, sky = _normal_inputs(6, 8)
    scaling, opacity, radii = _reg_inputs()
    pkg = {"rgb": torch.rand(3, 6, 8, generator=g), "acc": torch.rand(1, 6, 8, generator=g) * 0.9 + 0.05,
           "depth": torch.rand(1, 6, 8, generator=g) * 10, "normals": normals, "radii": radii}
    gt_img = torch.rand(3, 6, 8, generator=g)
    base = hz.train_loss(pkg, gt_img, sky_mask=sky)
    # the defaults, a lambda of 0 and a missing input leave the result as it is (CPU tensors: the PyTorch terms only)
    assert torch.equal(base, hz.train_loss(pkg, gt_img, sky_mask=sky, mono_normal=mono, world_view_transform=wvt,
                                           scaling=scaling, opacities=[opacity]))
    assert torch.equal(base, hz.train_loss(pkg, gt_img, sky_mask=sky, lambda_normal_mono=0.1,
                                           lambda_scale_flatten=0.1, lambda_opacity_sparse=0.1))
    for kw in (dict(mono_normal=mono, world_view_transform=wvt, lambda_normal_mono=0.1),
               dict(scaling=scaling, lambda_scale_flatten=0.1),
               dict(opacities=[opacity], lambda_opacity_sparse=0.1)):
        with pytest.raises(RuntimeError, match="no CPU path"):                                       # no fallback
            hz.train_loss(pkg, gt_img, sky_mask=sky, **kw)
