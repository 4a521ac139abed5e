"""GPU tests of the fused scale-flatten and opacity-sparse regularisers and of PSNR (gaussianrpg_amd/loss.py,
csrc/reg_loss.hip, csrc/metrics.hip) against the float64 statements of gaussian_model.py:271-280, train.py:197-203 and
loss_utils.py:61-78 (tests/reg_loss_truth.py) and against the same code run in float32 PyTorch on the device (the
reference's own arithmetic).

Bars (those of tests/test_gpu_aux_loss.py and tests/test_gpu_semantic_loss.py): each value within 1e-6 relative of
float64 and no further from it than twice the float32 PyTorch path plus 3e-7 relative; the gradient within relative
L2 1e-5 of float64 autograd; the counts exact.  Float32 PyTorch itself misses the first bar on the single Gaussian of
N = 1 (1.7e-6 relative: the cancellation in s2/s3 + s3/s2 - 2); the kernel evaluates (s2 - s3)^2 / (s2 s3) and meets it."""
import ctypes
import math
import os

import pytest
import torch

import normal_loss_truth as ntruth
import reg_loss_truth as truth
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

VAL_REL = 1e-6
VAL_FLOOR = 3e-7      # relative: a few ulp of a float32
GRAD_REL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 1: one lane; 63: a partial wave; 1000: a partial workgroup among whole ones; 70001: 274 workgroups of partials, odd
SIZES = [1, 63, 1000, 70001]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _inputs(N, dev, seed=0):
    """Continuous random log-scales with the planted rows (a value above the upper clamp, values under the lower one,
    an exact tie s1 == s2), opacities with planted +-20, 60 % visible."""
    g = torch.Generator().manual_seed(7 * N + seed)
    scaling = torch.randn(N, 3, generator=g) * 1.5 - 3
    opacity = torch.randn(N, 1, generator=g) * 4
    radii = (torch.rand(N, generator=g) < 0.6).int() * torch.randint(1, 40, (N,), generator=g).int()
    if N >= 63:
        scaling[5] = torch.tensor([4.0, -20.0, 0.0])           # exp(4) = 54.6 > 30
        scaling[N - 2] = torch.tensor([-13.0, -12.0, -14.0])   # all under 1e-5
        scaling[N // 2] = torch.tensor([-3.5, -1.0, -3.5])     # s1 == s2 exactly: index order decides
        opacity[3], opacity[N - 1] = 20.0, -20.0               # clamped: zero gradient
        radii[3], radii[N - 1], radii[7] = 9, 9, -1            # both visible; a negative radius is invisible
    else:
        radii[0] = 3
    return scaling.to(dev), opacity.to(dev), radii.to(dev)


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def _val_ok(v, v64, v32, what):
    v, v64, v32 = float(v), float(v64), float(v32)
    e, e32 = abs(v - v64), abs(v32 - v64)
    scale = max(abs(v64), 1e-30)
    print("%s: value %.9g float64 %.9g rel err %.3g (float32 torch %.3g)" % (what, v, v64, e / scale, e32 / scale))
    assert math.isfinite(v), (what, v)
    assert e <= VAL_REL * scale, (what, v, v64)
    assert e <= 2 * e32 + VAL_FLOOR * scale, (what, e, e32)


def _grad_ok(g, g64, what):
    assert bool(torch.isfinite(g).all()), what
    assert g.shape == g64.shape, what
    if float(g64.double().abs().max()) == 0.0:
        assert float(g.abs().max()) == 0.0, what
    else:
        print("%s: gradient rel L2 %.3g" % (what, _rel(g, g64)))
        assert _rel(g, g64) < GRAD_REL, (what, _rel(g, g64))


def _scale(scaling, activated=False):
    from gaussianrpg_amd import loss
    x = scaling.clone().requires_grad_(True)
    v = loss.scale_flatten_loss(x, activated=activated)
    v.backward()
    return v.detach(), x.grad


def _opacity(opacities, radii, activated=False):
    from gaussianrpg_amd import loss
    single = isinstance(opacities, torch.Tensor)
    xs = [o.clone().requires_grad_(True) for o in ([opacities] if single else opacities)]
    v = loss.opacity_sparse_loss(xs[0] if single else xs, radii, activated=activated)
    v.backward()
    return v.detach(), (xs[0].grad if single else [x.grad for x in xs])


# ---- scale flatten ----

@pytest.mark.parametrize("activated", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_scale_flatten_value_and_gradient(dev, N, activated):
    scaling, _, _ = _inputs(N, dev)
    if activated:
        scaling = torch.exp(scaling)
    v, g = _scale(scaling, activated)
    x64 = scaling.double().requires_grad_(True)
    v64 = truth.scale_flatten64(x64, activated)
    v64.backward()
    assert v.shape == () and v.dtype == torch.float32
    _val_ok(v, v64.detach(), truth.scale_flatten32(scaling, activated), "scale flatten N=%d activated=%s" % (N, activated))
    _grad_ok(g, x64.grad, "scale flatten N=%d activated=%s" % (N, activated))
    if N >= 63:
        # above the upper clamp and under the lower one: exactly 0, as torch's clamp passes nothing there
        assert float(g[5, 0]) == 0.0 and float(g[5, 1]) != 0.0 and float(g[5, 2]) != 0.0
        assert float(g[N - 2, 0]) == 0.0 and float(g[N - 2, 1]) == 0.0 and float(g[N - 2, 2]) != 0.0
        assert float(x64.grad[5, 0]) == 0.0 and float(x64.grad[N - 2, 0]) == 0.0 and float(x64.grad[N - 2, 1]) == 0.0
        # the tie: the stable sort makes column 0 s1 and column 2 s2
        tie = N // 2
        assert float(scaling[tie, 0]) == float(scaling[tie, 2])
        assert _rel(g[tie], x64.grad[tie]) < GRAD_REL
        assert float(g[tie, 0]) != float(g[tie, 2])


def test_scale_flatten_of_nothing_is_nan(dev):
    v, g = _scale(torch.empty(0, 3, device=dev))
    assert math.isnan(float(v)) and g.shape == (0, 3)


# ---- opacity sparse ----

@pytest.mark.parametrize("N", SIZES)
def test_opacity_sparse_value_and_gradient(dev, N):
    from gaussianrpg_amd.rasterizer import _C
    _, opacity, radii = _inputs(N, dev)
    v, g = _opacity(opacity, radii)
    x64 = opacity.double().requires_grad_(True)
    v64 = truth.opacity_sparse64(x64, radii)
    v64.backward()
    assert v.shape == () and v.dtype == torch.float32
    _val_ok(v, v64.detach(), truth.opacity_sparse32(opacity, radii), "opacity sparse N=%d" % N)
    _grad_ok(g, x64.grad, "opacity sparse N=%d" % N)
    assert float(g[radii <= 0].abs().max() if bool((radii <= 0).any()) else 0.0) == 0.0   # invisible: exactly 0
    if N >= 63:
        assert float(g[3]) == 0.0 and float(g[N - 1]) == 0.0                              # clamped: exactly 0
    # the visible count, taken on the device: exact, in the stats and in the workspace header
    stats, ws = _C.reg_loss_forward(torch.empty(0, device=dev), False, [opacity], False, radii, 0.0, 1.0)
    assert int(ws[:8].view(torch.int64)[0]) == int((radii > 0).sum()) == int(stats[3])
    # [N] instead of [N,1]: the same bits, a gradient of that shape
    v1, g1 = _opacity(opacity.reshape(-1), radii)
    assert torch.equal(v1, v) and g1.shape == (N,) and torch.equal(g1, g.reshape(-1))
    # activated=True takes get_opacity
    act = torch.sigmoid(opacity)
    va, ga = _opacity(act, radii, activated=True)
    a64 = act.double().requires_grad_(True)
    w64 = truth.opacity_sparse64(a64, radii, activated=True)
    w64.backward()
    _val_ok(va, w64.detach(), truth.opacity_sparse32(act, radii, activated=True), "opacity sparse activated N=%d" % N)
    _grad_ok(ga, a64.grad, "opacity sparse activated N=%d" % N)


def test_model_list_is_the_concatenation_bit_for_bit(dev):
    sizes = [1000, 0, 63, 257]
    _, opacity, radii = _inputs(sum(sizes), dev, seed=1)
    v, g = _opacity(opacity, radii)
    parts = list(torch.split(opacity, sizes))
    assert [p.shape[0] for p in parts] == sizes
    vl, gl = _opacity(parts, radii)
    assert torch.equal(vl, v)
    assert [tuple(x.shape) for x in gl] == [(n, 1) for n in sizes]
    assert torch.equal(torch.cat(gl), g)
    # separate allocations, one of them a float off its allocation, one flat
    own = []
    for i, p in enumerate(parts):
        buf = torch.empty(p.numel() + 1, device=dev)
        t = buf[1:].view(p.shape) if i == 2 else (p.reshape(-1).clone() if i == 3 else p.clone())
        t.copy_(p.reshape(t.shape))
        own.append(t)
    assert own[2].data_ptr() % 16 == 4
    vo, go = _opacity(own, radii)
    assert torch.equal(vo, v) and torch.equal(torch.cat([x.reshape(-1, 1) for x in go]), g)
    # only zero-length models: nothing visible
    ve, ge = _opacity([opacity[:0], opacity[:0]], radii[:0])
    assert math.isnan(float(ve)) and all(x.shape == (0, 1) for x in ge)


def test_nothing_visible_is_nan_with_a_zero_gradient(dev):
    _, opacity, radii = _inputs(1000, dev)
    v, g = _opacity(opacity, torch.zeros_like(radii))
    assert math.isnan(float(v)) and float(g.abs().max()) == 0.0 and not bool(torch.isnan(g).any())
    v, g = _opacity([opacity[:300], opacity[300:]], -radii.abs())
    assert math.isnan(float(v)) and all(float(x.abs().max()) == 0.0 for x in g)


# ---- both in one call ----

@pytest.mark.parametrize("N,P", [(1000, 70001), (70001, 63)])
def test_gaussian_reg_loss_is_the_weighted_sum(dev, N, P):
    from gaussianrpg_amd import loss
    scaling, _, _ = _inputs(N, dev)
    _, opacity, radii = _inputs(P, dev, seed=2)
    parts = [opacity[: P // 3], opacity[P // 3:]]
    ls, lo = 0.05, 0.3
    vs, gs = _scale(scaling)
    vo, go = _opacity(parts, radii)
    x = scaling.clone().requires_grad_(True)
    ys = [p.clone().requires_grad_(True) for p in parts]
    total, terms = loss.gaussian_reg_loss(scaling=x, opacities=ys, radii=radii, lambda_scale_flatten=ls,
                                          lambda_opacity_sparse=lo)
    total.backward()
    assert set(terms) == {"scale_flatten_loss", "opacity_sparse_loss"}
    assert torch.equal(terms["scale_flatten_loss"], vs) and torch.equal(terms["opacity_sparse_loss"], vo)
    assert not terms["scale_flatten_loss"].requires_grad
    assert torch.equal(total.detach(), ls * vs + lo * vo)
    assert _rel(x.grad, ls * gs.double()) < 1e-6
    for y, g in zip(ys, go):
        assert _rel(y.grad, lo * g.double()) < 1e-6
    # a lambda of 0 or a missing input turns a term off: not evaluated, no gradient
    x = scaling.clone().requires_grad_(True)
    y = opacity.clone().requires_grad_(True)
    only, terms = loss.gaussian_reg_loss(scaling=x, opacities=y, radii=radii, lambda_scale_flatten=ls)
    only.backward()
    assert set(terms) == {"scale_flatten_loss"} and y.grad is None and torch.equal(only.detach(), ls * vs)
    x = scaling.clone().requires_grad_(True)
    only, terms = loss.gaussian_reg_loss(scaling=x, opacities=parts, lambda_scale_flatten=ls,
                                         lambda_opacity_sparse=lo)               # no radii
    assert set(terms) == {"scale_flatten_loss"}
    only, terms = loss.gaussian_reg_loss(opacities=parts, radii=radii, lambda_scale_flatten=ls,
                                         lambda_opacity_sparse=lo)               # no scaling
    assert set(terms) == {"opacity_sparse_loss"} and torch.equal(only.detach(), lo * vo)


def test_identical_calls_give_identical_bits(dev):
    from gaussianrpg_amd import loss
    scaling, opacity, radii = _inputs(70001, dev, seed=3)
    parts = [opacity[:1000], opacity[1000:1000], opacity[1000:]]
    out = []
    for _ in range(2):
        x = scaling.clone().requires_grad_(True)
        ys = [p.clone().requires_grad_(True) for p in parts]
        v, _ = loss.gaussian_reg_loss(scaling=x, opacities=ys, radii=radii, lambda_scale_flatten=0.1,
                                      lambda_opacity_sparse=0.2)
        (g1, *h1) = torch.autograd.grad(v, [x] + ys, retain_graph=True)       # one forward, its backward twice
        (g2, *h2) = torch.autograd.grad(v, [x] + ys)
        assert torch.equal(g1, g2) and all(torch.equal(a, b) for a, b in zip(h1, h2))
        out.append((v.detach(), g1, h1))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert all(torch.equal(a, b) for a, b in zip(out[0][2], out[1][2]))
    # a view one float off its allocation: the bits of the aligned copy
    buf = torch.empty(scaling.numel() + 1, device=dev)
    off = buf[1:].view(scaling.shape)
    off.copy_(scaling)
    assert off.data_ptr() % 16 == 4
    va, ga = _scale(scaling)
    vb, gb = _scale(off)
    assert torch.equal(va, vb) and torch.equal(ga, gb)
    # a strided view is copied
    wide = torch.zeros(scaling.shape[0], 5, device=dev)
    wide[:, 1:4] = scaling
    vc, gc = _scale(wide[:, 1:4])
    assert torch.equal(va, vc) and torch.equal(ga, gc)


# ---- PSNR ----

@pytest.mark.parametrize("C,H,W", [(3, 37, 53), (3, 96, 200), (1, 64, 64)])
def test_psnr(dev, C, H, W):
    from gaussianrpg_amd import loss
    g = torch.Generator().manual_seed(H + W)
    a = torch.rand(C, H, W, generator=g).to(dev)
    b = (a.cpu() + torch.randn(C, H, W, generator=g) * 0.05).clamp(0, 1).to(dev)
    m = (torch.rand(1, H, W, generator=g) < 0.5).to(dev)
    for mask, what in ((None, "no mask"), (m, "mask"), (m[0], "[H,W] mask"), (m.to(torch.uint8), "uint8 mask")):
        v = loss.psnr(a, b, mask)
        assert v.shape == () and v.dtype == torch.float32 and not v.requires_grad
        _val_ok(v, truth.psnr64(a, b, mask), truth.psnr32(a, b, None if mask is None else mask.bool()),
                "psnr %dx%dx%d %s" % (C, H, W, what))
        assert torch.equal(v, loss.psnr(a, b, mask))                         # identical calls, identical bits
    assert math.isnan(float(loss.psnr(a, b, torch.zeros_like(m))))           # an empty selection
    assert float(loss.psnr(a, a.clone())) == float("inf")                    # identical images
    assert float(loss.psnr(a, a.clone(), m)) == float("inf")
    # an input that requires a gradient is accepted; none is provided
    assert not loss.psnr(a.clone().requires_grad_(True), b, m).requires_grad
    # planes one float off their allocation: the bits of the aligned copy
    buf = torch.empty(a.numel() + 1, device=dev)
    off = buf[1:].view(a.shape)
    off.copy_(a)
    assert torch.equal(loss.psnr(off, b, m), loss.psnr(a, b, m))


# ---- the C ABI and the harness ----

class _Seg(ctypes.Structure):
    _fields_ = [("opacity", ctypes.c_void_p), ("grad_opacity", ctypes.c_void_p), ("n", ctypes.c_longlong)]


def test_c_abi_rejects_bad_arguments(dev):
    torch.zeros(1, device=dev)                                # the device is up
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    fwd = lib.grpg_reg_loss_forward
    fwd.restype = ctypes.c_int
    fwd.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                    ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 3
    scaling, opacity, radii = _inputs(63, dev)
    stats = torch.full((4,), -1.0, device=dev)
    lib.grpg_reg_loss_workspace_bytes.restype = ctypes.c_size_t
    ws = torch.zeros(lib.grpg_reg_loss_workspace_bytes(2), dtype=torch.uint8, device=dev)
    segs = (_Seg * 2)(_Seg(opacity.data_ptr(), None, 40), _Seg(opacity.data_ptr() + 160, None, 23))
    ok = (scaling.data_ptr(), 63, 0, ctypes.addressof(segs), 2, 0, radii.data_ptr(), 63, 1.0, 1.0, stats.data_ptr(),
          ws.data_ptr(), None)
    # NULL / misaligned scaling, negative N, NULL table, negative count, NULL radii, radii / sum n mismatch, NULL stats,
    # NULL / misaligned workspace
    for i, bad in ((0, None), (0, scaling.data_ptr() + 2), (1, -1), (3, None), (4, -1), (6, None), (7, 62),
                   (10, None), (11, None), (11, ws.data_ptr() + 4)):
        args = list(ok)
        args[i] = bad
        assert fwd(*args) == -1, i
    bad_segs = (_Seg * 2)(_Seg(None, None, 40), _Seg(opacity.data_ptr() + 160, None, 23))
    args = list(ok)
    args[3] = ctypes.addressof(bad_segs)
    assert fwd(*args) == -1                                   # a NULL array with n > 0
    torch.cuda.synchronize()
    assert float(stats[0]) == -1.0                            # nothing was queued by the rejected calls
    assert fwd(*ok) == 0
    torch.cuda.synchronize()
    assert int(stats[3]) == int((radii > 0).sum())
    ps = lib.grpg_psnr_forward
    ps.restype = ctypes.c_int
    ps.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
    lib.grpg_psnr_workspace_bytes.restype = ctypes.c_size_t
    pws = torch.zeros(lib.grpg_psnr_workspace_bytes(), dtype=torch.uint8, device=dev)
    a = torch.rand(3, 8, 8, device=dev)
    pok = (3, 8, 8, a.data_ptr(), a.data_ptr(), None, stats.data_ptr(), pws.data_ptr(), None)
    for i, bad in ((0, 0), (1, 0), (3, None), (4, None), (3, a.data_ptr() + 1), (6, None), (7, None)):
        args = list(pok)
        args[i] = bad
        assert ps(*args) == -1, i
    assert ps(*pok) == 0
    torch.cuda.synchronize()


def test_train_loss_with_and_without_the_new_terms(dev):
    from gaussianrpg_amd import loss
    g = torch.Generator().manual_seed(2)
    H, W, N = 64, 53, 1000
    scaling, opacity, radii = _inputs(N, dev)
    mono = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).to(dev)
    wvt = torch.eye(4)
    wvt[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    wvt = wvt.to(dev)
    pkg = {"rgb": torch.rand(3, H, W, generator=g).to(dev), "acc": (torch.rand(1, H, W, generator=g) * 0.9 + 0.05).to(dev),
           "depth": (torch.rand(1, H, W, generator=g) * 20).to(dev), "normals": torch.randn(3, H, W, generator=g).to(dev),
           "radii": radii}
    gt_img = torch.rand(3, H, W, generator=g).to(dev)
    sky = (torch.rand(1, H, W, generator=g) < 0.3).to(dev)
    mask = (torch.rand(1, H, W, generator=g) < 0.8).to(dev)
    lidar = (torch.rand(1, H, W, generator=g) * 30).to(dev)
    parts = [opacity[:400], opacity[400:]]
    for kw in (dict(), dict(fused_aux=True), dict(lambda_dssim=0.2, mask=mask)):
        base = hz.train_loss(pkg, gt_img, lidar, sky, **kw)
        # the new keywords at their defaults, and inputs whose lambda is 0: bit-identical
        assert torch.equal(base, hz.train_loss(pkg, gt_img, lidar, sky, mono_normal=None, world_view_transform=None,
                                               lambda_normal_mono=0.0, scaling=None, opacities=None,
                                               lambda_scale_flatten=0.0, lambda_opacity_sparse=0.0, **kw))
        assert torch.equal(base, hz.train_loss(pkg, gt_img, lidar, sky, mono_normal=mono, world_view_transform=wvt,
                                               scaling=scaling, opacities=parts, **kw))
        full = hz.train_loss(pkg, gt_img, lidar, sky, mono_normal=mono, world_view_transform=wvt,
                             lambda_normal_mono=0.1, scaling=scaling, opacities=parts, lambda_scale_flatten=0.05,
                             lambda_opacity_sparse=0.3, **kw)
        want = base + 0.1 * loss.normal_loss(pkg["normals"], mono, wvt, kw.get("mask"), sky)
        want = want + loss.gaussian_reg_loss(scaling=scaling, opacities=parts, radii=radii, lambda_scale_flatten=0.05,
                                             lambda_opacity_sparse=0.3)[0]
        assert torch.equal(full, want)
    assert ntruth.selection(mask, sky, H, W).any()            # 64 rows: the 50-row cut leaves pixels
