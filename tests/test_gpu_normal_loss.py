"""GPU tests of the fused mono-normal loss (gaussianrpg_amd/loss.py, csrc/normal_loss.hip) against the float64
statement of train.py:206-225 behind F.normalize (tests/normal_loss_truth.py) and against the same code run in float32
PyTorch on the device (the reference's own arithmetic).

Bars (those of tests/test_gpu_aux_loss.py and tests/test_gpu_semantic_loss.py): each value within 1e-6 relative of
float64 and no further from it than twice the float32 PyTorch path plus 3e-7 relative; the gradient within relative
L2 1e-5 of float64 autograd; the count exact.  A pixel whose three raw values are exactly 0 has the gradient
g / 1e-12, which dominates any whole-array norm, so the gradient is compared on the zero-norm pixels and on the rest
separately, each against float64, and no pixel is left out of both."""
import ctypes
import math
import os

import pytest
import torch

import normal_loss_truth as truth

pytestmark = pytest.mark.gpu

VAL_REL = 1e-6
VAL_FLOOR = 3e-7      # relative: a few ulp of a float32
GRAD_REL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 37x53: an odd pixel count, a partial wave and a partial workgroup; 64x64: whole workgroups only; 96x200: 75
# workgroups of partials, and the 50-row cut is live
SHAPES = [(37, 53), (64, 64), (96, 200)]
MASKS = ["both", "mask", "sky", "none"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _inputs(H, W, dev, seed=0, zeros=True):
    """Raw planes (continuous random values of mixed length, a few exactly-zero pixels), unit mono normals, a camera
    matrix with a random rotation, 80 % mask, 30 % sky."""
    g = torch.Generator().manual_seed(100 * H + W + seed)
    normals = torch.randn(3, H, W, generator=g) * (torch.rand(1, H, W, generator=g) * 2 + 0.05)
    mono = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    wvt = torch.eye(4)
    wvt[:3, :3] = q
    wvt[3, :3] = torch.randn(3, generator=g) * 10
    mask = torch.rand(1, H, W, generator=g) < 0.8
    sky = torch.rand(1, H, W, generator=g) < 0.3
    if zeros:
        for y, x in ((H - 1, W - 1), (H - 3, 5), (H // 2 + 20 if H > 60 else H - 2, W // 2)):
            normals[:, y, x] = 0.0
            mask[0, y, x], sky[0, y, x] = True, False
    return [t.to(dev) for t in (normals, mono, wvt, mask, sky)]


def _pick(mask, sky, which):
    return (mask if which in ("both", "mask") else None), (sky if which in ("both", "sky") else None)


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
    if g64.numel() == 0 or float(g64.double().abs().max()) == 0.0:
        assert g.numel() == 0 or float(g.abs().max()) == 0.0, what
    else:
        print("%s: gradient rel L2 %.3g" % (what, _rel(g, g64)))
        assert _rel(g, g64) < GRAD_REL, (what, _rel(g, g64))


def _fused(normals, mono, wvt, mask, sky, **kw):
    from gaussianrpg_amd import loss
    x = normals.clone().requires_grad_(True)
    v = loss.normal_loss(x, mono, wvt, mask, sky, **kw)
    v.backward()
    return v.detach(), x.grad


def _check(normals, mono, wvt, mask, sky, what, normalize=True, top_rows=50):
    from gaussianrpg_amd import loss
    kw = dict(normalize=normalize, top_rows=top_rows)
    v, g = _fused(normals, mono, wvt, mask, sky, **kw)
    x64 = normals.double().requires_grad_(True)
    l1, cos, n = truth.terms64(x64, mono, wvt, mask, sky, **kw)
    (l1 + cos).backward()
    l1_32, cos_32, _ = truth.terms32(normals, mono, wvt, mask, sky, **kw)
    assert v.shape == () and v.dtype == torch.float32 and g.shape == normals.shape and n > 0
    t = loss.normal_loss_terms(normals, mono, wvt, mask, sky, **kw)
    assert t["n_selected"].dtype == torch.int64 and int(t["n_selected"]) == n                   # exact
    assert not t["normal_l1_loss"].requires_grad
    _val_ok(v, (l1 + cos).detach(), l1_32 + cos_32, what + " loss")
    _val_ok(t["normal_l1_loss"], l1.detach(), l1_32, what + " l1")
    _val_ok(t["normal_cos_loss"], cos.detach(), cos_32, what + " cos")
    H, W = normals.shape[1:]
    sel = truth.selection(mask, sky, H, W, top_rows).to(normals.device)
    assert float(g[:, ~sel].abs().max() if bool((~sel).any()) else 0.0) == 0.0                  # unselected: exactly 0
    zero = (normals == 0).all(0) & sel if normalize else torch.zeros_like(sel)
    _grad_ok(g[:, ~zero], x64.grad[:, ~zero], what + " (pixels with a norm)")
    _grad_ok(g[:, zero], x64.grad[:, zero], what + " (zero-norm pixels)")
    return v, g, int(zero.sum())


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("H,W", SHAPES)
def test_value_and_gradient(dev, H, W, normalize, which):
    normals, mono, wvt, mask, sky = _inputs(H, W, dev)
    mask, sky = _pick(mask, sky, which)
    top = 50 if H > 50 else 5           # the default cut where it leaves pixels (96x200); 5 rows on the small planes
    _, g, nzero = _check(normals, mono, wvt, mask, sky, "%dx%d normalize=%s %s" % (H, W, normalize, which),
                         normalize=normalize, top_rows=top)
    if normalize and which in ("both", "mask", "none"):
        assert nzero == 3                                    # the planted zero pixels are selected
    if sky is not None:
        assert float(g[:, :top].abs().max()) == 0.0         # the rows that are switched off
    else:
        assert float(g[:, :top].abs().max()) > 0.0          # no sky mask: no row cut


def test_default_row_cut_is_live_at_96x200(dev):
    from gaussianrpg_amd import loss
    normals, mono, wvt, mask, sky = _inputs(96, 200, dev, seed=1)
    _, g, _ = _check(normals, mono, wvt, mask, sky, "96x200 defaults")
    t = loss.normal_loss_terms(normals, mono, wvt, mask, sky)             # top_rows=50 by default
    assert int(t["n_selected"]) == int((mask & ~sky)[0, 50:].sum())
    assert float(g[:, :50].abs().max()) == 0.0 and float(g[:, 50:].abs().max()) > 0.0


def test_row_cut_removes_every_pixel(dev):
    """37x53 with a sky mask and the default 50 rows: NaN, and a gradient of exact zeros with no NaN in it."""
    from gaussianrpg_amd import loss
    normals, mono, wvt, mask, sky = _inputs(37, 53, dev)
    for normalize in (True, False):
        v, g = _fused(normals, mono, wvt, mask, sky, normalize=normalize)
        assert math.isnan(float(v))
        assert not bool(torch.isnan(g).any()) and float(g.abs().max()) == 0.0
        t = loss.normal_loss_terms(normals, mono, wvt, mask, sky, normalize=normalize)
        assert int(t["n_selected"]) == 0 and math.isnan(float(t["normal_l1_loss"]))
        assert math.isnan(float(t["normal_cos_loss"]))
    # an all-false mask without a sky mask
    v, g = _fused(normals, mono, wvt, torch.zeros_like(mask), None)
    assert math.isnan(float(v)) and float(g.abs().max()) == 0.0 and not bool(torch.isnan(g).any())


def test_layouts(dev):
    normals, mono, wvt, mask, sky = _inputs(37, 53, dev, seed=2)
    kw = dict(top_rows=4)
    v, g = _fused(normals, mono, wvt, mask, sky, **kw)
    # a non-contiguous world_view_transform (column-major memory), read through its strides
    wt = wvt.t().contiguous().t()
    assert not wt.is_contiguous() and torch.equal(wt, wvt)
    v1, g1 = _fused(normals, mono, wt, mask, sky, **kw)
    assert torch.equal(v1, v) and torch.equal(g1, g)
    # a [4,4] view into a larger buffer
    big = torch.zeros(6, 8, device=dev)
    big[1:5, 2:6] = wvt
    v2, g2 = _fused(normals, mono, big[1:5, 2:6], mask, sky, **kw)
    assert torch.equal(v2, v) and torch.equal(g2, g)
    # planes one float off their allocation: the bits of the aligned copy
    offs = []
    for t in (normals, mono):
        buf = torch.empty(t.numel() + 1, device=dev)
        off = buf[1:].view(t.shape)
        off.copy_(t)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        offs.append(off)
    v3, g3 = _fused(offs[0], offs[1], wvt, mask, sky, **kw)
    assert torch.equal(v3, v) and torch.equal(g3, g)
    # [H,W] masks, uint8 masks, a permuted view of the planes
    v4, g4 = _fused(normals, mono, wvt, mask[0], sky[0].to(torch.uint8), **kw)
    assert torch.equal(v4, v) and torch.equal(g4, g)
    view = normals.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not view.is_contiguous()
    v5, g5 = _fused(view, mono, wvt, mask, sky, **kw)
    assert torch.equal(v5, v) and torch.equal(g5, g)


def test_identical_calls_give_identical_bits(dev):
    from gaussianrpg_amd import loss
    normals, mono, wvt, mask, sky = _inputs(96, 200, dev, seed=3)
    v1, g1 = _fused(normals, mono, wvt, mask, sky)
    v2, g2 = _fused(normals, mono, wvt, mask, sky)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    t1 = loss.normal_loss_terms(normals, mono, wvt, mask, sky)
    t2 = loss.normal_loss_terms(normals, mono, wvt, mask, sky)
    assert all(torch.equal(t1[k], t2[k]) for k in t1)
    # one forward, its backward twice
    x = normals.clone().requires_grad_(True)
    v = loss.normal_loss(x, mono, wvt, mask, sky)
    (ga,) = torch.autograd.grad(v, x, retain_graph=True)
    (gb,) = torch.autograd.grad(v, x)
    assert torch.equal(ga, gb) and torch.equal(ga, g1)
    # an upstream factor arrives on the device; the zero-norm pixels scale with it like the rest
    x = normals.clone().requires_grad_(True)
    (0.25 * loss.normal_loss(x, mono, wvt, mask, sky)).backward()
    zero = (normals == 0).all(0)
    assert _rel(x.grad[:, ~zero], 0.25 * g1[:, ~zero].double()) < 1e-6
    assert _rel(x.grad[:, zero], 0.25 * g1[:, zero].double()) < 1e-6


def test_c_abi_rejects_bad_arguments(dev):
    torch.zeros(1, device=dev)                                # the device is up
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    fwd = lib.grpg_normal_loss_forward
    fwd.restype = ctypes.c_int
    fwd.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + \
                   [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
    normals, mono, wvt, _, _ = _inputs(8, 8, dev)
    stats = torch.zeros(4, device=dev)
    lib.grpg_normal_loss_workspace_bytes.restype = ctypes.c_size_t
    ws = torch.zeros(lib.grpg_normal_loss_workspace_bytes(8, 8), dtype=torch.uint8, device=dev)
    ok = (8, 8, normals.data_ptr(), mono.data_ptr(), wvt.data_ptr(), 4, 1, None, None, 1, 50, stats.data_ptr(),
          ws.data_ptr(), None)
    # H < 1, NULL normals / mono / rotation, a misaligned plane, top_rows < 0, NULL stats, NULL / misaligned workspace
    for i, bad in ((0, 0), (2, None), (3, None), (4, None), (2, normals.data_ptr() + 2), (10, -1), (11, None),
                   (12, None), (12, ws.data_ptr() + 4)):
        args = list(ok)
        args[i] = bad
        assert fwd(*args) == -1, i
    assert fwd(*ok) == 0
    torch.cuda.synchronize()
    assert math.isfinite(float(stats[0])) and int(stats[3]) == 64        # no mask at all: every pixel
