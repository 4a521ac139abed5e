"""GPU tests of the fused SSIM + L1 loss (gaussianrpg_amd/loss.py, csrc/ssim.hip) against the float64
statement of loss_utils (tests/ssim_truth.py, pinned to the reference by tests/golden/ref_ssim.npz) and
against the same formula run in float32 through F.conv2d on the device (the reference's own arithmetic).

Bars: values within 1e-5 absolute of float64, gradients within relative L2 1e-3 of float64 autograd, and
neither further from float64 than twice the float32 PyTorch path (plus a floor of a few float32 ulps, for
cases where the float32 path is exact, e.g. 1x1 images or an all-false mask)."""
import math

import numpy as np
import pytest
import torch

import ssim_truth
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

VAL_FLOOR = 1e-7      # ~2 ulp of a float32 near 1
GRAD_FLOOR = 1e-6     # relative L2


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _imgs(shape, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    return a.to(dev), b.to(dev)


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def _grad(fn, a, b, mask):
    t = a.clone().requires_grad_(True)
    v = fn(t, b, mask)
    v.backward()
    return v.detach(), t.grad


def _check_against_truth(kind, a, b, mask, size_average=True):
    from gaussianrpg_amd import loss
    if kind == "ssim":
        fused = lambda x, y, m: loss.ssim(x, y, size_average=size_average, mask=m).sum()
        ref = lambda x, y, m: ssim_truth.ssim(x, y, size_average=size_average, mask=m).sum()
    elif kind == "l1":
        fused = lambda x, y, m: loss.l1_loss(x, y, m)
        ref = lambda x, y, m: ssim_truth.l1(x, y, m)
    else:
        fused = lambda x, y, m: loss.l1_ssim_loss(x, y, m)[0]
        ref = lambda x, y, m: ssim_truth.mix(x, y, m)
    v, g = _grad(fused, a, b, mask)
    v64, g64 = _grad(ref, a.double(), b.double(), mask)
    v32, g32 = _grad(ref, a, b, mask)
    torch.cuda.synchronize()
    if math.isnan(float(v64)):
        assert math.isnan(float(v)), (kind, float(v))
    else:
        e, e32 = abs(float(v) - float(v64)), abs(float(v32) - float(v64))
        assert e < 1e-5, (kind, float(v), float(v64))
        assert e <= 2 * e32 + VAL_FLOOR, (kind, e, e32)
    if float(g64.double().norm()) == 0.0:
        assert float(g.abs().max()) == 0.0
    else:
        r, r32 = _rel(g, g64), _rel(g32, g64)
        assert r < 1e-3, (kind, r)
        assert r <= 2 * r32 + GRAD_FLOOR, (kind, r, r32)


SHAPES = [
    ("1920x1280", (3, 1280, 1920)),
    ("1242x375", (3, 375, 1242)),
    ("37x53", (3, 37, 53)),
    ("1281x1919", (3, 1281, 1919)),
    ("5x7", (3, 5, 7)),
    ("1x1", (3, 1, 1)),
    ("c1", (1, 64, 48)),
]


@pytest.mark.parametrize("kind", ["ssim", "l1", "mix"])
@pytest.mark.parametrize("name,shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_no_mask(dev, name, shape, kind):
    a, b = _imgs(shape, sum(map(ord, name)), dev)
    _check_against_truth(kind, a, b, None)


@pytest.mark.parametrize("kind", ["ssim", "l1", "mix"])
@pytest.mark.parametrize("mask_kind", ["random", "all_true", "all_false"])
@pytest.mark.parametrize("shape", [(3, 37, 53), (3, 375, 1242)], ids=["37x53", "1242x375"])
def test_masks(dev, shape, mask_kind, kind):
    a, b = _imgs(shape, 11, dev)
    H, W = shape[1:]
    if mask_kind == "random":
        m = torch.rand(1, H, W, device=dev) > 0.3
    else:
        m = torch.full((1, H, W), mask_kind == "all_true", dtype=torch.bool, device=dev)
    _check_against_truth(kind, a, b, m)


@pytest.mark.parametrize("size_average", [True, False])
@pytest.mark.parametrize("masked", [False, True])
def test_batched(dev, size_average, masked):
    a, b = _imgs((2, 3, 40, 56), 5, dev)
    m = (torch.rand(2, 1, 40, 56, device=dev) > 0.4) if masked else None
    _check_against_truth("ssim", a, b, m, size_average=size_average)
    if masked:   # a per-channel mask [C,H,W] broadcast over the batch
        m3 = torch.rand(3, 40, 56, device=dev) > 0.5
        _check_against_truth("ssim", a, b, m3, size_average=size_average)


def test_batched_per_image_values(dev):
    from gaussianrpg_amd import loss
    a, b = _imgs((3, 3, 24, 31), 8, dev)
    got = loss.ssim(a, b, size_average=False)
    ref = ssim_truth.ssim(a.double(), b.double(), size_average=False)
    assert got.shape == (3,)
    assert float((got.double() - ref).abs().max()) < 1e-5


@pytest.mark.parametrize("masked", [False, True])
def test_per_image_upstream_weights(dev, masked):
    """size_average=False under unequal upstream weights, one of them negative: .sum() hands every image the same
    coefficient, so only this shows an image that was scaled by its neighbour's.  The file's two gradient bars hold
    for each image's slice on its own, where a wrong coefficient cannot hide in the norm of the batch."""
    from gaussianrpg_amd import loss
    a, b = _imgs((3, 3, 24, 31), 8, dev)
    w = torch.tensor([0.3, -1.7, 2.0], device=dev)
    g = torch.Generator(device="cpu").manual_seed(9)
    m = (torch.rand(3, 1, 24, 31, generator=g) > 0.4).to(dev) if masked else None
    fused = lambda x, y, mm: (loss.ssim(x, y, size_average=False, mask=mm) * w).sum()
    ref = lambda x, y, mm: (ssim_truth.ssim(x, y, size_average=False, mask=mm) * w.to(x.dtype)).sum()
    v, gr = _grad(fused, a, b, m)
    v64, g64 = _grad(ref, a.double(), b.double(), m)
    v32, g32 = _grad(ref, a, b, m)
    torch.cuda.synchronize()
    e, e32 = abs(float(v) - float(v64)), abs(float(v32) - float(v64))
    print("weighted per-image ssim: value %.9g float64 %.9g (float32 torch error %.3g)" % (float(v), float(v64), e32))
    assert e < 1e-5, (float(v), float(v64))
    assert e <= 2 * e32 + VAL_FLOOR, (e, e32)
    for i in range(3):
        r, r32 = _rel(gr[i], g64[i]), _rel(g32[i], g64[i])
        print("image %d (weight %g): gradient rel L2 %.3g (float32 torch %.3g)" % (i, float(w[i]), r, r32))
        assert r < 1e-3, (i, r)
        assert r <= 2 * r32 + GRAD_FLOOR, (i, r, r32)


def test_non_contiguous(dev):
    big_a, big_b = _imgs((3, 90, 2 * 70), 3, dev)
    a, b = big_a[:, 5:85, ::2], big_b[:, 5:85, ::2]
    assert not a.is_contiguous()
    _check_against_truth("mix", a, b, None)
    hwc = big_a.permute(1, 2, 0).contiguous().permute(2, 0, 1)    # channels-last storage
    _check_against_truth("ssim", hwc, big_b, None)


def test_fused_loss_scaled_upstream_and_side_stream(dev):
    from gaussianrpg_amd import loss
    a, b = _imgs((3, 200, 300), 21, dev)
    m = torch.rand(1, 200, 300, device=dev) > 0.2
    t = a.clone().requires_grad_(True)
    l, ll1, ss = loss.l1_ssim_loss(t, b, m)
    assert not ll1.requires_grad and not ss.requires_grad
    (3.7 * l + 0.0 * ll1).backward()
    t64 = a.double().requires_grad_(True)
    (3.7 * ssim_truth.mix(t64, b.double(), m)).backward()
    assert _rel(t.grad, t64.grad) < 1e-3
    assert abs(float(ll1) - float(ssim_truth.l1(a.double(), b.double(), m))) < 1e-5
    assert abs(float(ss) - float(ssim_truth.ssim(a.double(), b.double(), mask=m))) < 1e-5
    # the upstream gradient is a device tensor (0.2 * (1 - ssim) in a larger graph)
    t2 = a.clone().requires_grad_(True)
    s_f = loss.ssim(t2, b, mask=m)
    (s_f * (1 - s_f.detach()) + loss.l1_loss(t2, b, m)).backward()
    t3 = a.double().requires_grad_(True)
    s_r = ssim_truth.ssim(t3, b.double(), mask=m)
    (s_r * (1 - s_r.detach()) + ssim_truth.l1(t3, b.double(), m)).backward()
    assert _rel(t2.grad, t3.grad) < 1e-3
    # non-default stream: same bits as the default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        t4 = a.clone().requires_grad_(True)
        l4 = loss.l1_ssim_loss(t4, b, m)[0]
        (3.7 * l4).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(l4.detach(), l.detach())
    assert torch.equal(t4.grad, t.grad)


def test_deterministic(dev):
    from gaussianrpg_amd import loss
    a, b = _imgs((3, 1280, 1920), 2, dev)
    m = torch.rand(1, 1280, 1920, device=dev) > 0.1
    outs = []
    for _ in range(2):
        t = a.clone().requires_grad_(True)
        l = loss.l1_ssim_loss(t, b, m)[0]
        l.backward()
        outs.append((l.detach().clone(), t.grad.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


# partial slots of the forward: B * C * ceil(W / 32) * ceil(H / 16); the one-workgroup reduce has 1024 threads
EXACT_SHAPES = [
    ("3slots", (3, 1, 1)),
    ("18slots", (3, 37, 53)),
    ("1083slots", (3, 304, 577)),        # some reduce threads add two slots
    ("2166slots", (2, 3, 304, 577)),     # the per-image ranges start at a non-zero slot
]


@pytest.mark.parametrize("name,shape", EXACT_SHAPES, ids=[s[0] for s in EXACT_SHAPES])
def test_exact_sums_through_the_reduction(dev, name, shape):
    """Values from {0, 0.5} against zeros: every partial sum is exactly representable, so the masked L1 mean has
    one right answer whatever the order of the additions, and a slot that is dropped or added twice shows."""
    from gaussianrpg_amd import loss
    g = torch.Generator(device="cpu").manual_seed(sum(shape))
    x1 = (0.5 * torch.randint(0, 2, shape, generator=g).float()).to(dev)
    x2 = torch.zeros_like(x1)
    m = (torch.rand((1,) + shape[-2:], generator=g) > 0.3).to(dev)
    assert bool(m.any())
    want = ((x1 * m).double().sum() / m.expand_as(x1).sum()).float()
    assert torch.equal(loss.l1_loss(x1, x2, m), want)
    if len(shape) == 4:
        per_image = loss.ssim(x1, x2, size_average=False, mask=m)
        for b in range(shape[0]):
            assert torch.equal(per_image[b], loss.ssim(x1[b], x2[b], mask=m))


def test_harness_train_loss_default_unchanged(dev):
    a, b = _imgs((3, 48, 64), 4, dev)
    pkg = {"rgb": a, "acc": torch.rand(1, 48, 64, device=dev), "depth": torch.rand(1, 48, 64, device=dev)}
    assert torch.equal(hz.train_loss(pkg, b), 1.0 * torch.abs(a - b).mean())
    got = hz.train_loss(pkg, b, lambda_dssim=0.2)
    assert abs(float(got) - float(ssim_truth.mix(a.double(), b.double()))) < 1e-5


def test_fit_with_reference_loss_mix(dev):
    """Toy scene -> GaussianRasterizer -> train.py:118 loss mix (lambda_dssim 0.2): the fit through the
    fused loss ends within 0.05 dB PSNR of the same fit through the float32 PyTorch loss."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussianrpg_amd import loss
    cam = hz.trajectory_camera(0, W=64, H=48, device=dev)
    rast = GaussianRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(cam, 0)))
    target_sc = hz.toy_scene(300, seed=40, sh_degree=0, scale=0.25, spread=1.2).to(dev)
    start = hz.toy_scene(300, seed=41, sh_degree=0, scale=0.25, spread=1.2).to(dev)

    def render(p, rot):
        return rast(means3D=p["means3D"], means2D=None, opacities=p["opacity"].clamp(0.01, 0.99), shs=p["shs"],
                    scales=p["scales"].clamp(0.02, 2.0), rotations=rot)[0]

    with torch.no_grad():
        tgt = render({k: getattr(target_sc, k) for k in ("means3D", "opacity", "shs", "scales")},
                     target_sc.rotations)

    def fit(loss_fn):
        p = {k: getattr(start, k).clone().requires_grad_(True) for k in ("means3D", "opacity", "shs", "scales")}
        opt = torch.optim.Adam(p.values(), lr=0.01)
        for _ in range(60):
            opt.zero_grad()
            loss_fn(render(p, start.rotations), tgt).backward()
            opt.step()
        with torch.no_grad():
            img = render(p, start.rotations).clamp(0, 1)
            mse = float(((img - tgt.clamp(0, 1)) ** 2).mean())
        return 10 * math.log10(1.0 / mse)

    fused = fit(lambda img, gt: loss.l1_ssim_loss(img, gt)[0])
    ref = fit(lambda img, gt: ssim_truth.mix(img, gt))
    assert abs(fused - ref) <= 0.05, (fused, ref)
