"""GPU tests of the fused lidar-depth / sky / object-alpha losses (gaussianrpg_amd/loss.py, csrc/aux_loss.hip)
against the float64 statement of train.py (tests/aux_loss_truth.py) and against the same formulas run in float32
PyTorch on the device (the reference's own arithmetic).

Bars: the lidar selection (N, k, the k-th error t) bit for bit; each term within 1e-6 relative of float64 and no
further from it than twice the float32 PyTorch path (plus a floor of a few float32 ulps); gradients within relative
L2 1e-5 of float64 autograd."""
import math

import pytest
import torch

import aux_loss_truth as truth
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

VAL_REL = 1e-6
VAL_FLOOR = 3e-7      # relative: a few ulp of a float32
GRAD_REL = 1e-5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _planes(H, W, seed, dev, coverage=0.66, lead=True):
    g = torch.Generator().manual_seed(seed)
    shape = (1, H, W) if lead else (H, W)
    depth = torch.rand(shape, generator=g) * 60 + 1
    acc = torch.rand(shape, generator=g) * 0.98 + 0.01
    lidar = torch.rand(shape, generator=g) * 80 + 0.5
    lidar[torch.rand(shape, generator=g) >= coverage] = 0
    mask = torch.rand(shape, generator=g) > 0.1
    sky = torch.rand(shape, generator=g) < 0.25
    acc_obj = torch.rand(shape, generator=g)
    bound = torch.rand(shape, generator=g) < 0.3
    return {k: v.to(dev) for k, v in dict(depth=depth, acc=acc, lidar=lidar, mask=mask, sky=sky, acc_obj=acc_obj,
                                          bound=bound).items()}


# the reference's float32 PyTorch code (train.py:121-127,145-158,164-176)
def torch32_lidar(depth, acc, lidar, mask=None):
    depth_mask = lidar > 0.0
    if mask is not None:
        depth_mask = torch.logical_and(depth_mask, mask)
    if torch.nonzero(depth_mask).any():
        expected = depth / (acc + 1e-10)
        err = torch.abs(expected[depth_mask] - lidar[depth_mask])
        err, _ = torch.topk(err, int(0.95 * err.size(0)), largest=False)
        return err.mean()
    return torch.zeros((), device=depth.device)


def torch32_sky(acc, sky, scale=1.0):
    a = torch.clamp(acc, min=1e-6, max=1. - 1e-6)
    v = torch.where(sky, -torch.log(1 - a), -torch.log(a)).mean()
    v *= scale
    return v


def torch32_obj(acc_obj, bound):
    a = torch.clamp(acc_obj, min=1e-6, max=1. - 1e-6)
    return torch.where(bound, -(a * torch.log(a) + (1. - a) * torch.log(1. - a)), -torch.log(1. - a)).mean()


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def _val_ok(v, v64, v32, what):
    v, v64, v32 = float(v), float(v64), float(v32)
    if math.isnan(v64):
        assert math.isnan(v), (what, v)
        return
    e, e32 = abs(v - v64), abs(v32 - v64)
    scale = max(abs(v64), 1e-30)
    assert e <= VAL_REL * scale, (what, v, v64)
    assert e <= 2 * e32 + VAL_FLOOR * scale, (what, e, e32)


def _grads(fn, leaves):
    ts = [t.clone().requires_grad_(True) for t in leaves]
    v = fn(*ts)
    v.backward()
    return v.detach(), [t.grad for t in ts]


def _grad_ok(g, g64, what):
    if float(g64.double().abs().max()) == 0.0:
        assert float(g.abs().max()) == 0.0, what
    else:
        assert _rel(g, g64) < GRAD_REL, (what, _rel(g, g64))


def _check_lidar(p, mask=True):
    from gaussianrpg_amd import loss
    m = p["mask"] if mask else None
    v, (gd, ga) = _grads(lambda d, a: loss.lidar_depth_loss(d, a, p["lidar"], m), (p["depth"], p["acc"]))
    v64, (gd64, ga64) = _grads(lambda d, a: truth.lidar(d, a, p["lidar"], m), (p["depth"].double(), p["acc"].double()))
    v32 = torch32_lidar(p["depth"], p["acc"], p["lidar"], m)
    _val_ok(v, v64, v32, "lidar")
    _grad_ok(gd, gd64, "lidar d/ddepth")
    _grad_ok(ga, ga64, "lidar d/dacc")
    return v, gd, ga


def _check_sky(p, scale=1.0):
    from gaussianrpg_amd import loss
    v, (ga,) = _grads(lambda a: loss.sky_loss(a, p["sky"], scale), (p["acc"],))
    v64, (ga64,) = _grads(lambda a: truth.sky(a, p["sky"], scale), (p["acc"].double(),))
    _val_ok(v, v64, torch32_sky(p["acc"], p["sky"], scale), "sky")
    _grad_ok(ga, ga64, "sky d/dacc")


def _check_obj(p):
    from gaussianrpg_amd import loss
    v, (go,) = _grads(lambda a: loss.obj_acc_loss(a, p["bound"]), (p["acc_obj"],))
    v64, (go64,) = _grads(lambda a: truth.obj(a, p["bound"]), (p["acc_obj"].double(),))
    _val_ok(v, v64, torch32_obj(p["acc_obj"], p["bound"]), "obj")
    _grad_ok(go, go64, "obj d/dacc_obj")


SIZES = [(1280, 1920), (375, 1242)]
COVER = [0.05, 0.66]


@pytest.mark.parametrize("coverage", COVER)
@pytest.mark.parametrize("H,W", SIZES)
def test_selection_is_exact(dev, H, W, coverage):
    from gaussianrpg_amd import loss
    p = _planes(H, W, H + int(100 * coverage), dev, coverage)
    sel = (p["lidar"] > 0) & p["mask"]
    e = torch.abs(p["depth"] / (p["acc"] + 1e-10) - p["lidar"])[sel]
    N = int(sel.sum())
    k = int(0.95 * N)
    t = torch.kthvalue(e, k).values
    s = loss.lidar_selection(p["depth"], p["acc"], p["lidar"], p["mask"])
    assert int(s["N"]) == N and int(s["k"]) == k
    assert int(s["t"].view(torch.int32)) == int(t.view(torch.int32)), (float(s["t"]), float(t))
    assert int(s["c_lt"]) == int((e < t).sum()) and int(s["c_eq"]) == int((e == t).sum())


@pytest.mark.parametrize("coverage", COVER)
@pytest.mark.parametrize("H,W", SIZES)
def test_tie_free_gradient_set_is_the_topk_set(dev, H, W, coverage):
    """acc = 1 (acc + 1e-10 == 1 in float32) and lidar = 1: e = depth - 1 exactly, distinct by construction."""
    from gaussianrpg_amd import loss
    g = torch.Generator().manual_seed(7)
    n = H * W
    sel = (torch.rand(n, generator=g) < coverage).to(dev)
    N = int(sel.sum())
    perm = (torch.randperm(N, generator=g) + 1).to(dev).float()
    depth = torch.full((n,), 1.5, device=dev)
    depth[sel] = 1.0 + perm * 2.0 ** -22
    lidar = torch.where(sel, torch.ones(n, device=dev), torch.zeros(n, device=dev))
    acc = torch.ones(n, device=dev)
    depth, lidar, acc = depth.view(1, H, W), lidar.view(1, H, W), acc.view(1, H, W)
    d = depth.clone().requires_grad_(True)
    loss.lidar_depth_loss(d, acc, lidar).backward()
    e = torch.abs(depth / (acc + 1e-10) - lidar)[lidar > 0]
    idx = torch.nonzero((lidar > 0).view(-1)).view(-1)[torch.topk(e, int(0.95 * N), largest=False).indices]
    got = torch.nonzero(d.grad.view(-1)).view(-1)
    assert torch.equal(torch.sort(idx).values, got)


@pytest.mark.parametrize("coverage", COVER)
@pytest.mark.parametrize("H,W", SIZES)
def test_values_and_gradients(dev, H, W, coverage):
    p = _planes(H, W, 3 * H + int(100 * coverage), dev, coverage)
    _check_lidar(p)
    _check_sky(p)
    _check_obj(p)


@pytest.mark.parametrize("with_obj", [False, True])
def test_combined_matches_terms(dev, with_obj):
    from gaussianrpg_amd import loss
    p = _planes(375, 1242, 5, dev)
    lam = dict(lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.1 if with_obj else 0.0)
    leaves = (p["depth"], p["acc"], p["acc_obj"])
    kw = dict(mask=p["mask"], sky_mask=p["sky"], sky_scale=0.5, obj_bound=p["bound"], **lam)
    ts = [t.clone().requires_grad_(True) for t in leaves]
    l, terms = loss.aux_loss(ts[0], ts[1], lidar_depth=p["lidar"], acc_obj=ts[2], **kw)
    (2.5 * l).backward()
    t64 = [t.double().requires_grad_(True) for t in leaves]
    l64 = truth.total(t64[0], t64[1], lidar_depth=p["lidar"], acc_obj=t64[2], **kw)
    (2.5 * l64).backward()
    assert abs(float(l) - float(l64)) <= 1e-6 * abs(float(l64))
    assert set(terms) == {"lidar_depth_loss", "sky_loss"} | ({"obj_acc_loss"} if with_obj else set())
    assert all(not v.requires_grad for v in terms.values())
    assert abs(float(terms["sky_loss"]) - float(truth.sky(p["acc"], p["sky"], 0.5))) < 1e-6
    for name, g, g64 in zip(("depth", "acc", "acc_obj"), [t.grad for t in ts], [t.grad for t in t64]):
        if name == "acc_obj" and not with_obj:
            assert g is None
            continue
        _grad_ok(g, g64, name)


def test_each_term_alone(dev):
    from gaussianrpg_amd import loss
    p = _planes(64, 96, 9, dev)
    base = dict(lidar_depth=p["lidar"], mask=p["mask"], sky_mask=p["sky"], acc_obj=p["acc_obj"], obj_bound=p["bound"])
    for lam, key in ((dict(lambda_depth_lidar=0.1), "lidar_depth_loss"), (dict(lambda_sky=0.05), "sky_loss"),
                     (dict(lambda_reg=0.1), "obj_acc_loss")):
        l, terms = loss.aux_loss(p["depth"], p["acc"], **base, **lam)
        assert set(terms) == {key}
        assert abs(float(l) - float(truth.total(p["depth"].double(), p["acc"].double(), **base, **lam))) \
            <= 1e-6 * abs(float(l))
    # a missing plane turns its term off
    l, terms = loss.aux_loss(p["depth"], p["acc"], lidar_depth=p["lidar"], lambda_depth_lidar=0.1, lambda_sky=0.05)
    assert set(terms) == {"lidar_depth_loss"}


@pytest.mark.parametrize("scale", [0.0, 0.5])
def test_sky_scale(dev, scale):
    p = _planes(375, 1242, 13, dev)
    _check_sky(p, scale)
    from gaussianrpg_amd import loss
    acc = p["acc"].clone()
    acc.view(-1)[17] = float("nan")
    assert math.isnan(float(loss.sky_loss(acc, p["sky"], scale)))   # NaN * 0 stays NaN


def test_zero_term_cases(dev):
    from gaussianrpg_amd import loss
    p = _planes(5, 7, 1, dev)
    for where, expect_nan in ((None, False), (0, False), (12, True)):
        lidar = torch.zeros_like(p["lidar"])
        if where is not None:
            lidar.view(-1)[where] = 7.0
        d, a = p["depth"].clone().requires_grad_(True), p["acc"].clone().requires_grad_(True)
        v = loss.lidar_depth_loss(d, a, lidar)
        v.backward()
        assert math.isnan(float(v)) == expect_nan and (expect_nan or float(v) == 0.0), (where, float(v))
        assert float(d.grad.abs().max()) == 0.0 and float(a.grad.abs().max()) == 0.0
        s = loss.lidar_selection(p["depth"], p["acc"], lidar)
        assert int(s["N"]) == (0 if where is None else 1) and int(s["k"]) == 0
    # the mask deselects everything
    _check_lidar(dict(p, mask=torch.zeros_like(p["mask"])))


def test_nan_depth_and_acc_edges(dev):
    p = _planes(37, 53, 21, dev, coverage=0.9)
    sel = ((p["lidar"] > 0) & p["mask"]).view(-1)
    idx = torch.nonzero(sel).view(-1)
    p["depth"].view(-1)[idx[3]] = float("nan")          # one NaN error: outside the smallest 95 %
    p["acc"].view(-1)[idx[10]] = 0.0                     # acc exactly 0 at a selected pixel
    p["depth"].view(-1)[idx[10]] = 5e-10                 # ... expected depth 5: a small error, so it is kept
    p["lidar"].view(-1)[idx[10]] = 10.0
    flat = p["acc"].view(-1)
    flat[0], flat[1], flat[2] = 0.0, truth.LO, truth.HI  # sky clamp: outside, on and on the bounds
    p["acc_obj"].view(-1)[:4] = torch.tensor([0.0, truth.LO, truth.HI, 1.0], device=dev)
    v, gd, _ = _check_lidar(p)
    assert float(gd.view(-1)[idx[3]]) == 0.0 and float(gd.view(-1)[idx[10]]) != 0.0
    _check_sky(p)
    _check_obj(p)
    # all selected errors NaN: NaN
    from gaussianrpg_amd import loss
    dn = p["depth"].clone()
    dn.view(-1)[sel] = float("nan")
    assert math.isnan(float(loss.lidar_depth_loss(dn, p["acc"], p["lidar"], p["mask"])))


def test_ties(dev):
    """Integer errors 0..9: the k-th value is tied many times; tied pixels share (k - c_lt) / c_eq."""
    from gaussianrpg_amd import loss
    H, W = 375, 1242
    g = torch.Generator().manual_seed(3)
    lidar = (torch.randint(1, 60, (1, H, W), generator=g).float()).to(dev)
    lidar[:, :, ::3] = 0
    depth = lidar + torch.randint(-9, 10, (1, H, W), generator=g).float().to(dev)
    acc = torch.ones(1, H, W, device=dev)
    d = depth.clone().requires_grad_(True)
    v = loss.lidar_depth_loss(d, acc, lidar)
    v.backward()
    v64 = truth.lidar(depth.double(), acc.double(), lidar)
    w64, N, k, t, c_lt, c_eq, _ = truth.lidar_weights(depth, acc, lidar)
    assert c_eq > 1000 and k - c_lt < c_eq
    assert abs(float(v) - float(v64)) <= 1e-6 * abs(float(v64))
    s = loss.lidar_selection(depth, acc, lidar)
    assert (int(s["N"]), int(s["k"]), float(s["t"]), int(s["c_lt"]), int(s["c_eq"])) == (N, k, t, c_lt, c_eq)
    w = d.grad.abs().double()                            # acc + 1e-10 == 1: |grad| is the weight
    e = torch.abs(depth - lidar)
    n0 = int(((lidar > 0) & (e == 0)).sum())             # sign(0) = 0: weight 1 / k each, no gradient
    assert abs(float(w.sum()) + n0 / k - 1.0) < 1e-5
    tied = (lidar > 0) & (e == t)
    expect = (k - c_lt) / c_eq / k
    assert torch.allclose(w[tied & (e != 0)], torch.full_like(w[tied & (e != 0)], expect), rtol=1e-6, atol=0)
    assert torch.allclose(w[(lidar > 0) & (e < t) & (e != 0)], torch.full((1,), 1.0 / k, dtype=torch.float64,
                                                                          device=dev), rtol=1e-6, atol=0)
    assert _rel(d.grad, torch.where(torch.sign(depth - lidar) != 0, w64 * torch.sign(depth - lidar), 0 * w64)) < 1e-6


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (37, 53), (61, 1)])
def test_small_and_odd_shapes(dev, H, W):
    p = _planes(H, W, H * 100 + W, dev, coverage=0.9)
    if H * W > 2:
        _check_lidar(p)
    _check_sky(p)
    _check_obj(p)


def test_hw_and_1hw_planes_agree(dev):
    from gaussianrpg_amd import loss
    p = _planes(37, 53, 4, dev)
    kw = dict(lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.1)
    l3, _ = loss.aux_loss(p["depth"], p["acc"], lidar_depth=p["lidar"], mask=p["mask"], sky_mask=p["sky"],
                          acc_obj=p["acc_obj"], obj_bound=p["bound"], **kw)
    q = {k: v[0] for k, v in p.items()}
    l2, _ = loss.aux_loss(q["depth"], q["acc"], lidar_depth=q["lidar"], mask=p["mask"], sky_mask=q["sky"],
                          acc_obj=q["acc_obj"], obj_bound=q["bound"].to(torch.uint8), **kw)
    assert torch.equal(l3, l2)
    d = q["depth"].clone().requires_grad_(True)
    loss.lidar_depth_loss(d, q["acc"], q["lidar"]).backward()
    assert d.grad.shape == (37, 53)


def test_upstream_gradients(dev):
    from gaussianrpg_amd import loss
    p = _planes(200, 300, 8, dev)
    leaves = (p["depth"], p["acc"], p["acc_obj"])
    kw = dict(lidar_depth=p["lidar"], mask=p["mask"], sky_mask=p["sky"], obj_bound=p["bound"],
              lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.1)

    def run(fn, ts, terms_fn):
        l = fn(ts)
        # a scaled upstream gradient on the total, and device-tensor upstreams on the terms
        lid = terms_fn(ts)
        (3.7 * l + lid * lid.detach()).backward()
        return [t.grad for t in ts]

    ts = [t.clone().requires_grad_(True) for t in leaves]
    g = run(lambda x: loss.aux_loss(x[0], x[1], acc_obj=x[2], **kw)[0], ts,
            lambda x: loss.lidar_depth_loss(x[0], x[1], p["lidar"], p["mask"]))
    t64 = [t.double().requires_grad_(True) for t in leaves]
    g64 = run(lambda x: truth.total(x[0], x[1], acc_obj=x[2], **kw), t64,
              lambda x: truth.lidar(x[0], x[1], p["lidar"], p["mask"]))
    for name, a, b in zip(("depth", "acc", "acc_obj"), g, g64):
        _grad_ok(a, b, name)


def test_deterministic(dev):
    from gaussianrpg_amd import loss
    p = _planes(1280, 1920, 2, dev)
    outs = []
    for _ in range(2):
        ts = [p[k].clone().requires_grad_(True) for k in ("depth", "acc", "acc_obj")]
        l, _ = loss.aux_loss(ts[0], ts[1], lidar_depth=p["lidar"], mask=p["mask"], sky_mask=p["sky"], acc_obj=ts[2],
                             obj_bound=p["bound"], lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.1)
        l.backward()
        stats = loss.lidar_selection(p["depth"], p["acc"], p["lidar"], p["mask"])
        outs.append([l.detach().clone()] + [t.grad.clone() for t in ts] + [stats["t"].clone(), stats["c_lt"].clone()])
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _sleep_ms(ms):
    torch.cuda._sleep(int(ms * 1e-3 * 2.4e9))      # cycles at ~2.4 GHz


def test_no_host_sync(dev):
    from gaussianrpg_amd import loss
    p = _planes(375, 1242, 6, dev)

    def fused():
        d = p["depth"].clone().requires_grad_(True)
        l, _ = loss.aux_loss(d, p["acc"], lidar_depth=p["lidar"], mask=p["mask"], sky_mask=p["sky"],
                             acc_obj=p["acc_obj"], obj_bound=p["bound"], lambda_depth_lidar=0.1, lambda_sky=0.05,
                             lambda_reg=0.1)
        l.backward()

    def control():
        d = p["depth"].clone().requires_grad_(True)
        torch32_lidar(d, p["acc"], p["lidar"], p["mask"]).backward()

    for fn in (fused, control):   # warm the caching allocator
        fn()
    torch.cuda.synchronize()
    _sleep_ms(50)
    slept = torch.cuda.Event()
    slept.record()
    fused()
    assert not torch.cuda.current_stream().query(), "the fused loss waited for the device"
    assert not slept.query()
    torch.cuda.synchronize()
    _sleep_ms(50)
    slept = torch.cuda.Event()
    slept.record()
    control()
    assert slept.query(), "the PyTorch lidar path was expected to wait for the device"


def test_side_stream(dev):
    from gaussianrpg_amd import loss
    p = _planes(375, 1242, 12, dev)
    kw = dict(lidar_depth=p["lidar"], mask=p["mask"], sky_mask=p["sky"], obj_bound=p["bound"],
              lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.1)

    def run():
        ts = [p[k].clone().requires_grad_(True) for k in ("depth", "acc", "acc_obj")]
        l, _ = loss.aux_loss(ts[0], ts[1], acc_obj=ts[2], **kw)
        l.backward()
        return [l.detach()] + [t.grad for t in ts]

    ref = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def test_harness_fused_aux_at_config5_size(dev):
    """harness.train_loss(fused_aux=True) at P = 1 M, 1920x1280 through the rasterizer: matches the default path,
    and keeps the properties test_config4_train_full_size asserts."""
    sc = hz.street_scene(1_000_000, seed=149).to(dev)
    cam = hz.trajectory_camera(5, device=dev)
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(3, hz.WAYMO_H, hz.WAYMO_W, generator=g).to(dev)
    lidar = (torch.rand(1, hz.WAYMO_H, hz.WAYMO_W, generator=g) * 80.0).to(dev)
    lidar[:, ::2] = 0.0
    sky = (torch.rand(1, hz.WAYMO_H, hz.WAYMO_W, generator=g) < 0.25).to(dev)
    runs = []
    for fused in (False, True):
        leaves = hz.Scene(*(t.clone().requires_grad_(True) if isinstance(t, torch.Tensor) else t for t in sc))
        pkg = hz.render_kernel(leaves, cam, mode="train")
        pkg["acc"].retain_grad()
        pkg["depth"].retain_grad()
        loss = hz.train_loss(pkg, gt, lidar_depth=lidar, sky_mask=sky, fused_aux=fused)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach(), pkg, leaves))
    (l0, p0, _), (l1, p1, leaves) = runs
    assert abs(float(l1) - float(l0)) <= 1e-5 * abs(float(l0))
    assert _rel(p1["acc"].grad, p0["acc"].grad) < GRAD_REL
    assert _rel(p1["depth"].grad, p0["depth"].grad) < GRAD_REL
    vis = p1["visibility_filter"]
    assert 0.3e6 < int(vis.sum()) < 1.0e6
    g2d = p1["viewspace_points"].grad
    for name, t in (("means2D", g2d), ("means3D", leaves.means3D.grad), ("opacity", leaves.opacity.grad),
                    ("shs", leaves.shs.grad), ("scales", leaves.scales.grad), ("rotations", leaves.rotations.grad)):
        assert torch.isfinite(t).all(), name
        assert float(t[~vis].abs().max()) == 0.0, name + ": culled Gaussians must get zero gradient"
        assert float(t[vis].abs().max()) > 0.0, name
    ax = g2d[:, 0].abs() + g2d[:, 1].abs()
    assert bool((g2d[:, 2] >= ax * (1 - 1e-4) - 1e-12).all())


def test_fit_with_full_loss_mix(dev):
    """Toy scene -> GaussianRasterizer -> fused L1 + SSIM plus the lidar, sky and object terms: the fit with the
    fused aux terms ends within 0.05 dB PSNR of the same fit with the float32 PyTorch aux terms."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussianrpg_amd import loss
    cam = hz.trajectory_camera(0, W=64, H=48, device=dev)
    rast = GaussianRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(cam, 0)))
    target_sc = hz.toy_scene(300, seed=40, sh_degree=0, scale=0.25, spread=1.2).to(dev)
    start = hz.toy_scene(300, seed=41, sh_degree=0, scale=0.25, spread=1.2).to(dev)

    def render(p, rot):
        color, _, depth, acc, _ = rast(means3D=p["means3D"], means2D=None, opacities=p["opacity"].clamp(0.01, 0.99),
                                       shs=p["shs"], scales=p["scales"].clamp(0.02, 2.0), rotations=rot)
        return color, depth, acc

    with torch.no_grad():
        tgt, tdepth, tacc = render({k: getattr(target_sc, k) for k in ("means3D", "opacity", "shs", "scales")},
                                   target_sc.rotations)
        lidar = torch.where(tacc > 0.5, tdepth / (tacc + 1e-10), torch.zeros_like(tdepth))
        sky = tacc < 0.2
        bound = tacc > 0.6
        lidar, sky, bound = lidar.reshape(1, 48, 64), sky.reshape(1, 48, 64), bound.reshape(1, 48, 64)

    def fused_aux(depth, acc):
        return loss.aux_loss(depth, acc, lidar_depth=lidar, sky_mask=sky, acc_obj=acc, obj_bound=bound,
                             lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.1)[0]

    def torch_aux(depth, acc):
        return 0.1 * torch32_lidar(depth, acc, lidar) + 0.05 * torch32_sky(acc, sky) + 0.1 * torch32_obj(acc, bound)

    def fit(aux_fn):
        p = {k: getattr(start, k).clone().requires_grad_(True) for k in ("means3D", "opacity", "shs", "scales")}
        opt = torch.optim.Adam(p.values(), lr=0.01)
        for _ in range(60):
            opt.zero_grad()
            img, depth, acc = render(p, start.rotations)
            depth, acc = depth.reshape(1, 48, 64), acc.reshape(1, 48, 64)
            (loss.l1_ssim_loss(img, tgt)[0] + aux_fn(depth, acc)).backward()
            opt.step()
        with torch.no_grad():
            img = render(p, start.rotations)[0].clamp(0, 1)
            mse = float(((img - tgt.clamp(0, 1)) ** 2).mean())
        return 10 * math.log10(1.0 / mse)

    fused = fit(fused_aux)
    ref = fit(torch_aux)
    assert abs(fused - ref) <= 0.05, (fused, ref)
