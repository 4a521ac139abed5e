"""GPU tests of the feature planes of a composed frame (csrc/features.hip, ComposedRasterizer.forward_features):
against the float64 truth of tests/feature_truth.py and against the classic op on the composed tensors.  The scene: a
200x136 camera, a background of 300 Gaussians and actors of 130, 67 and 1 -- no multiple of the 256-thread workgroup,
workgroups that straddle up to three segments, the first actor partly flipped."""
import json
import math
import os

import pytest
import torch

import feature_truth as ft
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu
W, H = 200, 136
COUNTS = (300, 130, 67, 1)
# measured values land next to the bench tools' results (git-ignored); GRPG_RESULTS_DIR names another folder
OUT = os.environ.get("GRPG_RESULTS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "bench_out")


def _logit(p):
    return torch.log(p / (1 - p))


def _build(seed):
    from gaussianrpg_amd.composed import ActorPose, ModelParams
    g = torch.Generator().manual_seed(seed)
    nb = COUNTS[0]
    sc = hz.street_scene(nb, seed=seed, sh_degree=1)
    # log-scales: a permutation of (0, 0.3, 0.6) plus noise of +-0.05 -- the two smallest differ by e^0.2 at least
    def log_scales(n, base):
        steps = torch.tensor([0.0, 0.3, 0.6])[torch.argsort(torch.rand(n, 3, generator=g), dim=1)]
        return base + steps + 0.1 * (torch.rand(n, 3, generator=g) - 0.5)
    bgxyz = sc.means3D.clone()
    bgxyz[:, 2] = 4.0 + 30.0 * torch.rand(nb, generator=g)     # in front of the camera, in view
    bgxyz[:, 0] = (torch.rand(nb, generator=g) - 0.5) * 0.6 * bgxyz[:, 2]
    bgxyz[:, 1] = (torch.rand(nb, generator=g) - 0.5) * 0.4 * bgxyz[:, 2]
    models = [ModelParams(bgxyz, log_scales(nb, math.log(0.15)), sc.rotations * (0.5 + torch.rand(nb, 1, generator=g)),
                          _logit(sc.opacity.clamp(1e-2, 1 - 1e-2)), sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous())]
    poses = [None]
    for k, n in enumerate(COUNTS[1:]):
        F = (3, 1, 2)[k]
        xyz = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([3.0, 1.6, 2.0])
        flip = (torch.rand(n, generator=g) < 0.5) if k == 0 else None
        models.append(ModelParams(xyz, log_scales(n, math.log(0.12)), torch.randn(n, 4, generator=g),
                                  0.5 + torch.randn(n, 1, generator=g), 0.5 * torch.randn(n, F, 3, generator=g),
                                  0.15 * torch.randn(n, 3, 3, generator=g), flip))
        q = torch.randn(4, generator=g)
        q = q / q.norm() * (1.0 + 0.01 * k)
        poses.append(ActorPose(q.tolist(), [-3.0 + 3.0 * k, 0.5, 10.0 + 4.0 * k], 0.2 + 0.3 * k))
    return models, poses


def _tuples(poses):
    return [None if p is None else (p.obj_rot, p.obj_trans, p.fourier_time) for p in poses]


def _conditions(models, poses, campos):
    """(smallest relative gap between the two smallest scales, smallest |dot|) on the float64 truth"""
    means, scales, rots = ft.world(models, _tuples(poses))
    s = torch.sort(scales, dim=1).values
    _, _, dot = ft.normals_of(means, scales, rots, campos.double(), with_details=True)
    return float(((s[:, 1] - s[:, 0]) / s[:, 0]).min()), float(dot.abs().min())


@pytest.fixture(scope="module")
def scene():
    """CPU models / poses, the camera, and per-S semantic arrays; the seed is the first for which no Gaussian sits
    within 1e-3 of a tie in the axis choice or in the sign (asserted by the test that relies on it)."""
    cam = hz.trajectory_camera(2, W=W, H=H, device="cpu")
    for seed in range(11, 40):
        models, poses = _build(seed)
        gap, dot = _conditions(models, poses, cam.campos)
        if gap > 1e-3 and dot > 1e-3:
            break
    g = torch.Generator().manual_seed(77)
    sems = {S: [torch.randn(n, S, generator=g) for n in COUNTS] for S in (3, 12, 15, 17, 30)}
    return models, poses, cam, sems


def _to(m, dev, grad=False, dtype=None):
    f = lambda t: (t.to(dev) if dtype is None else t.to(dev, dtype)).clone().requires_grad_(grad)   # noqa: E731
    return type(m)(*(f(t) for t in m[:6]), None if m.flip is None else m.flip.to(dev))


def _settings(cam, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = type(cam)(*(t.to(dev) if isinstance(t, torch.Tensor) else t for t in cam))
    return GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1, bg=torch.tensor([0.2, 0.1, 0.3], device=dev)))


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm()) / (float(ref.norm()) + 1e-300)


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("S", [0, 3, 17])
def test_compose_features_matches_truth(scene, S, normals):
    """semantic channels bit-exact; axis and sign exact; components within 1e-6 of the float64 value (unit vectors: a
    handful of float32 roundings below 1 is <= 4 * 2^-24 * 4)"""
    from gaussianrpg_amd.composed import compose_features
    models, poses, cam, sems = scene
    dev = torch.device("cuda:0")
    gap, dot = _conditions(models, poses, cam.campos)
    assert gap > 1e-3 and dot > 1e-3, (gap, dot)     # nothing needs exempting
    sem = None if S == 0 else sems[S]
    got = compose_features([_to(m, dev) for m in models], poses, None if sem is None else [s.to(dev) for s in sem],
                           normals, cam.campos.to(dev)).cpu()
    P = sum(COUNTS)
    assert got.shape == (P, 3 * normals + S) and got.dtype == torch.float32
    truth = ft.features(models, _tuples(poses), sem, normals, cam.campos)
    if S:
        assert torch.equal(got[:, 3 * normals:], torch.cat(sem, 0))
    if normals:
        means, scales, rots = ft.world(models, _tuples(poses))
        n64, k, d = ft.normals_of(means, scales, rots, cam.campos.double(), with_details=True)
        R = ft.ct.quaternion_to_matrix(rots)
        col = R[torch.arange(P), :, k]
        # the axis: the got normal is closest to +-column k among the three columns; the sign: that of the truth
        dots = torch.einsum("pi,pic->pc", got[:, :3].double(), R)
        assert torch.equal(dots.abs().argmax(dim=1), k)
        assert torch.equal(torch.sign(torch.sum(got[:, :3].double() * col, 1)), torch.where(d >= 0, 1.0, -1.0).double())
        err = float((got[:, :3].double() - truth[:, :3]).abs().max())
        print("normal components: max |error| %.3e" % err)
        assert err <= 1e-6, err


def test_edge_rows():
    """two equal smallest scales -> the lowest index; a Gaussian at the camera centre -> -R[:, k]; a model without a
    semantic array -> zeros"""
    from gaussianrpg_amd.composed import ModelParams, compose_features, gaussian_normals
    dev = torch.device("cuda:0")
    campos = torch.tensor([1.0, 2.0, 3.0], device=dev)
    xyz = torch.tensor([[1.0, 2.0, 9.0], [1.0, 2.0, 9.0], [1.0, 2.0, 3.0], [1.0, 2.0, 9.0]], device=dev)
    ls = math.log(0.5)
    scaling = torch.tensor([[ls, ls, 0.0], [0.0, ls, ls], [0.0, ls, 0.1], [ls, ls, ls]], device=dev)
    rot = torch.tensor([[0.9, 0.1, 0.2, -0.3]] * 4, device=dev)
    got = gaussian_normals(scaling, rot, xyz, campos).cpu()
    R = ft.ct.quaternion_to_matrix(rot[:1].double().cpu())[0]
    facing = lambda c: c if float(-(xyz[0].cpu().double() - campos.cpu().double()) @ c) >= 0 else -c   # noqa: E731
    for row, k in ((0, 0), (1, 1), (3, 0)):
        assert float((got[row].double() - facing(R[:, k])).abs().max()) <= 1e-6, (row, k)
    assert float((got[2].double() + R[:, 1]).abs().max()) <= 1e-6      # at the camera centre: negated
    # a NULL semantic segment
    m = ModelParams(xyz, scaling, rot, xyz.new_zeros(4, 1), xyz.new_zeros(4, 1, 3), xyz.new_zeros(4, 0, 3))
    sem = torch.arange(12.0, device=dev).reshape(4, 3) + 1
    f = compose_features([m, m, m], [None, None, None], [sem, None, sem]).cpu()
    assert torch.equal(f[:4], sem.cpu()) and not f[4:8].any() and torch.equal(f[8:], sem.cpu())


@pytest.mark.parametrize("S,normals", [(0, True), (15, False), (12, True), (17, True)])
def test_forward_features_equals_classic_op(scene, S, normals):
    """the same render over the same inputs: every plane bit-identical (F = 3, 15, 15 and 20 > RENDER_NSEM = 16: the
    second semantic launch runs), on the training and on the evaluation path"""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.composed import ComposedRasterizer, compose, compose_features
    models, poses, cam, sems = scene
    dev = torch.device("cuda:0")
    rs = _settings(cam, dev)
    ms = [_to(m, dev) for m in models]
    sem = None if S == 0 else [s.to(dev) for s in sems[S]]
    c1, r1, d1, a1, f1 = ComposedRasterizer(rs).forward_features(ms, poses, sem, normals)
    means, scales, rots, opac, shs = compose(ms, poses)
    feats = compose_features(ms, poses, sem, normals, rs.campos)
    c2, r2, d2, a2, f2 = GaussianRasterizer(rs)(means3D=means, means2D=None, opacities=opac, shs=shs, scales=scales,
                                                rotations=rots, semantics=feats)
    torch.cuda.synchronize()
    assert f1.shape == (3 * normals + S, H, W)
    assert int((r1 > 0).sum()) > 250 and int((r1[COUNTS[0]:] > 0).sum()) > 100, "the scene must be in view"
    assert float(f1.abs().max()) > 0
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and torch.equal(d1, d2) and torch.equal(a1, a2)
    assert torch.equal(f1, f2)
    # the training path renders the same planes
    mt = [_to(m, dev, grad=True) for m in models]
    c3, r3, d3, a3, f3 = ComposedRasterizer(rs).forward_features(mt, poses, sem, normals)
    assert c3.requires_grad and (f3.requires_grad or 3 * normals + S == 0)
    assert torch.equal(c3, c1) and torch.equal(f3, f1) and torch.equal(r3, r1) and torch.equal(d3, d1)


def _feature_leaves(models, poses, sem, dev, dtype):
    from gaussianrpg_amd.composed import ActorPose
    ms = [_to(m, dev, grad=True, dtype=dtype) for m in models]
    ps = [None if p is None else ActorPose(torch.tensor(p.obj_rot, device=dev, dtype=dtype, requires_grad=True),
                                           torch.tensor(p.obj_trans, device=dev, dtype=dtype), p.fourier_time)
          for p in poses]
    ss = [s.to(dev, dtype).clone().requires_grad_(True) for s in sem]
    return ms, ps, ss


def test_compose_features_backward_alone(scene):
    """random dL_dfeatures; gradients w.r.t. the raw rotations, obj_rot and the semantic arrays against float64 autograd
    through the truth.  The bar: 4x the error of float32 PyTorch autograd through the same restatement on the same
    inputs (that yardstick is measured, not the kernel).  Semantic gradient bit-exact; two calls, identical bits."""
    from gaussianrpg_amd.composed import compose_features
    models, poses, cam, sems = scene
    dev = torch.device("cuda:0")
    S = 3
    P = sum(COUNTS)
    gF = torch.randn(P, 3 + S, generator=torch.Generator().manual_seed(5))
    campos = cam.campos.to(dev)

    def run_kernel():
        ms, ps, ss = _feature_leaves(models, poses, sems[S], dev, torch.float32)
        (compose_features(ms, ps, ss, True, campos) * gF.to(dev)).sum().backward()
        return ([m.rotation.grad for m in ms], [p.obj_rot.grad for p in ps if p is not None], [s.grad for s in ss],
                [m.xyz.grad for m in ms] + [m.scaling.grad for m in ms])

    def run_truth(dtype):
        ms, ps, ss = _feature_leaves(models, poses, sems[S], dev, dtype)
        f = ft.features(ms, _tuples(ps), ss, True, campos, dtype=dtype)
        (f * gF.to(dev, dtype)).sum().backward()
        return [m.rotation.grad for m in ms], [p.obj_rot.grad for p in ps if p is not None], [s.grad for s in ss]

    k_rot, k_pose, k_sem, k_none = run_kernel()
    k2_rot, k2_pose, k2_sem, _ = run_kernel()
    t_rot, t_pose, t_sem = run_truth(torch.float64)
    y_rot, y_pose, y_sem = run_truth(torch.float32)
    torch.cuda.synchronize()
    assert all(g is None for g in k_none)      # no gradient through the means or the scales
    off = 0
    for i, g in enumerate(k_sem):
        assert torch.equal(g.cpu(), gF[off:off + COUNTS[i], 3:]), i
        off += COUNTS[i]
    for a, b in zip(k_rot + k_pose + k_sem, k2_rot + k2_pose + k2_sem):
        assert torch.equal(a, b)
    for name, ks, ts, ys in (("rotation", k_rot, t_rot, y_rot), ("obj_rot", k_pose, t_pose, y_pose)):
        for i, (k, t, y) in enumerate(zip(ks, ts, ys)):
            assert float(t.abs().max()) > 0
            e_k, e_y = _rel(k, t), _rel(y, t)
            print("%s %d: kernel %.3e, float32 autograd %.3e" % (name, i, e_k, e_y))
            assert e_k <= 4 * e_y, (name, i, e_k, e_y)


def test_full_backward(scene):
    """loss over colour, depth, alpha and the feature planes through forward_features, against autograd through the
    PyTorch composition + the truth features + the classic op: every gradient array within the project's standing
    bar, relative L2 1e-3."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.composed import ActorPose, ComposedRasterizer
    from oracle import compose_torch as ct
    models, poses, cam, sems = scene
    dev = torch.device("cuda:0")
    rs = _settings(cam, dev)
    S, P = 3, sum(COUNTS)
    g = torch.Generator().manual_seed(3)
    gc = torch.randn(3, H, W, generator=g).to(dev)
    gd = (0.1 * torch.randn(1, H, W, generator=g)).to(dev)
    ga = torch.randn(1, H, W, generator=g).to(dev)
    gf = torch.randn(3 + S, H, W, generator=g).to(dev)

    def leaves():
        ms = [_to(m, dev, grad=True) for m in models]
        ps = [None if p is None else ActorPose(torch.tensor(p.obj_rot, device=dev, requires_grad=True),
                                               torch.tensor(p.obj_trans, device=dev, requires_grad=True),
                                               p.fourier_time) for p in poses]
        ss = [s.to(dev).clone().requires_grad_(True) for s in sems[S]]
        return ms, ps, ss, torch.zeros(P, 3, device=dev, requires_grad=True)

    def loss_of(color, depth, alpha, feats):
        return (color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum() + (feats * gf).sum()

    ms, ps, ss, m2d = leaves()
    color, radii, depth, alpha, feats = ComposedRasterizer(rs).forward_features(ms, ps, ss, True, means2D=m2d)
    loss_of(color, depth, alpha, feats).backward()
    mr, pr, sr, m2r = leaves()
    means, scales, rots, opac, shs = ct.compose(mr, _tuples(pr))
    ftr = ft.features(mr, _tuples(pr), sr, True, rs.campos, dtype=torch.float32)
    c2, r2, d2, a2, f2 = GaussianRasterizer(rs)(means3D=means, means2D=m2r, opacities=opac, shs=shs, scales=scales,
                                                rotations=rots, semantics=ftr)
    loss_of(c2, d2, a2, f2).backward()
    torch.cuda.synchronize()
    measured = {"means2D": _rel(m2d.grad, m2r.grad)}
    for i, (a, b) in enumerate(zip(ms, mr)):
        for f in a._fields[:6]:
            ga_, gb_ = getattr(a, f).grad, getattr(b, f).grad
            assert float(gb_.abs().max()) > 0, (i, f)
            measured["model %d %s" % (i, f)] = _rel(ga_, gb_)
    for i, (a, b) in enumerate(zip(ps, pr)):
        if a is not None:
            measured["pose %d rot" % i] = _rel(a.obj_rot.grad, b.obj_rot.grad)
            measured["pose %d trans" % i] = _rel(a.obj_trans.grad, b.obj_trans.grad)
    for i, (a, b) in enumerate(zip(ss, sr)):
        measured["semantic %d" % i] = _rel(a.grad, b.grad)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "features_parity.json"), "w") as fh:
        json.dump({"scene": "200x136, models of %s, S = 3 + normals" % (COUNTS,), "relative_l2": measured}, fh, indent=1)
    print(json.dumps(measured, indent=1))
    worst = max(measured, key=measured.get)
    assert measured[worst] <= 1e-3, (worst, measured[worst])


def _three_models(scene):
    """the background (300), the partly flipped actor (130) and the single-Gaussian actor; W = 200 is no multiple of
    the 16-pixel tile"""
    models, poses, cam, sems = scene
    keep = (0, 1, 3)
    return [models[i] for i in keep], [poses[i] for i in keep], cam, {S: [v[i] for i in keep] for S, v in sems.items()}


def test_training_frame_without_feature_planes_is_forward(scene):
    """forward_features without semantics and normals (F = 0), training: an empty [0,H,W] feature tensor, and the
    frame of forward() on the same inputs -- every plane bit for bit (the forward is deterministic), the same count"""
    from gaussianrpg_amd.composed import ComposedRasterizer
    models, poses, cam, _ = _three_models(scene)
    dev = torch.device("cuda:0")
    rs = _settings(cam, dev)
    ms = [_to(m, dev, grad=True) for m in models]
    plain, feat = ComposedRasterizer(rs), ComposedRasterizer(rs)
    c1, r1, d1, a1 = plain(ms, poses)
    c2, r2, d2, a2, f2 = feat.forward_features(ms, poses, None, normals=False)
    torch.cuda.synchronize()
    assert c1.requires_grad and c2.requires_grad
    assert f2.shape == (0, H, W)
    assert int((r1 > 0).sum()) > 100, "the scene must be in view"
    assert torch.equal(c2, c1) and torch.equal(d2, d1) and torch.equal(a2, a1) and torch.equal(r2, r1)
    assert feat.num_rendered == plain.num_rendered and plain.num_rendered > 0


@pytest.mark.parametrize("S,normals", [(0, False), (3, True)])
def test_backward_of_a_loss_on_alpha_alone(scene, S, normals):
    """only g_alpha reaches the backward (colour, depth and the feature planes arrive as None): every parameter, the
    tensor-valued poses and means2D get a finite gradient of their own shape; of the semantic arrays, the one that
    requires grad gets one and the one that does not gets None"""
    from gaussianrpg_amd.composed import ActorPose, ComposedRasterizer
    models, poses, cam, sems = _three_models(scene)
    dev = torch.device("cuda:0")
    rs = _settings(cam, dev)
    ms = [_to(m, dev, grad=True) for m in models]
    ps = [None if p is None else ActorPose(torch.tensor(p.obj_rot, device=dev, requires_grad=True),
                                           torch.tensor(p.obj_trans, device=dev, requires_grad=True), p.fourier_time)
          for p in poses]
    m2d = torch.zeros(sum(m.xyz.shape[0] for m in ms), 3, device=dev, requires_grad=True)
    # semantics: the background's requires grad, the first actor's does not, the single Gaussian has none
    ss = None if S == 0 else [sems[S][0].to(dev).clone().requires_grad_(True), sems[S][1].to(dev).clone(), None]
    out = ComposedRasterizer(rs).forward_features(ms, ps, ss, normals, means2D=m2d)
    assert out[4].shape == (3 * normals + S, H, W)
    out[3].sum().backward()
    torch.cuda.synchronize()
    leaves = [t for m in ms for t in m[:6]] + [t for p in ps if p is not None for t in (p.obj_rot, p.obj_trans)] + [m2d]
    for t in leaves:
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all())
    assert float(ms[0].opacity.grad.abs().max()) > 0 and float(ms[1].xyz.grad.abs().max()) > 0
    if ss is not None:
        assert ss[0].grad is not None and ss[0].grad.shape == ss[0].shape and bool(torch.isfinite(ss[0].grad).all())
        assert ss[1].grad is None


def test_backward_above_32_channels_is_refused(scene):
    """F = 33: the forward works, a backward is refused with the message of grpg_backward, the next call succeeds"""
    from gaussianrpg_amd.composed import ComposedRasterizer
    models, poses, cam, sems = scene
    dev = torch.device("cuda:0")
    rs = _settings(cam, dev)
    ms = [_to(m, dev) for m in models]
    s30 = [s.to(dev).clone().requires_grad_(True) for s in sems[30]]
    color, radii, depth, alpha, feats = ComposedRasterizer(rs).forward_features(ms, poses, s30, True)
    torch.cuda.synchronize()
    assert feats.shape == (33, H, W) and float(feats[32].detach().abs().max()) > 0
    with pytest.raises(RuntimeError, match="at most 32 semantic channels"):
        feats.sum().backward()
    s12 = [s.to(dev).clone().requires_grad_(True) for s in sems[12]]
    feats = ComposedRasterizer(rs).forward_features(ms, poses, s12, True)[4]
    feats.sum().backward()
    torch.cuda.synchronize()
    assert all(float(s.grad.abs().max()) > 0 for s in s12[:3])


def test_toy_fit_of_semantic_logits(scene):
    """60 Adam steps on the semantic arrays through forward_features + semantic_loss: the loss decreases and ends
    within 2 % of the same fit through the classic-op path (compose + torch.cat + GaussianRasterizer(semantics=)).
    The two paths compute the same values; they differ by the order of the blend backward's float atomics only."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.composed import ComposedRasterizer, compose
    from gaussianrpg_amd.loss import semantic_loss
    models, poses, cam, sems = scene
    dev = torch.device("cuda:0")
    rs = _settings(cam, dev)
    ms = [_to(m, dev) for m in models]
    S = 3
    target = (torch.arange(W, device=dev)[None, :] * S // W).expand(H, W).contiguous().long()[None]
    flat = compose(ms, poses)

    def fit(fused):
        ss = [(0.01 * s).to(dev).clone().requires_grad_(True) for s in sems[S]]
        opt = torch.optim.Adam(ss, lr=0.05)
        losses = []
        for _ in range(60):
            opt.zero_grad(set_to_none=True)
            if fused:
                planes = ComposedRasterizer(rs).forward_features(ms, poses, ss)[4]
            else:
                planes = GaussianRasterizer(rs)(means3D=flat[0], means2D=None, opacities=flat[3], shs=flat[4],
                                                scales=flat[1], rotations=flat[2], semantics=torch.cat(ss, 0))[4]
            loss = semantic_loss(planes, target)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return losses

    a, b = fit(True), fit(False)
    print("toy fit: fused %.6f -> %.6f, classic %.6f -> %.6f" % (a[0], a[-1], b[0], b[-1]))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "features_toy_fit.json"), "w") as fh:
        json.dump({"fused": [a[0], a[-1]], "classic": [b[0], b[-1]]}, fh)
    assert a[-1] < 0.9 * a[0], (a[0], a[-1])
    assert abs(a[-1] - b[-1]) <= 0.02 * b[-1], (a[-1], b[-1])
