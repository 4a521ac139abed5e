"""-m gpu: the object-alpha plane of a composed TRAINING frame (csrc/object_alpha.hip, grpg_object_alpha_forward /
grpg_backward_composed_objects, ComposedRasterizer.forward_objects) against what it replaces -- the second
ComposedRasterizer.forward over the object models of train.py:145-158 -- and against the float64 truth.

The plane is not merely close: the main frame's tile lists hold the object entries in the order the objects-only
frame sorts them, the other class contributes T x 1, and the blend arithmetic is blend_math.h's, so alpha_object must
carry the very bits of the objects-only alpha.  Gradients pass through float atomics (like the blend backward) and are
held to the project's gradient bar, relative L2 <= 1e-3 (README).

Scenes are built like _objects_scene of tests/test_gpu_layers.py -- a toy_scene background and three compact
clusters -- as a scene graph: the background in three static models, each cluster an actor with its own pose, the
classes interleaved in concatenation order (background, actor, background, actor, actor, background)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

FLAGS = [False, True, False, True, True, False]
GRAD_BAR = 1e-3
FIELDS = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _logit(p):
    return torch.log(p / (1 - p))


def _raw(sc, g, opacity_mul, scale_mul):
    from gaussianrpg_amd.composed import ModelParams
    n = sc.means3D.shape[0]
    return ModelParams(sc.means3D.contiguous(), torch.log(sc.scales * scale_mul),
                       sc.rotations * (0.5 + torch.rand(n, 1, generator=g)),          # un-normalised, as stored
                       _logit((sc.opacity * opacity_mul).clamp(1e-4, 1 - 1e-4)),
                       sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous())


def _objects_graph(P_bg, P_obj, seed, depth=6.0, opacity_mul=1.0, scale_mul=1.0):
    """(models, poses) on the CPU: models 1, 3, 4 are the actors (FLAGS)."""
    from gaussianrpg_amd.composed import ActorPose
    g = torch.Generator().manual_seed(seed + 1000)
    bg = hz.toy_scene(P_bg, seed=seed, sh_degree=1, depth=depth)
    cuts = [0, P_bg // 3, 2 * P_bg // 3 + 1, P_bg]
    bgs = [hz.Scene(*(t[cuts[i]:cuts[i + 1]] if isinstance(t, torch.Tensor) else t for t in bg)) for i in range(3)]
    centres = [[-1.5, 0.3, depth - 2.0], [1.2, -0.2, depth - 1.0], [0.1, 0.5, depth + 1.5]]
    actors, poses = [], []
    for k, c in enumerate(centres):
        o = hz.toy_scene(P_obj // 3, seed=int(torch.randint(0, 10000, (1,), generator=g)), sh_degree=1, depth=0.0,
                         spread=0.35, scale=0.05)
        actors.append(hz.Scene(o.means3D * torch.tensor([1.0, 1.0, 0.2]), o.opacity.clamp(min=0.6), o.scales,
                               o.rotations, o.shs, 1))
        a = 0.1 + 0.15 * k                                  # a small yaw: the flat side keeps facing the camera
        poses.append(ActorPose([math.cos(a / 2), 0.0, math.sin(a / 2), 0.0], c, 0.0))
    order = [bgs[0], actors[0], bgs[1], actors[1], actors[2], bgs[2]]
    pose_list = [None, poses[0], None, poses[1], poses[2], None]
    return [_raw(s, g, opacity_mul, scale_mul) for s in order], pose_list


def _leaves(models, poses, dev, pose_grad=True):
    """device copies that require grad; actor poses as tensors"""
    from gaussianrpg_amd.composed import ActorPose
    ms = [type(m)(*(t.to(dev).clone().requires_grad_(True) for t in m[:6])) for m in models]
    ps = [None if p is None else ActorPose(torch.tensor(p.obj_rot, device=dev).requires_grad_(pose_grad),
                                           torch.tensor(p.obj_trans, device=dev).requires_grad_(pose_grad), p.fourier_time)
          for p in poses]
    return ms, ps


def _rasterizer(dev, W, H, frame=0):
    from gaussianrpg_amd.composed import ComposedRasterizer
    from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
    cam = hz.trajectory_camera(frame, W=W, H=H, device=dev)
    return ComposedRasterizer(GaussianRasterizationSettings(
        **hz.settings_kwargs(cam, 1, bg=torch.tensor([0.2, 0.1, 0.3], device=dev)))), cam


def _subset(xs, flags=FLAGS):
    return [x for x, f in zip(xs, flags) if f]


def _same_bits(name, a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d values differ, max %.3e" % (
        name, int((a != b).sum()), a.size, float(np.abs(a - b).max()))


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm()) / (float(ref.norm()) + 1e-300)


def _check_forward(dev, models, poses, W, H, object_models, frame=0):
    """forward_objects == (plain forward, forward over the object models alone), bit for bit; training mode"""
    rast, _ = _rasterizer(dev, W, H, frame)
    ms, ps = _leaves(models, poses, dev, pose_grad=False)
    one = rast.forward_objects(ms, ps, object_models)
    main = rast.forward(ms, ps)
    objs = rast.forward(_subset(ms), _subset(ps))
    torch.cuda.synchronize()
    assert one[5].shape == (1, H, W) and one[5].requires_grad
    _same_bits("alpha_object", one[5], objs[3])
    for k, name in enumerate(("color", "radii", "depth", "alpha")):
        if name == "radii":
            assert torch.equal(one[k], main[k])
        else:
            _same_bits(name, one[k], main[k])
    assert one[4].shape == (0, H, W)
    return one


@pytest.fixture(scope="module")
def scene1():
    return _objects_graph(6000, 900, seed=3)


@pytest.fixture(scope="module")
def plane1(dev, scene1):
    """alpha_object of scene 1 at 160x96 (default classes: the frame's own segment table)"""
    return _check_forward(dev, *scene1, 160, 96, None)[5].detach()


def test_forward_bits_default_classes(plane1):
    m = float(plane1.mean())
    assert 0.02 < m < 0.9, m


def test_forward_bits_partial_tiles_explicit_classes(dev, scene1):
    one = _check_forward(dev, *scene1, 200, 136, FLAGS)
    assert 0.02 < float(one[5].detach().mean()) < 0.9
    assert float((one[5] - one[3]).detach().abs().max()) > 0.05      # not the frame's alpha


def test_long_lists_both_binning_algorithms_and_capacity_overflow(dev):
    """thousands of entries per tile, several batches per tile, the 1e-4 stop and the 0.99 clamp"""
    from gaussianrpg_amd.rasterizer import _C
    models, poses = _objects_graph(60000, 6000, seed=11, depth=5.0, opacity_mul=0.35, scale_mul=2.5)
    P = sum(m.xyz.shape[0] for m in models)
    alg = _C.get_binning_algorithm()
    try:
        for a in (1, 0):
            _C.set_binning_algorithm(a)
            _C.reset_capacity_hints()
            one = _check_forward(dev, models, poses, 256, 160, None)
            _check_forward(dev, models, poses, 256, 160, FLAGS, frame=3)   # a speculative frame
        assert float(one[5].detach().max()) > 0.999                # pixels that ran into the 1e-4 stop
        _C.set_capacity_hint(P, 256, 160, 3000, 3000)     # far too small: the forward's tail runs twice
        _check_forward(dev, models, poses, 256, 160, None)
    finally:
        _C.set_binning_algorithm(alg)
        _C.reset_capacity_hints()


def _weights(H, W, dev, seed=5):
    """seeded weights of the three main planes, scaled like the mean in obj_acc_loss (so that neither term of the loss
    drowns the other), and the object bound"""
    g = torch.Generator().manual_seed(seed)
    return ([(torch.randn(c, H, W, generator=g) / (H * W)).to(dev) for c in (3, 1, 1)],
            (torch.rand(1, H, W, generator=g) < 0.5).to(dev))


def _main_loss(out, w):
    return (out[0] * w[0]).sum() + (out[2] * w[1]).sum() + (out[3] * w[2]).sum()


def _grads(ms, ps):
    g = {"%s[%d]" % (f, i): getattr(m, f).grad for i, m in enumerate(ms) for f in FIELDS}
    for i, p in enumerate(ps):
        if p is not None and p.obj_rot.requires_grad:
            g["obj_rot[%d]" % i], g["obj_trans[%d]" % i] = p.obj_rot.grad, p.obj_trans.grad
    return g


def test_degenerate_no_objects_only_objects_empty(dev, scene1):
    from gaussianrpg_amd.loss import obj_acc_loss
    models, poses = scene1
    W, H = 160, 96
    rast, _ = _rasterizer(dev, W, H)
    w, bound = _weights(H, W, dev)
    # no object model: the plane is exactly zero, the backward is the plain one
    results = []
    for objects in (True, False):
        ms, ps = _leaves(models, poses, dev)
        m2 = torch.zeros(sum(m.xyz.shape[0] for m in ms), 3, device=dev, requires_grad=True)
        if objects:
            out = rast.forward_objects(ms, ps, [False] * len(ms), means2D=m2)
            assert float(out[5].detach().abs().max()) == 0.0
            (_main_loss(out, w) + obj_acc_loss(out[5], bound)).backward()
        else:
            _main_loss(rast.forward(ms, ps, means2D=m2), w).backward()
        results.append((_grads(ms, ps), m2.grad))
    for k, v in results[1][0].items():
        r = _rel(results[0][0][k], v)
        assert r <= 1e-5, (k, r)      # the same kernels on the same data: float atomics reorder the sums, no more
    assert _rel(results[0][1], results[1][1]) <= 1e-5
    # ... bit for bit where the sums cannot reorder.  One 16x16 tile with a list below 256 entries is walked by two
    # half-tile waves (render_bwd.hip, light tiles): at most two float atomics per gradient-record word, and a + b ==
    # b + a.  The poses are constants here: the per-actor pose sums of the preprocess backward are float atomics over
    # all of an actor's Gaussians and may reorder; the per-Gaussian parameter gradients do not pass through them.
    tiny = _objects_graph(120, 30, seed=9)
    rast16, _ = _rasterizer(dev, 16, 16)
    w16, bound16 = _weights(16, 16, dev)
    results = []
    for objects in (True, False):
        ms, ps = _leaves(*tiny, dev, pose_grad=False)
        if objects:
            out = rast16.forward_objects(ms, ps, [False] * len(ms))
            (_main_loss(out, w16) + obj_acc_loss(out[5], bound16)).backward()
        else:
            _main_loss(rast16.forward(ms, ps), w16).backward()
        results.append(_grads(ms, ps))
    assert any(float(v.abs().max()) > 0 for v in results[1].values())
    for k, v in results[1].items():
        _same_bits(k, results[0][k], v)
    # only object models: the plane has the bits of alpha
    ms, ps = _leaves(models, poses, dev)
    out = rast.forward_objects(ms, ps, [True] * len(ms))
    _same_bits("alpha_object == alpha", out[5], out[3])
    # under no_grad: the same tuple, no graph
    with torch.no_grad():
        quiet = rast.forward_objects(ms, ps, [True] * len(ms))
    assert len(quiet) == 6 and not quiet[5].requires_grad
    _same_bits("no_grad plane", quiet[5], out[5])
    # P == 0 through the C ABI: a zero plane, no blob looked at
    lib = _lib()
    plane = torch.full((H, W), float("nan"), device=dev)
    ws = torch.empty(lib.grpg_object_alpha_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
    rc = lib.grpg_object_alpha_forward(0, W, H, None, None, None, None, _p(plane), _p(ws),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and float(plane.abs().max()) == 0.0
    # an empty model is refused like ComposedRasterizer.forward refuses it
    empty = type(ms[0])(*(t[:0] for t in ms[0][:6]))
    with pytest.raises(RuntimeError, match="empty"):
        rast.forward_objects([empty], [None])


@pytest.mark.parametrize("which", [1, 2])
def test_gradients_against_the_two_call_route(dev, scene1, which):
    """loss = sum w_c color + sum w_d depth + sum w_a alpha + obj_acc_loss(alpha_object, obj_bound): ONE forward and
    ONE backward chain against the reference's route -- forward on all models, forward on the object models, backward
    of the summed loss"""
    from gaussianrpg_amd.loss import obj_acc_loss
    if which == 1:
        (models, poses), W, H = scene1, 160, 96
    else:
        (models, poses), W, H = _objects_graph(60000, 6000, seed=11, depth=5.0, opacity_mul=0.35, scale_mul=2.5), 256, 160
    rast, _ = _rasterizer(dev, W, H)
    w, bound = _weights(H, W, dev)
    counts = [m.xyz.shape[0] for m in models]
    P = sum(counts)
    obj_rows = torch.repeat_interleave(torch.tensor(FLAGS), torch.tensor(counts)).to(dev)

    ms, ps = _leaves(models, poses, dev)
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    out = rast.forward_objects(ms, ps, None, means2D=m2)
    (_main_loss(out, w) + obj_acc_loss(out[5], bound)).backward()
    one, one_m2 = _grads(ms, ps), m2.grad

    ms, ps = _leaves(models, poses, dev)
    m2a = torch.zeros(P, 3, device=dev, requires_grad=True)
    m2b = torch.zeros(int(obj_rows.sum()), 3, device=dev, requires_grad=True)
    main = rast.forward(ms, ps, means2D=m2a)
    objs = rast.forward(_subset(ms), _subset(ps), means2D=m2b)
    _same_bits("alpha_object", out[5], objs[3])
    (_main_loss(main, w) + obj_acc_loss(objs[3], bound)).backward()
    two = _grads(ms, ps)
    two_m2 = m2a.grad.clone()
    two_m2[obj_rows] += m2b.grad
    torch.cuda.synchronize()

    worst = {}
    for k, ref in two.items():
        r = _rel(one[k], ref)
        worst[k.split("[")[0]] = max(worst.get(k.split("[")[0], 0.0), r)
        print("scene %d  %-18s rel L2 %.3e  |ref| %.3e" % (which, k, r, float(ref.norm())))
    r_m2 = _rel(one_m2, two_m2)
    print("scene %d  means2D            rel L2 %.3e" % (which, r_m2))
    # the object term is really in there: without it the actors' opacity gradient is far off
    assert _rel(main_only_reference(rast, models, poses, dev, w)["opacity[1]"], two["opacity[1]"]) > 10 * GRAD_BAR
    for k, ref in two.items():
        assert _rel(one[k], ref) <= GRAD_BAR, (k, _rel(one[k], ref))
    assert r_m2 <= GRAD_BAR, r_m2


def main_only_reference(rast, models, poses, dev, w):
    ms, ps = _leaves(models, poses, dev)
    _main_loss(rast.forward(ms, ps), w).backward()
    return _grads(ms, ps)


def test_gradients_against_float64(dev, scene1):
    """loss on alpha_object alone; the truth: helpers.float64_truth_gradients on the object subset (gc = gd = 0), carried
    to the raw parameters by float64 autograd through the composition (tests/feature_truth.py world())"""
    import feature_truth as ft
    from helpers import float64_truth_gradients, oracle_kwargs
    from gaussianrpg_amd.composed import compose
    models, poses = scene1
    W, H = 160, 96
    rast, _ = _rasterizer(dev, W, H)
    g = torch.Generator().manual_seed(21)
    ga = torch.randn(1, H, W, generator=g)
    ms, ps = _leaves(models, poses, dev, pose_grad=False)
    out = rast.forward_objects(ms, ps, None)
    (out[5] * ga.to(dev)).sum().backward()
    torch.cuda.synchronize()

    om, op = _subset(models), _subset(poses)
    raw = [type(m)(*(t.double().clone().requires_grad_(True) for t in m[:6])) for m in om]
    means, scales, rots = ft.world(raw, [(p.obj_rot, p.obj_trans) for p in op])
    opac = torch.sigmoid(torch.cat([m.opacity for m in raw]))
    with torch.no_grad():
        shs = compose([type(m)(*(t.to(dev) for t in m[:6])) for m in om], op)[4].cpu()
    cam = hz.trajectory_camera(0, W=W, H=H, device="cpu")
    truth = float64_truth_gradients(hz.Scene(means.detach(), opac.detach(), scales.detach(), rots.detach(), shs, 1),
                                    oracle_kwargs(cam, 1, bg=torch.zeros(3)), torch.zeros(3, H, W),
                                    torch.zeros(1, H, W), ga)
    outs = [means, opac, scales, rots]
    gouts = [torch.from_numpy(np.ascontiguousarray(truth[k])) for k in
             ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations")]
    leaves = [t for m in raw for t in (m.xyz, m.opacity, m.scaling, m.rotation)]
    t64 = torch.autograd.grad(outs, leaves, grad_outputs=gouts)
    got_models = _subset(ms)
    for j, f in enumerate(("xyz", "opacity", "scaling", "rotation")):
        ref = torch.cat([t64[4 * i + j].reshape(-1) for i in range(len(raw))])
        got = torch.cat([getattr(m, f).grad.reshape(-1) for m in got_models])
        r = _rel(got, ref)
        print("%-9s rel L2 vs float64 %.3e  |ref| %.3e" % (f, r, float(ref.norm())))
        assert float(ref.norm()) > 0
        assert r <= GRAD_BAR, (f, r)
    for m in ms:      # the plane knows no colour
        assert float(m.features_dc.grad.abs().max()) == 0.0 and float(m.features_rest.grad.abs().max()) == 0.0


def test_feature_planes_ride_along(dev, scene1):
    """S = 3 semantic channels and the normals (F = 6) with the plane's gradient: grpg_backward_composed_objects at
    F > 0 against forward_features + forward over the object models"""
    from gaussianrpg_amd.loss import obj_acc_loss
    models, poses = scene1
    W, H = 200, 136
    rast, _ = _rasterizer(dev, W, H)
    w, bound = _weights(H, W, dev)
    g = torch.Generator().manual_seed(31)
    wf = (torch.randn(6, H, W, generator=g) / (H * W)).to(dev)
    sem_cpu = [torch.randn(m.xyz.shape[0], 3, generator=g) for m in models]
    routes = []
    for one_call in (True, False):
        ms, ps = _leaves(models, poses, dev)
        sems = [t.to(dev).requires_grad_(True) for t in sem_cpu]
        if one_call:
            out = rast.forward_objects(ms, ps, FLAGS, sems, True)
            plane = out[5]
        else:
            out = rast.forward_features(ms, ps, sems, True)
            plane = rast.forward(_subset(ms), _subset(ps))[3]
        assert out[4].shape == (6, H, W)
        (_main_loss(out, w) + (out[4] * wf).sum() + obj_acc_loss(plane, bound)).backward()
        gr = _grads(ms, ps)
        gr.update({"semantic[%d]" % i: t.grad for i, t in enumerate(sems)})
        routes.append((gr, out[4].detach(), plane.detach()))
    _same_bits("features", routes[0][1], routes[1][1])
    _same_bits("alpha_object", routes[0][2], routes[1][2])
    for k, ref in routes[1][0].items():
        r = _rel(routes[0][0][k], ref)
        print("F = 6  %-18s rel L2 %.3e  |ref| %.3e" % (k, r, float(ref.norm())))
        assert r <= GRAD_BAR, (k, r)


def test_plane_is_deterministic(dev, scene1, plane1):
    rast, _ = _rasterizer(dev, 160, 96)
    ms, ps = _leaves(*scene1, dev, pose_grad=False)
    for _ in range(2):
        _same_bits("repeat", rast.forward_objects(ms, ps, None)[5], plane1)


# ---- the C ABI through ctypes ----
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from gaussianrpg_amd.build import LIB_PATH
    lb = ctypes.CDLL(LIB_PATH)
    for f in ("grpg_forward", "grpg_forward_flags", "grpg_backward", "grpg_object_alpha_forward"):
        getattr(lb, f).restype = ctypes.c_int
    lb.grpg_object_alpha_workspace_bytes.restype = ctypes.c_size_t
    lb.grpg_last_error.restype = ctypes.c_char_p
    return lb


def test_c_abi_flat_training_frame(dev, scene1, plane1):
    """grpg_object_alpha_forward on the blobs of a FLAT training forward (the composition's tensors, an explicit
    layer_class) gives the plane of the composed frame; evaluation blobs and NULL arguments are refused"""
    from test_gpu_cabi_backward import Frame, GRPG_ERR_BAD_BUFFER, GRPG_ERR_INVALID_ARGUMENT, GRPG_FORWARD_NO_BACKWARD
    from gaussianrpg_amd.composed import compose
    models, poses = scene1
    W, H = 160, 96
    lib = _lib()
    with torch.no_grad():
        means, scales, rots, opac, shs = compose([type(m)(*(t.to(dev) for t in m[:6])) for m in models], poses)
    sc = hz.Scene(means.cpu(), opac.cpu(), scales.cpu(), rots.cpu(), shs.cpu(), 1)
    counts = [m.xyz.shape[0] for m in models]
    cls = torch.repeat_interleave(torch.tensor(FLAGS, dtype=torch.uint8), torch.tensor(counts)).to(dev)
    cam = hz.trajectory_camera(0, W=W, H=H)
    fr = Frame(lib, dev, sc, cam)
    nbytes = lib.grpg_object_alpha_workspace_bytes(W, H)
    assert nbytes >= W * H * 4 + ((W + 15) // 16) * ((H + 15) // 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    plane = torch.full((1, H, W), float("nan"), device=dev)
    args = lambda f, **kw: [kw.get("P", f.P), W, H, kw.get("cls", _p(cls)), kw.get("geom", _p(f.geom)),   # noqa: E731
                            _p(f.binning), _p(f.image), kw.get("out", _p(plane)), kw.get("ws", _p(ws)), f.stream]
    rc = lib.grpg_object_alpha_forward(*args(fr))
    torch.cuda.synchronize()
    assert rc == 0, lib.grpg_last_error()
    _same_bits("flat frame's plane", plane, plane1)
    for bad in (dict(out=None), dict(ws=None), dict(geom=None), dict(P=-1)):
        assert lib.grpg_object_alpha_forward(*args(fr, **bad)) == GRPG_ERR_INVALID_ARGUMENT, bad
    # grpg_backward_composed_objects: the plane's three arguments are checked before anything else is looked at
    lib.grpg_backward_composed_objects.restype = ctypes.c_int
    f1 = ctypes.c_float(1.0)
    for k in range(3):
        three = [_p(plane), _p(ws), _p(plane)]
        three[k] = None
        rc = lib.grpg_backward_composed_objects(
            None, None, 0, None, 0, 0, 1, 4, 0, None, W, H, f1, None, None, None, f1, f1, None, None, None, None, None,
            None, None, None, None, None, None, None, None, *three, 0, fr.stream)
        assert rc == GRPG_ERR_INVALID_ARGUMENT, k
    ev = Frame(lib, dev, sc, cam, flags=GRPG_FORWARD_NO_BACKWARD)
    assert lib.grpg_object_alpha_forward(*args(ev)) == GRPG_ERR_BAD_BUFFER
    assert b"evaluation" in lib.grpg_last_error()
