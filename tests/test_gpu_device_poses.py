"""GPU tests of the device-pose hand-over: ``tracks.PoseBatch.rows`` -> ``composed.PoseTable`` -> C ABI
``grpg_bind_device_poses`` -> ``segment_pose_gather_kernel`` (csrc/segment_pose.hip).

The yardstick is the older hand-over of the SAME pose batch through the host, ``PoseBatch.frame`` -> ``PoseRows``: the
gather kernel copies words, so behind it the device segment table holds the bytes the host route uploads, and every
entry point must return the same bits -- ``torch.equal``, no tolerance.  Frames are 64 x 48 (4 x 3 tiles), the
background 2 000 Gaussians, the actors 8-64 Gaussians each (4 at the large segment counts).

Backward gradients are compared bit for bit as well.  That needs a loss the backward sums in ONE order: the blend
backward reduces a splat's gradient inside each wave in a fixed order and then adds it to the splat's record with one
float atomic per wave (csrc/render_bwd.hip), and the order in which different waves arrive changes from run to run --
with a loss over the whole frame the HOST route does not repeat its own bits (measured on the MI355X: 27 of the 6 000
background xyz gradients differ between two runs of ``PoseRows``, by up to 3.1e-5).  The loss here is therefore
supported on one 16 x 4 pixel strip, a quarter tile -- the pixels of one wave in every decomposition the backward
uses (quarter, half and whole-tile waves) -- so every record receives at most one non-zero contribution per kernel
and the sum has one order.  The actors' pose sums are float atomics as well (csrc/preprocess_bwd.hip: one per lane in a
workgroup that spans a model boundary, one per wave and workgroup otherwise), so the backward frames show actors 4, 0
and 3 -- Gaussians 2000-2047, 2048-2055 and 2056-2075 of the frame: each actor inside one wave of one workgroup, its
sum one atomic instruction.  (With actor 2 straddling Gaussian 2048 the host route's opt_rots gradient did not
repeat: 2 of 25 elements, 4.8e-7.)  ``_backward_case`` first asserts that the yardstick repeats its own bits under that
loss; only then does equality with it say anything."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tracks_truth as tt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
SEGMENT_BYTES, POSE_BEGIN, POSE_END = 144, 80, 108     # SegmentDev: rot at 80, trans at 96, the spare word at 108


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _raw(sc, dev, g, fourier=1):
    from gaussianrpg_amd.composed import ModelParams
    n = sc.means3D.shape[0]
    op = sc.opacity.clamp(1e-3, 1 - 1e-3)
    dc = sc.shs[:, :1].contiguous()
    if fourier > 1:
        dc = torch.cat([dc, 0.1 * torch.randn(n, fourier - 1, 3, generator=g)], 1)
    return ModelParams(*(t.to(dev).clone().requires_grad_(True) for t in (
        sc.means3D.contiguous(), torch.log(sc.scales), sc.rotations * (0.5 + torch.rand(n, 1, generator=g)),
        torch.log(op / (1 - op)), dc, sc.shs[:, 1:].contiguous())))


class World:
    """2 000 background Gaussians and five actors (8, 33, 64, 20 and 48 Gaussians; Fourier dimensions 1, 3, 1, 2, 1)
    whose tracklets put them in front of a 64 x 48 camera; a pose batch of T = 3 stamps"""

    def __init__(self, dev):
        from gaussianrpg_amd import harness as hz
        from gaussianrpg_amd.composed import ComposedRasterizer
        from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
        from gaussianrpg_amd.tracks import TrackTable, TrackedActorPoses
        g = torch.Generator().manual_seed(23)
        self.dev = dev
        self.background = _raw(hz.toy_scene(2000, seed=3, sh_degree=1, depth=6.0), dev, g)
        self.actor_models = []
        for k, (n, f) in enumerate(((8, 1), (33, 3), (64, 1), (20, 2), (48, 1))):
            o = hz.toy_scene(n, seed=40 + k, sh_degree=1, depth=0.0, spread=0.3, scale=0.06)
            self.actor_models.append(_raw(hz.Scene(o.means3D, o.opacity.clamp(min=0.6), o.scales, o.rotations, o.shs, 1),
                                          dev, g, f))
        F, A = 5, 5
        tr = tt._empty(F, A)
        spots = ((-1.3, 4.5), (1.1, 5.0), (0.1, 4.0), (-0.5, 5.5), (0.7, 4.4))
        for f in range(F):
            for a, (x, z) in enumerate(spots):
                tr[f, a] = np.concatenate([[a + 1], [x + 0.04 * f, 0.2 - 0.02 * f, z + 0.08 * f],
                                           tt.yaw_quat(0.3 * a + 0.05 * f)])
        stamps = tt.BASE + 0.1 * np.arange(F)
        case = tt.Case(tr, stamps, {a + 1: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1]) for a in range(A)})
        self.actors = TrackedActorPoses(TrackTable.from_tracklets(case.tracklets, case.stamps, case.obj_info), device=dev)
        ot, orr = tt.opt_arrays(case, 4)
        with torch.no_grad():
            self.actors.opt_trans.copy_(torch.from_numpy(ot * 0.2))
            self.actors.opt_rots.copy_(torch.from_numpy(orr))
        ego = np.eye(4, dtype=np.float32)
        ego[:3, 3] = [0.05, -0.03, 0.1]
        self.ego = torch.from_numpy(ego).to(dev)
        self.stamps = [tt.BASE + 0.13, tt.BASE + 0.21, tt.BASE + 0.34]
        cam = hz.trajectory_camera(0, W=64, H=48, device=dev)
        self.settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1, bg=torch.tensor([0.2, 0.1, 0.3], device=dev)))
        self.rast = ComposedRasterizer(self.settings)
        self.campos = self.settings.campos

    def batch(self):
        return self.actors.poses(self.stamps, self.ego)

    def models(self, visible, static=1):
        return [self.background] * static + [self.actor_models[a] for a in visible]

    def params(self, models):
        seen, out = set(), []
        for m in models:
            for t in m[:6]:
                if id(t) not in seen:
                    seen.add(id(t))
                    out.append(t)
        return out + [self.actors.opt_trans, self.actors.opt_rots]


@pytest.fixture(scope="module")
def world(dev):
    return World(dev)


VISIBLE, TIMES, T = [3, 0, 2], [0.7, 0.0, 0.3], 1        # non-monotonic visible list, a stamp inside the batch
BACKWARD = ([4, 0, 3], [0.0, 0.0, 0.7])                  # the backward frames' actors: each inside one wave (above)


def _both(world, visible=VISIBLE, times=TIMES, t=T, static=1, batch=None):
    """the two hand-overs of one pose batch: (PoseTable, PoseRows)"""
    batch = world.batch() if batch is None else batch
    return batch.rows(t, visible, times, static=static), batch.frame(t, visible, times, static=static)


def _same(a, b, what=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), \
            "%s differs: %d of %d elements" % (what, int((a != b).sum()), a.numel())
    else:
        assert a == b, what


def _in_picture(radii, n_background):
    assert int((radii > 0).sum()) > 500 and int((radii[n_background:] > 0).sum()) > 20


# ---- bit identity, per entry point ----

@pytest.mark.parametrize("training", [False, True])
def test_forward(world, training):
    models = world.models(VISIBLE)
    table, rows = _both(world)
    with torch.set_grad_enabled(training):
        a, b = world.rast.forward(models, table), world.rast.forward(models, rows)
    assert (a[0].grad_fn is not None) == training
    _in_picture(a[1], 2000)
    _same(a, b, "forward")


def test_forward_layers(world):
    models = world.models(VISIBLE)
    table, rows = _both(world)
    _same(world.rast.forward_layers(models, table), world.rast.forward_layers(models, rows), "forward_layers")


def test_forward_frame_bytes(world):
    models = world.models(VISIBLE)
    table, rows = _both(world)
    dst_a = torch.empty(48, 64, 3, dtype=torch.uint8, device=world.dev)
    dst_b = torch.empty_like(dst_a)
    a, b = world.rast.forward_frame(models, table, out=dst_a), world.rast.forward_frame(models, rows, out=dst_b)
    assert a["rgb8"].dtype == torch.uint8 and a["rgb8"].is_cuda and int(a["rgb8"].max()) > 0
    _same(a, b, "forward_frame")
    assert torch.equal(dst_a, dst_b)


def _semantics(world, models):
    g = torch.Generator().manual_seed(2)
    return [torch.randn(m.xyz.shape[0], 3, generator=g).to(world.dev).requires_grad_(True) for m in models]


@pytest.mark.parametrize("training", [False, True])
def test_forward_features_and_objects(world, training):
    models = world.models(VISIBLE)
    sems = _semantics(world, models)
    table, rows = _both(world)
    with torch.set_grad_enabled(training):
        _same(world.rast.forward_features(models, table, sems, normals=True),
              world.rast.forward_features(models, rows, sems, normals=True), "forward_features")
        a = world.rast.forward_objects(models, table, semantics=sems, normals=True)
        _same(a, world.rast.forward_objects(models, rows, semantics=sems, normals=True), "forward_objects")
    assert a[4].shape[0] == 6 and float(a[5].detach().max()) > 0


def test_compose_and_compose_features(world):
    from gaussianrpg_amd.composed import compose, compose_features
    models = world.models(VISIBLE)
    sems = _semantics(world, models)
    table, rows = _both(world)
    with torch.no_grad():
        _same(compose(models, table), compose(models, rows), "compose")
        _same(compose_features(models, table, sems, True, world.campos),
              compose_features(models, rows, sems, True, world.campos), "compose_features")
    a = compose_features(models, table, sems, True, world.campos)          # with a graph: its own backward
    b = compose_features(models, _both(world)[1], sems, True, world.campos)
    _same(a, b, "compose_features (training)")
    w = torch.rand(a.shape, generator=torch.Generator().manual_seed(8)).to(world.dev)
    inputs = world.params(models) + sems
    ga = torch.autograd.grad((a * w).sum(), inputs, allow_unused=True)
    gb = torch.autograd.grad((b * w).sum(), inputs, allow_unused=True)
    assert ga[-len(sems) - 1] is not None and float(ga[-len(sems) - 1].abs().max()) > 0   # opt_rots: through obj_rot
    _same([g for g in ga if g is not None], [g for g in gb if g is not None], "compose_features gradients")


def _strip(world, models):
    """[48,64] mask of the 16 x 4 strip (a quarter tile) the actors cover most"""
    with torch.no_grad():
        cover = world.rast.forward_objects(models, _both(world, *BACKWARD)[1])[5][0]
    k = int(cover.view(12, 4, 4, 16).sum((1, 3)).argmax())
    mask = torch.zeros(12, 4, 4, 16, device=world.dev)
    mask[k // 4, :, k % 4, :] = 1.0
    assert float((cover * mask.view(48, 64)).sum()) > 8.0          # the actors are in it
    return mask.view(48, 64)


def _grads(world, render, models, extra=()):
    """gradients of one weighted loss through `render(poses, means2D)` for the PoseTable route, the PoseRows route and
    the PoseRows route once more -> (table, rows, rows again)"""
    out = []
    strip = _strip(world, models)
    for route in (0, 1, 1):
        means2D = torch.zeros(sum(m.xyz.shape[0] for m in models), 3, device=world.dev, requires_grad=True)
        planes = render(_both(world, *BACKWARD)[route], means2D)
        gen = torch.Generator().manual_seed(5)
        loss = sum((p * torch.rand(p.shape, generator=gen).to(world.dev) * strip).sum() for p in planes)
        out.append(torch.autograd.grad(loss, world.params(models) + list(extra) + [means2D]))
    return out


def _backward_case(world, name, render, models, extra=()):
    table, rows, again = _grads(world, render, models, extra)
    k = len(world.params(models))                          # ... whose last two are opt_trans and opt_rots
    assert float(table[k - 2].abs().max()) > 0 and float(table[k - 1].abs().max()) > 0
    for i, (x, y, z) in enumerate(zip(table, rows, again)):
        print("%s gradient %d %s: rows repeat %s, table == rows %s, max |table - rows| %.3e" % (
            name, i, tuple(x.shape), torch.equal(y, z), torch.equal(x, y), float((x - y).abs().max())))
    _same(list(rows), list(again), name + ": the yardstick's own gradients, run twice")
    _same(list(table), list(rows), name + " gradients")


def test_backward_of_forward(world):
    models = world.models(BACKWARD[0])
    _backward_case(world, "forward", lambda poses, m2d: [p for i, p in enumerate(
        world.rast.forward(models, poses, means2D=m2d)) if i != 1], models)


def test_backward_of_forward_features(world):
    models = world.models(BACKWARD[0])
    sems = _semantics(world, models)
    _backward_case(world, "forward_features", lambda poses, m2d: [p for i, p in enumerate(
        world.rast.forward_features(models, poses, sems, normals=True, means2D=m2d)) if i != 1], models, sems)


def test_backward_of_forward_objects(world):
    models = world.models(BACKWARD[0])
    sems = _semantics(world, models)
    _backward_case(world, "forward_objects", lambda poses, m2d: [p for i, p in enumerate(
        world.rast.forward_objects(models, poses, semantics=sems, normals=True, means2D=m2d)) if i != 1], models, sems)


def test_pose_gradient_is_dense_over_the_table(world):
    """the gradient that reaches the batch: [T,A,...], zero at the stamps and actors the frame does not show, and what
    the host route's index_select graph delivers"""
    models = world.models(VISIBLE)
    got = []
    for route in (0, 1):
        batch = world.batch()
        batch.rot.retain_grad()
        batch.trans.retain_grad()
        color = world.rast.forward(models, _both(world, batch=batch)[route])[0]
        (color * torch.rand(color.shape, generator=torch.Generator().manual_seed(5)).to(world.dev)).sum().backward()
        got.append((batch.rot.grad.clone(), batch.trans.grad.clone()))
    g_rot, g_trans = got[0]
    assert tuple(g_rot.shape) == (3, 5, 4) and tuple(g_trans.shape) == (3, 5, 3)
    shown = torch.zeros(3, 5, dtype=torch.bool, device=world.dev)
    shown[T, VISIBLE] = True
    assert not g_rot[~shown].any() and not g_trans[~shown].any()
    assert bool(g_trans[shown].abs().sum(-1).gt(0).all())
    for p in world.params(models):
        p.grad = None


# ---- segment-count boundaries of the gather kernel (256 threads a workgroup, one thread per segment) ----

@pytest.fixture(scope="module")
def crowd(dev):
    """1 023 actors of 4 Gaussians each, cut from one set of tensors, and a pose batch (T = 1) straight from a generator"""
    from gaussianrpg_amd.composed import ModelParams
    from gaussianrpg_amd.tracks import PoseBatch
    g = torch.Generator().manual_seed(77)
    A, n = 1023, 4
    big = [(torch.randn(A * n, 3, generator=g) * 0.05), torch.full((A * n, 3), -3.2), torch.randn(A * n, 4, generator=g),
           torch.full((A * n, 1), 1.5), torch.rand(A * n, 1, 3, generator=g), torch.rand(A * n, 3, 3, generator=g) * 0.1]
    big = [t.to(dev) for t in big]
    models = [ModelParams(*(t[a * n:(a + 1) * n] for t in big)) for a in range(A)]
    rot = torch.nn.functional.normalize(torch.randn(1, A, 4, generator=g), dim=-1)
    trans = torch.stack([torch.rand(A, generator=g) * 3.0 - 1.5, torch.rand(A, generator=g) * 2.0 - 1.0,
                         3.5 + 3.0 * torch.rand(A, generator=g)], -1)[None]
    return models, PoseBatch(rot.to(dev), trans.to(dev).contiguous(), torch.ones(1, A, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("nseg", [1, 2, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024])
def test_segment_count_boundaries(world, crowd, nseg):
    from gaussianrpg_amd.composed import compose
    actor_models, batch = crowd
    order = torch.randperm(1023, generator=torch.Generator().manual_seed(nseg))[:nseg - 1].tolist()
    models = [world.background] + [actor_models[a] for a in order]
    table, rows = batch.rows(0, order), batch.frame(0, order)
    assert list(table.row) == [-1] + order
    with torch.no_grad():
        a, b = compose(models, table), compose(models, rows)       # every segment's means and rotations: no one hides
        _same(a, b, "compose at %d segments" % nseg)
        if nseg > 1:    # ... and the poses did arrive: the last actor's means are not its local ones
            assert not torch.equal(a[0][-4:], models[-1].xyz)
        _same(world.rast.forward(models, table), world.rast.forward(models, rows), "forward at %d segments" % nseg)


# ---- pose-row mixes ----

def test_mix_of_static_device_posed_and_host_posed_models(world):
    """two static models, actors 4 and 1 from the device at t = 2, actor 2 posed by the host (row -1, rigid), then
    actor 4 once more"""
    from gaussianrpg_amd.composed import ActorPose, PoseTable, compose
    batch = world.batch()
    t = 2
    host_rot, host_trans = [0.9689124, 0.0, 0.2474040, 0.0], [0.25, -0.1, 4.75]
    models = [world.background, world.actor_models[3], world.actor_models[4], world.actor_models[2], world.actor_models[1],
              world.actor_models[4]]
    times = [0.0, 0.0, 0.0, 0.4, 0.6, 0.0]
    table = PoseTable(batch.rot[t], batch.trans[t], [-1, -1, 4, -1, 1, 4], [False, False, True, True, True, True], times,
                      [None, None, None, (host_rot, host_trans), None, None])
    listed = [None, None, ActorPose(batch.rot[t, 4], batch.trans[t, 4], 0.0), ActorPose(host_rot, host_trans, 0.4),
              ActorPose(batch.rot[t, 1], batch.trans[t, 1], 0.6), ActorPose(batch.rot[t, 4], batch.trans[t, 4], 0.0)]
    with torch.no_grad():
        _same(compose(models, table), compose(models, listed), "compose of the mix")
        a, b = world.rast.forward(models, table), world.rast.forward(models, listed)
        _same(a, b, "forward of the mix")
        _same(world.rast.forward_layers(models, table), world.rast.forward_layers(models, listed), "layers of the mix")
    _in_picture(a[1], 2000)


def test_same_actor_twice_and_a_later_stamp(world):
    models = world.models([2, 2, 0])
    for t in (0, 2):
        table, rows = _both(world, [2, 2, 0], [0.1, 0.2, 0.0], t)
        with torch.no_grad():
            _same(world.rast.forward(models, table), world.rast.forward(models, rows), "forward at t = %d" % t)
    # the twice-shown actor receives a pose gradient (its exact routing: tests/test_device_poses_host.py)
    batch = world.batch()
    batch.trans.retain_grad()
    world.rast.forward(models, batch.rows(2, [2, 2, 0], [0.1, 0.2, 0.0]))[0].sum().backward()
    assert float(batch.trans.grad[2, 2].abs().max()) > 0 and not batch.trans.grad[2, [1, 3, 4]].any()
    for p in world.params(models):
        p.grad = None


# ---- the table is otherwise untouched ----

def _segment_table(world, models, poses):
    """the device segment table an evaluation forward left in its geometry blob, [n, 144] bytes: found by the six
    parameter pointers its first row starts with"""
    from gaussianrpg_amd.composed import _pack, _rasterize
    lists, pose_t, idft_t = _pack(models, poses)
    with torch.no_grad():
        geom = _rasterize(world.settings, lists, pose_t, idft_t, [], False, 0, False)[6]
    blob = geom.cpu().numpy().tobytes()
    heads = [np.asarray([t.data_ptr() for t in m[:6]], dtype=np.uint64).tobytes() for m in models]
    found, at = [], blob.find(heads[0])
    while at >= 0:      # (a recycled blob may hold an older frame's table elsewhere: every row must be this frame's)
        if all(blob[at + i * SEGMENT_BYTES:at + i * SEGMENT_BYTES + 48] == h for i, h in enumerate(heads)):
            found.append(at)
        at = blob.find(heads[0], at + 1)
    assert len(found) == 1, "the frame's segment table must be found once, found %d times" % len(found)
    return np.frombuffer(blob, np.uint8, len(models) * SEGMENT_BYTES, found[0]).reshape(len(models), SEGMENT_BYTES)


def test_only_the_pose_words_of_bound_rows_change(world):
    from gaussianrpg_amd.composed import PoseTable
    visible, times = [3, 0, 2], [0.7, 0.0, 0.3]
    models = world.models(visible, static=2)
    with torch.no_grad():
        table, rows = _both(world, visible, times, 1, static=2)
        zero = PoseTable(torch.zeros_like(table.rot), torch.zeros_like(table.trans), table.row, table.posed,
                         table.fourier_time)
        bound, hosted, zeroed = (_segment_table(world, models, p) for p in (table, rows, zero))
    assert bound.tobytes() == hosted.tobytes()                     # byte for byte the table of the host route
    differs = bound != zeroed
    assert not differs[:2].any()                                   # static rows: nothing
    assert not differs[:, :POSE_BEGIN].any() and not differs[:, POSE_END:].any()
    assert differs[2:, POSE_BEGIN:POSE_END].any(axis=1).all()      # every bound row took its pose
    assert not zeroed[:, POSE_BEGIN:POSE_END + 4].any()            # zero poses, and the spare word is back at zero
    assert not bound[:, POSE_END:POSE_END + 4].any()
    pose = bound[2:, POSE_BEGIN:POSE_END].copy().view(np.float32).reshape(3, 7)
    want = torch.cat([table.rot[visible], table.trans[visible]], 1).cpu().numpy()
    assert pose.tobytes() == want.tobytes()


# ---- the copy is gone ----

def test_no_host_copy_in_the_pose_hand_over(world):
    """Guarded region: the pose hand-over of an evaluation frame -- ``PoseBatch.rows`` (or ``.frame``) plus the entry
    point's packing step ``composed._pack`` -- under ``torch.cuda.set_sync_debug_mode("error")``.  The PoseTable route
    raises nothing; the PoseRows route raises inside the same region (its ``.cpu()``), which proves the check bites."""
    from gaussianrpg_amd.composed import _pack
    models = world.models(VISIBLE)
    with torch.no_grad():
        batch = world.batch()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            _, pose_arg, _ = _pack(models, batch.rows(T, VISIBLE, TIMES))
            with pytest.raises(RuntimeError, match="synchroniz"):
                _pack(models, batch.frame(T, VISIBLE, TIMES))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert isinstance(pose_arg, tuple) and pose_arg[1].data_ptr() == batch.rot[T].data_ptr()


# ---- binding lifetime ----

def _lists(models):
    from gaussianrpg_amd.composed import _model_lists
    return _model_lists(models)[0]


def test_an_unbound_call_behind_a_bound_one_renders_its_host_poses(world):
    from gaussianrpg_amd.composed import ActorPose
    models = world.models(VISIBLE)
    listed = [None] + [ActorPose([1.0, 0.0, 0.0, 0.0], [0.3 * k - 0.3, 0.0, 4.0 + 0.5 * k], 0.0) for k in range(3)]
    with torch.no_grad():
        before = world.rast.forward(models, listed)
        bound = world.rast.forward(models, _both(world)[0])
        after = world.rast.forward(models, listed)
    _same(before, after, "the unbound call")
    assert not torch.equal(before[0], bound[0])


def test_a_binding_that_does_not_fit_is_refused_and_gone(world):
    """binds through the C ABI itself (the Python binding refuses these two before the library sees them), consumes
    with the extension's compose on the same thread"""
    from gaussianrpg_amd.composed import ActorPose, _pack
    from gaussianrpg_amd.rasterizer import _C
    lib = ctypes.CDLL(LIB)
    lib.grpg_bind_device_poses.restype = ctypes.c_int
    lib.grpg_bind_device_poses.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.grpg_device_poses_bound.restype = ctypes.c_int
    models = world.models(VISIBLE)
    n = len(models)
    listed = [None] + [ActorPose([1.0, 0.0, 0.0, 0.0], [0.3 * k - 0.3, 0.0, 4.0 + 0.5 * k], 0.0) for k in range(3)]
    lists, pose_t, idft_t = _pack(models, listed)
    batch = world.batch()
    rot, trans = batch.rot[0].detach().contiguous(), batch.trans[0].detach().contiguous()
    with torch.no_grad():
        want = _C.compose(*lists, pose_t, idft_t)
        for rows, message in (([-1, 0, 1, 2, 3], "another number of segments"), ([0, 1, 2, 3], "names a static segment")):
            arr = (ctypes.c_int * len(rows))(*rows)
            assert lib.grpg_bind_device_poses(rot.data_ptr(), trans.data_ptr(), arr, len(rows)) == 0
            assert lib.grpg_device_poses_bound() == 1
            with pytest.raises(RuntimeError, match=message):
                _C.compose(*lists, pose_t, idft_t)
            assert lib.grpg_device_poses_bound() == 0
            _same(_C.compose(*lists, pose_t, idft_t), want, "the call behind the refused one")
        # a binding that fits, made the same way, is honoured: the same bits as the PoseTable route
        arr = (ctypes.c_int * n)(-1, 3, 0, 2)
        assert lib.grpg_bind_device_poses(rot.data_ptr(), trans.data_ptr(), arr, n) == 0
        got = _C.compose(*lists, pose_t, idft_t)
        from gaussianrpg_amd.composed import compose
        _same(got, compose(models, batch.rows(0, VISIBLE, [0.0, 0.0, 0.0])), "bound through the C ABI")
        assert not torch.equal(got[0], want[0])


# ---- soak ----

def test_two_hundred_alternating_frames(world):
    """both routes through forward_frame, alternating: the forward's staging buffer is reused by every call"""
    models = world.models(VISIBLE)
    with torch.no_grad():
        batch = world.batch()
        table, rows = batch.rows(T, VISIBLE, TIMES), batch.frame(T, VISIBLE, TIMES)
        want = world.rast.forward_frame(models, rows)["rgb8"].clone()
        bad = 0
        for k in range(200):
            got = world.rast.forward_frame(models, table if k % 2 == 0 else rows)["rgb8"]
            bad += int(not torch.equal(got, want))
    assert bad == 0


def test_training_steps_alternate_through_the_backward_ring(world):
    """twenty forward + backward pairs, routes alternating: the backward's staging ring (8 slots) comes round; the
    forward planes repeat bit for bit and every pose gradient is finite and non-zero"""
    models = world.models(VISIBLE)
    want = None
    for k in range(20):
        batch = world.batch()
        batch.trans.retain_grad()
        color = world.rast.forward(models, _both(world, batch=batch)[k % 2])[0]
        want = color.detach().clone() if want is None else want
        assert torch.equal(color.detach(), want)
        color.sum().backward()
        g = batch.trans.grad[T, VISIBLE]
        assert bool(torch.isfinite(g).all()) and bool(g.abs().sum(-1).gt(0).all())
    for p in world.params(models):
        p.grad = None
