"""GPU tests of the fused tracklet -> actor-pose op (gaussianrpg_amd/tracks.py, csrc/tracks.hip).

Selection: ``chosen`` equals numpy's stable ``argsort(|stamps - t|)[:2]`` exactly.  Values: against the float64
restatement (tests/tracks_truth.py); the yardstick is the float32 restatement's own distance from that truth on the
same inputs, measured here, and the HIP result's group relative L2 and worst row may be at most 4x that (the margin the
project uses for float32 formulas against a float64 truth), floored at 4 float32 ulps of the row's magnitude where
the restatement happens to be exact.  Every value case is first asserted on the CPU to take the same branches in
float32 and float64.  Every figure is collected in bench_out/tracks_parity.json (committed copy:
profiles/tracks_parity.json).  The backward is held to float64 autograd through the restatement under the same rule,
with float32 autograd as the yardstick.
"""
import json
import os

import numpy as np
import pytest
import torch

import tracks_truth as tt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 0.1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _record(name, figures):
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "tracks_parity.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[name] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(name, json.dumps(figures))


def _actors(dev, case, ot=None, orr=None):
    from gaussianrpg_amd.tracks import TrackTable, TrackedActorPoses
    table = TrackTable.from_tracklets(case.tracklets, case.stamps, case.obj_info)
    m = TrackedActorPoses(table, opt_track=ot is not None, camera_timestamps=case.camera_timestamps, device=dev)
    if ot is not None:
        with torch.no_grad():
            m.opt_trans.copy_(torch.from_numpy(ot))
            m.opt_rots.copy_(torch.from_numpy(orr))
    return m


def _poses(m, dev, ts, egos, is_val=False, cam=None):
    b = m.poses(ts, torch.from_numpy(np.stack(egos)).to(dev), is_val=is_val, cam=cam)
    assert b.rot.dtype == torch.float32 and b.active.dtype == torch.uint8 and b.chosen.dtype == torch.int32
    return b, dict(rot=b.rot.detach().cpu().numpy(), trans=b.trans.detach().cpu().numpy(),
                   active=b.active.cpu().numpy(), chosen=b.chosen.cpu().numpy())


def _truths(case, ot, orr, ts, egos, is_val=False, cam=None):
    t32, t64 = tt.Truth(case, ot, orr, torch.float32), tt.Truth(case, ot, orr, torch.float64)
    return t32, t64, t32.batch(ts, egos, is_val, cam), t64.batch(ts, egos, is_val, cam)


def _check(dev, name, case, ts, egos, ot=None, orr=None, is_val=False, cam=None, branches=True):
    """forward on the device against the restatement: chosen / active exactly, values under the 4x rule"""
    if branches:
        assert tt.same_branches(case, ts, ot, orr, is_val, cam) > 0
    m = _actors(dev, case, ot, orr)
    _, got = _poses(m, dev, ts, egos, is_val, cam)
    _, _, f32, f64 = _truths(case, ot, orr, ts, egos, is_val, cam)
    assert np.all(np.isfinite(got["rot"])) and np.all(np.isfinite(got["trans"]))
    report = {}
    try:
        tt.compare(got, f32, f64, report=report, name=name)
    finally:
        if report:
            _record(name, report[name])
    off = got["active"] == 0
    assert np.array_equal(got["rot"][off], np.tile(np.float32([1, 0, 0, 0]), (int(off.sum()), 1)))
    assert not got["trans"][off].any() and (got["chosen"][off] == -1).all()
    return got, f64


def _egos(n, seed=0):
    return [tt.ego_pose(k % 4, seed + k // 4) for k in range(n)]


# ---- selection ----

@pytest.mark.parametrize("L", [2, 63, 64, 65, 130])
def test_selection_at_every_list_length(dev, L):
    """stamps at 1.5e9 + 0.1 k; the closest pair at the head of the list, across the wave boundary (63, 64) and at
    the tail; actor 1 is a two-entry list throughout"""
    case = tt.long_track(L)
    assert abs(case.stamps[0] - 1.5e9) < 1e-6 and np.float32(case.stamps[0]) == np.float32(case.stamps[-1])
    pairs = [(0, 1), (L - 2, L - 1)] + ([(63, 64)] if L >= 65 else []) + ([(L // 2 - 1, L // 2)] if L >= 4 else [])
    ts, want = [], []
    for lo, hi in pairs:
        for frac in (0.3, 0.7):
            ts.append(case.stamps[lo] + frac * (case.stamps[hi] - case.stamps[lo]))
            want.append([lo, hi] if frac < 0.5 else [hi, lo])
    ot, orr = tt.opt_arrays(case, seed=L)
    got, f64 = _check(dev, "selection_L%d" % L, case, ts, _egos(len(ts)), ot, orr)
    assert got["chosen"][:, 0, :2].tolist() == want
    assert (got["chosen"][:, 1, :2] >= 0).all() and (got["chosen"][:, :, 2:] == -1).all()


def test_same_side_pair_extrapolates(dev):
    case = tt.same_side_scene()
    t = tt.BASE + 0.45              # behind the gap: entries 3 (0.15 away) and 2 (0.25) both lie before it
    got, _ = _check(dev, "same_side", case, [t], _egos(1))
    assert got["chosen"][0, 0].tolist() == [3, 2, -1, -1]
    assert case.stamps[3] < t and case.stamps[2] < t


def test_exact_tie_goes_to_the_lower_position(dev):
    """the query sits on entry 4's own stamp: entries 3 and 5 are equally far, and the other entry's weight is zero
    whichever is taken -- the value is entry 4's pose either way, the position must be the lower one"""
    case = tt.tie_scene()
    t = float(case.stamps[4])
    assert abs(case.stamps[3] - t) == abs(case.stamps[5] - t)
    got, _ = _check(dev, "tie", case, [t], _egos(1))
    assert got["chosen"][0, 0].tolist() == [4, 3, -1, -1]


# ---- values and branches ----

QUERIES = [0.33, 2.5 + 0.011, 4.4, 5.62, 6.8]      # in units of the step; 0.33 and 6.8: actor 1 (id 5) is inactive


def _small(seed=0):
    case = tt.small_scene(seed)
    ot, orr = tt.opt_arrays(case, seed)
    return case, ot, orr, [tt.BASE + STEP * q for q in QUERIES]


def test_values_with_every_ego_candidate_and_an_inactive_actor_in_the_middle(dev):
    case, ot, orr, ts = _small()
    got, _ = _check(dev, "small_scene", case, ts, _egos(5), ot, orr)
    assert got["active"].tolist() == [[1, 0, 1], [1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 0, 1]]
    assert got["chosen"][4, 0, :2].tolist() == [7, 6]      # q0 . q1 < 0 lies between entries 4 / 5 / 6 of actor 0


def test_opt_track_off(dev):
    case, _, _, ts = _small(1)
    _check(dev, "opt_absent", case, ts, _egos(5, 1))


@pytest.mark.parametrize("with_opt", [False, True])
def test_slerp_branches(dev, with_opt):
    """equal adjacent rotations (W = 0: finite, q0), q0 . q1 < 0, W near pi / 2, raw angle near pi -- each under each
    of the four matrix_to_quaternion candidates"""
    case = tt.branch_scene()
    ot = orr = None
    if with_opt:
        ot, orr = tt.opt_arrays(case, 2, zero_cells=[(1, 0), (2, 0)])
    ts = [tt.BASE + STEP * q for q in (1.2, 1.45, 1.7, 1.93)]
    got, f64 = _check(dev, "branches_opt%d" % with_opt, case, ts, _egos(4), ot, orr)
    assert got["chosen"][:, :, :2].tolist() == [[[1, 2]] * 4, [[1, 2]] * 4, [[2, 1]] * 4, [[2, 1]] * 4]
    # W = 0: the rotation is q_e (x) normalize(q0) at every step
    q0 = torch.from_numpy(case.tracklets[1, 0, 4:8])
    for k, ego in enumerate(_egos(4)):
        qe = tt.matrix_to_quaternion(torch.from_numpy(ego[:3, :3]).double().unsqueeze(0))
        want = tt.quaternion_raw_multiply(qe, torch.nn.functional.normalize(q0.unsqueeze(0)))[0].numpy()
        assert np.abs(got["rot"][k, 0] - want).max() < 16 * tt.EPS32


@pytest.mark.parametrize("cam,paths", [(0, "camera stamps"), (1, "fallback")])
def test_validation_frame(dev, cam, paths):
    case, ot, orr, ts = _small(2)
    got, _ = _check(dev, "validation_cam%d" % cam, case, ts, _egos(5, 2), ot, orr, is_val=True, cam=cam)
    four = (got["chosen"][..., 2:] >= 0).all(-1)
    if cam == 0:
        assert four[got["active"] == 1].all()               # every actor's span holds two of camera 0's stamps
    else:
        assert not four.any()                               # one stamp: get_tracking_*_ at the frame's own stamp
    # the plain path of the same frame is a different pose where the camera stamps are used
    plain = _poses(_actors(dev, case, ot, orr), dev, ts, _egos(5, 2))[1]
    assert (np.abs(plain["rot"] - got["rot"]).max() > 1e-5) == (cam == 0)


def test_boundary_cases_are_finite(dev):
    """forward only, either side accepted: a slerp at the small-angle switch and one with q0 . q1 = 0"""
    case = tt.branch_scene()
    q = case.tracklets[1, :, 4:8].copy()
    tr = case.tracklets.copy()
    tr[2, 0, 4:8] = tt._qmul_np(q[0], tt.yaw_quat(2 * np.arccos(tt.SMALL_C)))
    tr[2, 1, 4:8] = tt._qmul_np(q[1], tt.yaw_quat(np.pi))
    case = tt.Case(tr, case.stamps, case.obj_info)
    _, got = _poses(_actors(dev, case), dev, [tt.BASE + 0.14], _egos(1))
    assert np.all(np.isfinite(got["rot"])) and np.all(np.isfinite(got["trans"]))
    f64 = tt.Truth(case, None, None, torch.float64).batch([tt.BASE + 0.14], _egos(1))["rot"].numpy()
    assert np.abs(got["rot"][0, 0] - f64[0, 0]).max() < 1e-5                           # continuous across the switch
    assert np.abs(np.linalg.norm(got["rot"][0], axis=-1) - 1).max() < 1e-3             # either arc: a unit rotation


# ---- batching and repeatability ----

def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("is_val", [False, True])
def test_a_batch_equals_single_calls_and_repeats(dev, is_val):
    case, ot, orr, ts = _small(3)
    m, egos = _actors(dev, case, ot, orr), _egos(5, 3)
    _, whole = _poses(m, dev, ts, egos, is_val, 0 if is_val else None)
    _, again = _poses(m, dev, ts, egos, is_val, 0 if is_val else None)
    for k in whole:
        assert _bits(whole[k], again[k]), k
    for i in range(5):
        _, one = _poses(m, dev, ts[i:i + 1], egos[i:i + 1], is_val, 0 if is_val else None)
        for k in whole:
            assert _bits(whole[k][i:i + 1], one[k]), (k, i)


# ---- backward ----

def _backward(dev, name, case, ot, orr, ts, egos, is_val=False, cam=None, seed=0):
    assert tt.same_branches(case, ts, ot, orr, is_val, cam) > 0
    rng = np.random.RandomState(700 + seed)
    A = case.shape[2]
    g_rot = rng.normal(0, 1, (len(ts), A, 4)).astype(np.float32)
    g_trans = rng.normal(0, 1, (len(ts), A, 3)).astype(np.float32)
    m = _actors(dev, case, ot, orr)
    b, got = _poses(m, dev, ts, egos, is_val, cam)
    assert b.rot.requires_grad and b.trans.requires_grad and not b.active.requires_grad
    loss = (b.rot * torch.from_numpy(g_rot).to(dev)).sum() + (b.trans * torch.from_numpy(g_trans).to(dev)).sum()
    loss.backward()
    grads = dict(g_opt_trans=m.opt_trans.grad.cpu().numpy(), g_opt_rots=m.opt_rots.grad.cpu().numpy())
    assert grads["g_opt_trans"].shape == ot.shape and grads["g_opt_rots"].shape == orr.shape
    t32, t64, f32, f64 = _truths(case, ot, orr, ts, egos, is_val, cam)
    r32 = dict(zip(grads, t32.gradients(f32, g_rot, g_trans)))
    r64 = dict(zip(grads, t64.gradients(f64, g_rot, g_trans)))
    report = {}
    try:
        tt.compare(grads, r32, r64, groups=tuple(grads), report=report, name=name)
    finally:
        if report:
            _record(name, report[name])
    # dense: exact zeros wherever the truth has none -- untouched cells, cells of id -1, cells of inactive rows
    touched = np.zeros(case.shape[:2], bool)
    for t in range(len(ts)):
        for a in range(A):
            for p in got["chosen"][t, a]:
                if p >= 0:
                    touched[tuple(case.track_idx[a][p])] = True
    assert touched.any() and not touched.all()
    assert not grads["g_opt_trans"][~touched].any() and not grads["g_opt_rots"][~touched].any()
    assert not grads["g_opt_trans"][case.tracklets[..., 0] == -1].any()
    assert np.array_equal(r64["g_opt_trans"][~touched], np.zeros_like(r64["g_opt_trans"][~touched]))
    assert grads["g_opt_trans"][touched].all(-1).any() and grads["g_opt_rots"][touched].any()
    return m, grads, (g_rot, g_trans)


def test_backward_against_float64_autograd(dev):
    case, ot, orr, ts = _small(4)
    _backward(dev, "backward_small_scene", case, ot, orr, ts, _egos(5, 4))


def test_backward_of_a_validation_frame(dev):
    case, ot, orr, ts = _small(5)
    _backward(dev, "backward_validation", case, ot, orr, ts, _egos(5, 5), is_val=True, cam=0, seed=1)


def test_backward_through_the_slerp_branches(dev):
    case = tt.branch_scene()
    ot, orr = tt.opt_arrays(case, 6, zero_cells=[(1, 0), (2, 0)])
    ts = [tt.BASE + STEP * q for q in (1.2, 1.45, 1.7, 1.93)]
    _backward(dev, "backward_branches", case, ot, orr, ts, _egos(4), seed=2)


def test_backward_of_queries_that_share_entries_repeats_its_bits(dev):
    """all five queries of actor 0 lie between entries 2 and 4: the same cells are added to five times, in order"""
    case = tt.small_scene(6)
    ot, orr = tt.opt_arrays(case, 6)
    ts = [tt.BASE + STEP * q for q in (2.2, 2.4, 2.9, 3.1, 3.3)]
    m, first, (g_rot, g_trans) = _backward(dev, "backward_shared_entries", case, ot, orr, ts, _egos(5, 6), seed=3)
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        b, _ = _poses(m, dev, ts, _egos(5, 6))
        ((b.rot * torch.from_numpy(g_rot).to(dev)).sum() + (b.trans * torch.from_numpy(g_trans).to(dev)).sum()).backward()
        assert _bits(m.opt_trans.grad.cpu().numpy(), first["g_opt_trans"])
        assert _bits(m.opt_rots.grad.cpu().numpy(), first["g_opt_rots"])


def test_no_grad_is_the_forward_alone(dev):
    case, ot, orr, ts = _small(7)
    m = _actors(dev, case, ot, orr)
    with torch.no_grad():
        b, quiet = _poses(m, dev, ts, _egos(5, 7))
    assert not b.rot.requires_grad and b.rot.grad_fn is None
    _, loud = _poses(m, dev, ts, _egos(5, 7))
    assert _bits(quiet["rot"], loud["rot"]) and _bits(quiet["trans"], loud["trans"])


def test_refusals_on_the_device(dev):
    case, ot, orr, ts = _small(8)
    m = _actors(dev, case, ot, orr)
    ego = torch.from_numpy(tt.ego_pose(0)).to(dev)
    with pytest.raises(TypeError, match="ego_pose must be float32"):
        m.poses(ts[0], ego.double())
    with pytest.raises(TypeError, match="timestamps must be float64"):
        m.poses(torch.tensor(ts, device=dev).float(), ego)
    with pytest.raises(ValueError, match="ego poses for"):
        m.poses(ts, ego.expand(2, 4, 4))
    from gaussianrpg_amd.rasterizer import _C
    table = m.table.tensors(dev)
    tsd = torch.tensor(ts[:1], dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="come together"):
        _C.track_poses_forward(table, tsd, ego[None].contiguous(), m.opt_trans.detach(), None, None)
    short = list(table)
    short[7] = short[7].clone()
    short[7][1] = 1                                     # actor 0 with one entry, on the host copy the entry checks
    with pytest.raises(RuntimeError, match="fewer than two entries"):
        _C.track_poses_forward(short, tsd, ego[None].contiguous(), None, None, None)


# ---- the composed frame ----

def _frame(dev):
    """500 background + 2 x 100 actor Gaussians in front of a 64 x 48 camera; the actors' tracklets put them there"""
    from gaussianrpg_amd import harness as hz
    from gaussianrpg_amd.composed import ComposedRasterizer, ModelParams
    from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
    g = torch.Generator().manual_seed(11)

    def raw(sc):
        n = sc.means3D.shape[0]
        op = sc.opacity.clamp(1e-3, 1 - 1e-3)
        return ModelParams(*(t.to(dev).clone().requires_grad_(True) for t in (
            sc.means3D.contiguous(), torch.log(sc.scales), sc.rotations * (0.5 + torch.rand(n, 1, generator=g)),
            torch.log(op / (1 - op)), sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous())))
    models = [raw(hz.toy_scene(500, seed=3, sh_degree=1, depth=6.0))]
    for k in range(2):
        o = hz.toy_scene(100, seed=20 + k, sh_degree=1, depth=0.0, spread=0.35, scale=0.05)
        models.append(raw(hz.Scene(o.means3D, o.opacity.clamp(min=0.6), o.scales, o.rotations, o.shs, 1)))
    F, M = 4, 2
    tr = tt._empty(F, M)
    for f in range(F):
        for a, (x, z) in enumerate(((-1.2, 4.5), (1.1, 5.0))):
            tr[f, a] = np.concatenate([[a + 1], [x + 0.05 * f, 0.2 - 0.02 * f, z + 0.1 * f], tt.yaw_quat(0.2 * a + 0.05 * f)])
    stamps = tt.BASE + STEP * np.arange(F)
    case = tt.Case(tr, stamps, {a + 1: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1]) for a in range(2)})
    ego = np.eye(4, dtype=np.float32)
    ego[:3, 3] = [0.05, -0.03, 0.1]
    cam = hz.trajectory_camera(0, W=64, H=48, device=dev)
    rast = ComposedRasterizer(GaussianRasterizationSettings(
        **hz.settings_kwargs(cam, 1, bg=torch.tensor([0.2, 0.1, 0.3], device=dev))))
    ot, orr = tt.opt_arrays(case, 9)
    return rast, models, _actors(dev, case, ot * 0.2, orr), tt.BASE + 0.13, torch.from_numpy(ego).to(dev)


def test_composed_frame_from_pose_rows_equals_the_actor_pose_list(dev):
    from gaussianrpg_amd.composed import ActorPose
    rast, models, actors, t, ego = _frame(dev)
    with torch.no_grad():
        rows = actors.poses(t, ego).frame(0, [0, 1], [0.0, 0.0])
        a = rast.forward(models, rows)
        listed = [None] + [ActorPose(rows.rot[i], rows.trans[i], 0.0) for i in (1, 2)]
        b = rast.forward(models, listed)
        c = rast.forward(models, [None] + [ActorPose(rows.rot[i].tolist(), rows.trans[i].tolist(), 0.0) for i in (1, 2)])
    assert int((a[1] > 0).sum()) > 300 and int((a[1][500:] > 0).sum()) > 100     # the actors are in the picture
    for x, y, z in zip(a, b, c):
        assert _bits(x.cpu().numpy(), y.cpu().numpy()) and _bits(x.cpu().numpy(), z.cpu().numpy())


def test_composed_training_frame_reaches_opt_trans_and_opt_rots(dev):
    """the gradients at opt_trans / opt_rots equal the composed backward's pose gradients fed into the op's backward
    by hand"""
    from gaussianrpg_amd.rasterizer import _C
    rast, models, actors, t, ego = _frame(dev)
    batch = actors.poses(t, ego)
    rows = batch.frame(0, [0, 1], [0.0, 0.0])
    seen = {}
    rows.rot.register_hook(lambda g: seen.__setitem__("rot", g.clone()))
    rows.trans.register_hook(lambda g: seen.__setitem__("trans", g.clone()))
    color = rast.forward(models, rows)[0]
    w = torch.rand(color.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    (color * w).sum().backward()
    assert set(seen) == {"rot", "trans"} and float(seen["rot"][1:].abs().max()) > 0
    assert not seen["rot"][0].any() and not seen["trans"][0].any()                 # the background's row
    ts = torch.tensor([t], dtype=torch.float64, device=dev)
    g_ot, g_or = _C.track_poses_backward(actors.table.tensors(dev), ts, ego[None].contiguous(), actors.opt_trans.detach(),
                                         actors.opt_rots.detach(), None, seen["rot"][1:][None].contiguous(),
                                         seen["trans"][1:][None].contiguous())
    assert float(g_ot.abs().max()) > 0 and float(g_or.abs().max()) > 0
    assert _bits(actors.opt_trans.grad.cpu().numpy(), g_ot.cpu().numpy())
    assert _bits(actors.opt_rots.grad.cpu().numpy(), g_or.cpu().numpy())
    assert all(m.xyz.grad is not None for m in models)
