"""CPU tests (-m "not gpu") of the tracklet -> actor-pose step (gaussianrpg_amd/tracks.py, csrc/tracks.hip): the static
table against ``torch.argwhere``, the host lookup of camera stamps, ``PoseRows`` through ``_pack`` against the
``ActorPose`` list, the state-dict keys, the exports, the refusals that fire before the device is needed, the
stand-in slerp against scipy, and the comparator of tests/test_gpu_tracks.py against planted errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tracks_truth as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
SYMBOLS = ("grpg_track_poses_forward", "grpg_track_poses_backward")


def _table(case):
    from gaussianrpg_amd.tracks import TrackTable
    return TrackTable.from_tracklets(case.tracklets, case.stamps, case.obj_info)


# ---- the static table ----

@pytest.mark.parametrize("builder,args", [("small_scene", {}), ("long_track", dict(L=130)), ("branch_scene", {}),
                                          ("same_side_scene", {})])
def test_entry_lists_equal_argwhere(builder, args):
    case = tt.build_case(builder, args)
    table = _table(case)
    ids = torch.from_numpy(case.tracklets).float()[..., 0]
    assert table.track_ids == list(case.obj_info.keys()) and table.shape == case.shape
    for a, track_id in enumerate(case.obj_info):
        want = torch.argwhere(ids == track_id).numpy()                      # actor_pose.py:30
        assert table.entry_list(a).dtype == np.int32 and np.array_equal(table.entry_list(a), want)
        assert table.start[a] == case.obj_info[track_id]['start_timestamp']
        assert table.end[a] == case.obj_info[track_id]['end_timestamp']
    assert table.stamps.dtype == np.float64 and np.array_equal(table.stamps, case.stamps)
    assert np.array_equal(table.input_trans, case.tracklets[..., 1:4].astype(np.float32))
    assert np.array_equal(table.input_rots, case.tracklets[..., 4:8].astype(np.float32))


def test_small_scene_holds_what_it_is_there_for():
    case = tt.small_scene()
    table = _table(case)
    ids = case.tracklets[..., 0]
    assert (ids == -1).sum() > 0 and (ids == 7).sum() == 2 and 7 not in case.obj_info      # padding; an unlisted id
    listed = {tuple(e) for a in range(3) for e in table.entry_list(a)}
    assert not any(ids[f, c] in (-1, 7) for f, c in listed) and len(listed) == len(table.entries) == 8 + 4 + 8
    assert sorted(set(table.entry_list(2)[:, 1])) == [1, 2] and sorted(set(table.entry_list(1)[:, 1])) == [1, 2]
    assert np.all(np.diff(table.entry_list(2)[:, 0]) > 0)                                   # row-major: by frame


def test_a_track_needs_two_entries():
    from gaussianrpg_amd.tracks import TrackTable
    case = tt.small_scene()
    info = dict(case.obj_info)
    info[99] = dict(start_timestamp=0.0, end_timestamp=1.0)                # absent from the tracklets
    with pytest.raises(ValueError, match="track 99 has 0 entries"):
        TrackTable.from_tracklets(case.tracklets, case.stamps, info)
    tr = case.tracklets.copy()
    tr[3:, :, 0][tr[3:, :, 0] == 5] = -1                                   # id 5 keeps one cell
    with pytest.raises(ValueError, match="track 5 has 1 entries"):
        TrackTable.from_tracklets(tr, case.stamps, case.obj_info)
    with pytest.raises(ValueError, match=r"tracklets must be \[F,M,8\]"):
        TrackTable.from_tracklets(tr[..., :7], case.stamps, case.obj_info)
    with pytest.raises(ValueError, match="must agree"):
        TrackTable.from_tracklets(tr, case.stamps[:-1], case.obj_info)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _table(case).tensors("cpu")


# ---- camera stamps of a validation frame ----

def test_closest_camera_timestamps():
    from gaussianrpg_amd.tracks import closest_camera_timestamps
    case = tt.small_scene()
    truth = tt.Truth(case, *tt.opt_arrays(case))
    n = 0
    for cam in case.camera_timestamps:
        for a, track_id in enumerate(case.obj_info):
            info = case.obj_info[track_id]
            for t in tt.BASE + 0.1 * np.array([0.2, 2.6, 3.37, 5.1, 7.0]):
                want = truth.camera_stamps(a, t, cam)
                got = closest_camera_timestamps(case.camera_timestamps[cam]['train_timestamps'],
                                                info['start_timestamp'], info['end_timestamp'], t)
                assert got == want
                n += want[0] is not None
    assert n == 15                                                         # camera 0 for all three actors; camera 1 never
    c1, c2 = closest_camera_timestamps([1.0, 2.0, 3.0, 10.0], 0.0, 5.0, 2.9)
    assert (c1, c2) == (3.0, 2.0)
    assert closest_camera_timestamps([1.0, 10.0], 0.0, 5.0, 2.0) == (None, None)


def test_val_stamps_array():
    from gaussianrpg_amd.tracks import TrackedActorPoses
    case = tt.small_scene()
    m = TrackedActorPoses(_table(case), camera_timestamps=case.camera_timestamps, device="cpu")
    ts = [tt.BASE + 0.26, tt.BASE + 0.51]
    assert m.val_stamps(ts, False, None) is None
    v = m.val_stamps(ts, [True, False], 0)
    assert v.shape == (2, 3, 2) and v.dtype == np.float64 and np.isnan(v[1]).all() and np.isfinite(v[0]).all()
    truth = tt.Truth(case, *tt.opt_arrays(case))
    for a in range(3):
        assert tuple(v[0, a]) == truth.camera_stamps(a, ts[0], 0)
    assert np.isnan(m.val_stamps(ts, True, 1)).all()                      # one stamp: the fallback everywhere
    with pytest.raises(ValueError, match="needs camera_timestamps and cam"):
        m.val_stamps(ts, True, None)
    off = TrackedActorPoses(_table(case), opt_track=False, camera_timestamps=case.camera_timestamps, device="cpu")
    assert off.val_stamps(ts, True, 0) is None                            # validation frames exist with opt_track only


# ---- the module ----

def test_state_dict_is_the_reference_s():
    from gaussianrpg_amd.tracks import TrackedActorPoses
    case = tt.small_scene()
    m = TrackedActorPoses(_table(case), device="cpu")
    sd = m.state_dict()
    assert list(sd) == ["opt_trans", "opt_rots"]                           # actor_pose.py:22-25: the only two
    assert tuple(sd["opt_trans"].shape) == (8, 3, 3) and tuple(sd["opt_rots"].shape) == (8, 3, 1)
    assert not sd["opt_trans"].any() and not sd["opt_rots"].any() and sd["opt_trans"].dtype == torch.float32
    assert m.opt_trans.requires_grad and m.opt_rots.requires_grad
    ref = {"params": {"opt_trans": torch.randn(8, 3, 3), "opt_rots": torch.randn(8, 3, 1)}}
    m.load_state_dict(ref["params"])                                       # strict
    assert torch.equal(m.opt_trans, ref["params"]["opt_trans"])
    assert list(TrackedActorPoses(_table(case), opt_track=False, device="cpu").state_dict()) == []


def test_poses_refuses_before_the_device_is_needed():
    from gaussianrpg_amd.tracks import TrackedActorPoses
    case = tt.small_scene()
    m = TrackedActorPoses(_table(case), device="cpu")
    ego = torch.eye(4)
    with pytest.raises(TypeError, match="ego_pose must be a tensor"):
        m.poses(tt.BASE, ego.numpy())
    with pytest.raises(TypeError, match="ego_pose must be float32"):
        m.poses(tt.BASE, ego.double())
    with pytest.raises(ValueError, match=r"ego_pose must be \[4,4\] or \[T,4,4\]"):
        m.poses(tt.BASE, ego[:3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.poses(tt.BASE, ego)                                              # everything right but the device


def test_binding_refusals():
    from gaussianrpg_amd.rasterizer import _C
    case = tt.small_scene()
    t = _table(case)
    table = [torch.from_numpy(x) for x in (t.stamps, t.input_trans, t.input_rots, t.entries, t.entry_offsets, t.start,
                                           t.end, t.entry_offsets)]
    ts, ego = torch.tensor([tt.BASE], dtype=torch.float64), torch.eye(4)[None].contiguous()
    ot, orr = torch.zeros(8, 3, 3), torch.zeros(8, 3, 1)
    with pytest.raises(RuntimeError, match="timestamps must be a contiguous float64"):
        _C.track_poses_forward(table, ts.float(), ego)
    with pytest.raises(RuntimeError, match="stamps must be a contiguous float64"):
        _C.track_poses_forward([table[0].float()] + table[1:], ts, ego)
    with pytest.raises(RuntimeError, match="the table is"):
        _C.track_poses_forward(table[:7], ts, ego)
    with pytest.raises(RuntimeError, match=r"ego must be a contiguous float32 \[T,4,4\]"):
        _C.track_poses_forward(table, ts, ego[0])
    with pytest.raises(RuntimeError, match="come together or not at all"):
        _C.track_poses_forward(table, ts, ego, ot, None)
    with pytest.raises(RuntimeError, match="val_stamps needs opt_trans"):
        _C.track_poses_forward(table, ts, ego, None, None, torch.zeros(1, 3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"opt_rots must be a contiguous float32 \[F,M,1\]"):
        _C.track_poses_forward(table, ts, ego, ot, torch.zeros(8, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.track_poses_forward(table, ts, ego, ot, orr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.track_poses_backward(table, ts, ego, ot, orr, None, torch.zeros(1, 3, 4), torch.zeros(1, 3, 3))


# ---- PoseRows through _pack ----

def test_pose_rows_pack_to_the_bytes_of_the_actor_pose_list():
    from gaussianrpg_amd.composed import ActorPose, ModelParams, PoseRows, _pack, _posed_flags
    rng = np.random.RandomState(4)
    dims = [1, 3, 1, 2]
    models = [ModelParams(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 1),
                          torch.zeros(5, d, 3), torch.zeros(5, 3, 3)) for d in dims]
    rot = torch.from_numpy(rng.normal(0, 1, (4, 4)).astype(np.float32))
    trans = torch.from_numpy(rng.normal(0, 30, (4, 3)).astype(np.float32))
    rot[2] = -3.0                                            # a static model's row is ignored, whatever it holds
    posed, times = [False, True, False, True], [0.7, 0.25, 0.1, 0.9]
    rows = PoseRows(rot, trans, posed, times)
    for form in ("tensors", "floats"):
        val = (lambda v: v) if form == "tensors" else (lambda v: v.tolist())
        listed = [ActorPose(val(rot[i]), val(trans[i]), times[i]) if posed[i] else None for i in range(4)]
        _, pose_a, idft_a = _pack(models, rows)
        _, pose_b, idft_b = _pack(models, listed)
        assert pose_a.dtype == pose_b.dtype == torch.float32 and pose_a.shape == pose_b.shape == (4, 8)
        assert pose_a.numpy().tobytes() == pose_b.numpy().tobytes()
        assert idft_a.numpy().tobytes() == idft_b.numpy().tobytes()
    assert _posed_flags(rows) == posed == _posed_flags(listed)
    with pytest.raises(ValueError, match="one pose row, posed flag and fourier_time per model"):
        _pack(models[:3], rows)
    with pytest.raises(ValueError, match="pose rows must be rot"):
        _pack(models, PoseRows(rot[:3], trans, posed, times))


def test_pose_batch_frame_builds_the_row_set():
    from gaussianrpg_amd.tracks import PoseBatch
    rot = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4).requires_grad_(True)
    trans = torch.arange(2 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3)
    rows = PoseBatch(rot, trans, torch.ones(2, 3, dtype=torch.uint8)).frame(1, [2, 0], [0.5, 0.25])
    assert rows.posed == [False, True, True] and rows.fourier_time == [0.0, 0.5, 0.25]
    assert torch.equal(rows.rot[1:], rot[1, [2, 0]]) and torch.equal(rows.trans[1:], trans[1, [2, 0]])
    assert not rows.rot[0].any() and rows.rot.requires_grad                      # the rows keep their graph
    with pytest.raises(ValueError, match="one fourier_time per actor"):
        PoseBatch(rot, trans, None).frame(0, [0, 1], [0.0])


# ---- the exports ----

def test_symbols_are_declared_and_exported_and_the_abi_version_stays():
    import torch  # noqa: F401  (loads the libamdhip64 the library links)
    with open(HEADER) as f:
        header = f.read()
    lib = ctypes.CDLL(LIB)
    for s in SYMBOLS:
        assert re.search(r"GRPG_API int %s\(" % s, header), s
        assert hasattr(lib, s), s
    assert "typedef struct grpg_track_table" in header
    assert re.search(r"#define GRPG_ABI_VERSION 7\b", header)
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7
    from gaussianrpg_amd import build
    assert "tracks.hip" in build.HIP_UNITS and "-ffp-contract=off" in build.HIP_UNITS["tracks.hip"]


def test_device_entries_fail_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib = ctypes.CDLL(LIB)
    lib.grpg_last_error.restype = ctypes.c_char_p
    for s, n in zip(SYMBOLS, (12, 12)):
        fn = getattr(lib, s)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * (n - 2)
        assert fn(None, 1, *([None] * (n - 2))) == -2
        assert b"no usable HIP device" in lib.grpg_last_error()


# ---- the stand-in slerp ----

def test_stand_in_slerp_is_the_shortest_arc_geodesic():
    """as rotations (sign-free) against scipy's Slerp for s in [0, 1]; q0 at W = 0; the series meets the closed form
    at the switch; extrapolation continues the same great circle"""
    R = pytest.importorskip("scipy.spatial.transform")
    rng = np.random.RandomState(8)
    worst = 0.0
    for _ in range(200):
        q = rng.normal(0, 1, (2, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        if rng.rand() < 0.3:
            q[1] = tt._qmul_np(q[0], tt.yaw_quat(rng.uniform(-0.02, 0.02)))        # nearby: the series and its surroundings
        s = rng.uniform(0, 1)
        got = tt.unitquat_slerp(torch.from_numpy(q[:1]), torch.from_numpy(q[1:]), torch.tensor([s], dtype=torch.float64))
        got = got[0, 0].numpy()
        ref = R.Slerp([0.0, 1.0], R.Rotation.from_quat(q))([s]).as_quat()[0]
        worst = max(worst, min(np.abs(got - ref).max(), np.abs(got + ref).max()))
    assert worst < 1e-11, worst
    q0 = torch.from_numpy(q[:1])
    for s in (-0.5, 0.0, 0.3, 1.0, 1.7):
        same = tt.unitquat_slerp(q0, q0.clone(), torch.tensor([s], dtype=torch.float64))[0]
        assert torch.isfinite(same).all() and (same - q0).abs().max() < 1e-15
    # s outside [0, 1]: slerp(q0, q1, 2) is q1 turned once more by the same rotation
    a, b = q[0], tt._qmul_np(q[0], tt.yaw_quat(0.4))
    twice = tt.unitquat_slerp(torch.from_numpy(a[None]), torch.from_numpy(b[None]), torch.tensor([2.0], dtype=torch.float64))
    assert np.abs(twice[0, 0].numpy() - tt._qmul_np(a, tt.yaw_quat(0.8))).max() < 1e-14


# ---- the comparator rejects planted errors ----

def _batches(case, ot, orr, ts, egos, variant, is_val=False, cam=None):
    return (tt.Truth(case, ot, orr, torch.float32, variant).batch(ts, egos, is_val, cam),
            tt.Truth(case, ot, orr, torch.float32).batch(ts, egos, is_val, cam),
            tt.Truth(case, ot, orr, torch.float64).batch(ts, egos, is_val, cam))


@pytest.mark.parametrize("variant", tt.VARIANTS)
def test_comparator_rejects(variant):
    if variant == "bracket":
        case, ts = tt.same_side_scene(), [tt.BASE + 0.45]
    else:
        case = tt.small_scene()
        ts = [tt.BASE + 0.1 * q for q in (0.33, 2.511, 4.4, 5.62, 6.8)]
    ot, orr = tt.opt_arrays(case)
    egos = [tt.ego_pose(k % 4) for k in range(len(ts))]
    with np.errstate(all="ignore"):                                       # stamps32: every stamp is the same float32
        got, f32, f64 = _batches(case, ot, orr, ts, egos, variant)
    tt.compare(f32, f32, f64, name="restatement")                         # the yardstick passes its own bar
    with pytest.raises(AssertionError, match=variant):
        tt.compare(got, f32, f64, name=variant)


@pytest.mark.parametrize("variant", ["half_angle", "weights_swapped", "no_sign"])
def test_comparator_rejects_wrong_gradients(variant):
    case = tt.small_scene()
    ts = [tt.BASE + 0.1 * q for q in (0.33, 2.511, 4.4, 5.62, 6.8)]
    ot, orr = tt.opt_arrays(case)
    egos = [tt.ego_pose(k % 4) for k in range(5)]
    rng = np.random.RandomState(1)
    g_rot, g_trans = rng.normal(0, 1, (5, 3, 4)).astype(np.float32), rng.normal(0, 1, (5, 3, 3)).astype(np.float32)
    names = ("g_opt_trans", "g_opt_rots")
    grads = []
    for dtype, v in ((torch.float32, variant), (torch.float32, None), (torch.float64, None)):
        th = tt.Truth(case, ot, orr, dtype, v)
        grads.append(dict(zip(names, th.gradients(th.batch(ts, egos), g_rot, g_trans))))
    tt.compare(grads[1], grads[1], grads[2], groups=names, name="restatement")
    with pytest.raises(AssertionError, match=variant):
        tt.compare(grads[0], grads[1], grads[2], groups=names, name=variant)
    # a gradient that is not dense fails too: one untouched cell off zero
    bad = {k: v.copy() for k, v in grads[1].items()}
    assert case.tracklets[0, 2, 0] == -1 and not bad["g_opt_trans"][0, 2].any()          # a padded cell
    bad["g_opt_trans"][0, 2, 0] = 1e-3
    with pytest.raises(AssertionError, match="dense"):
        tt.compare(bad, grads[1], grads[2], groups=names, name="dense")
