"""Generate tests/golden/ref_tracks.json + ref_tracks.npz.  Needs a checkout of the reference (GaussianRPG); never run
by a test:

    python tests/golden/make_golden_tracks.py <path to the reference>

Cuts ``find_closest_indices``, ``find_closest_camera_timestamps`` and the four ``get_tracking_*`` methods out of the
reference's lib/models/actor_pose.py, and ``quaternion_raw_multiply``, ``matrix_to_quaternion``,
``_sqrt_positive_part`` and ``quaternion_slerp`` out of its lib/utils/general_utils.py, with ``ast`` (the modules
themselves import roma, the config and the CUDA extensions, which are not installed here) and executes them on CPU
tensors over a stub object that holds what ``ActorPose.__init__`` sets up (actor_pose.py:13-30, built here with the
reference's own expressions).  The ego product of ``parse_camera`` (street_gaussian_model.py:272-274) sits inside a
long method and is applied here with the reference's functions, in its three lines.

``roma.utils.unitquat_slerp`` is a stand-in, ``unitquat_slerp`` of tests/tracks_truth.py, which implements the formula
of DESIGN.md section 21 -- THE ONE STEP NOT EXECUTED FROM THE REFERENCE: roma is not installed, and its float32 bits
are not pinned by this fixture.  The generator checks the stand-in against ``scipy.spatial.transform.Slerp`` as
rotations (sign-free) for s in [0, 1] where scipy imports.

The files hold numbers only.  Inputs are not stored: a case names its builder in tests/tracks_truth.py and the
builder's arguments (legacy numpy RandomState: stable) and records the sha256 of the input's bytes, the query stamps,
the ego poses' builder arguments, and per (query, actor) what the reference returned: get_tracking_rotation,
get_tracking_translation, and the world pose after the ego product.
"""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tracks_truth as tt   # noqa: E402  (the input builders and the stand-in slerp)

METHODS = ["find_closest_indices", "find_closest_camera_timestamps", "get_tracking_translation_",
           "get_tracking_translation", "get_tracking_rotation_", "get_tracking_rotation"]
FUNCTIONS = ["quaternion_raw_multiply", "matrix_to_quaternion", "_sqrt_positive_part", "quaternion_slerp"]


class _RomaUtils:
    unitquat_slerp = staticmethod(tt.unitquat_slerp)


class _Roma:
    utils = _RomaUtils


def _reference(ref):
    ns = {"torch": torch, "np": np, "F": torch.nn.functional, "roma": _Roma, "Camera": object}
    path = os.path.join(ref, "lib", "utils", "general_utils.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS]
    assert sorted(n.name for n in fns) == sorted(FUNCTIONS)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    path = os.path.join(ref, "lib", "models", "actor_pose.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ActorPose"][0]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in methods) == sorted(METHODS)
    stub = ast.ClassDef(name="ActorPoseMethods", bases=[], keywords=[], body=methods, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[stub], type_ignores=[])), path, "exec"), ns)
    return ns


class _Camera:
    def __init__(self, timestamp, cam, is_val):
        self.meta = dict(timestamp=timestamp, cam=cam, is_val=is_val)


def _actor_pose(ns, case, opt):
    """what ActorPose.__init__ leaves on self (actor_pose.py:13-30), on the CPU"""
    o = ns["ActorPoseMethods"]()
    tracklets = torch.from_numpy(case.tracklets).float()
    o.track_ids = tracklets[..., 0]
    o.input_trans = tracklets[..., 1:4]
    o.input_rots = tracklets[..., 4:8]
    o.timestamps = case.stamps
    o.camera_timestamps = case.camera_timestamps
    o.opt_track = opt is not None
    if o.opt_track:
        o.opt_trans = torch.from_numpy(opt[0].copy())
        o.opt_rots = torch.from_numpy(opt[1].copy())
    o.obj_info = {k: dict(v) for k, v in case.obj_info.items()}
    for track_id in o.obj_info.keys():
        o.obj_info[track_id]['track_idx'] = torch.argwhere(o.track_ids == track_id)
    return o


def _cases():
    q = [0.33, 2.511, 4.4, 5.62, 6.8]
    small = ("small_scene", dict(seed=0))
    return [
        ("plain", *small, 0, q, False, None, ""),
        ("validation_camera_stamps", *small, 0, q, True, 0, "every actor's span holds two of camera 0's stamps"),
        ("validation_fallback", *small, 0, q, True, 1, "camera 1 has one stamp: fewer than two inside any track"),
        ("opt_track_off", *small, None, q, False, None, ""),
        ("opt_track_off_is_val", *small, None, q, True, 0, "is_val without opt_track is the plain path"),
        ("branches", "branch_scene", dict(seed=3), None, [1.2, 1.45, 1.7, 1.93], False, None,
         "W = 0, q0 . q1 < 0, W near pi / 2, raw angle near pi"),
        ("branches_opt", "branch_scene", dict(seed=3), 2, [1.2, 1.45, 1.7, 1.93], False, None, ""),
        ("same_side", "same_side_scene", {}, 1, [4.5], False, None, "both closest entries before the query"),
        ("long_track_65", "long_track", dict(L=65), 3, [0.3, 63.4, 63.7], False, None, ""),
    ]


def _check_standin():
    try:
        from scipy.spatial.transform import Rotation, Slerp
    except ImportError:
        return None
    rng = np.random.RandomState(8)
    worst = 0.0
    for _ in range(500):
        q = rng.normal(0, 1, (2, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        s = rng.uniform(0, 1)
        got = tt.unitquat_slerp(torch.from_numpy(q[:1]), torch.from_numpy(q[1:]), torch.tensor([s], dtype=torch.float64))
        ref = Slerp([0.0, 1.0], Rotation.from_quat(q))([s]).as_quat()[0]
        worst = max(worst, min(np.abs(got[0, 0].numpy() - ref).max(), np.abs(got[0, 0].numpy() + ref).max()))
    assert worst < 1e-11, worst
    return worst


def main(ref):
    ns = _reference(ref)
    arrays, rows = {}, []
    for name, builder, args, opt_seed, queries, is_val, cam, note in _cases():
        case = tt.build_case(builder, args)
        opt = None if opt_seed is None else tt.opt_arrays(case, opt_seed)
        pose = _actor_pose(ns, case, opt)
        ts = [tt.BASE + 0.1 * q for q in queries]
        egos = [tt.ego_pose(k % 4) for k in range(len(ts))]
        out = {k: [] for k in ("rot", "trans", "obj_rot", "obj_trans")}
        active = []
        for t, ego in zip(ts, egos):
            camera = _Camera(t, cam, is_val)
            ego_pose = torch.from_numpy(ego)
            for track_id, info in case.obj_info.items():
                on = info['start_timestamp'] <= t <= info['end_timestamp']      # street_gaussian_model.py:244
                active.append(int(on))
                if not on:
                    continue
                obj_rot = pose.get_tracking_rotation(track_id, camera)
                obj_trans = pose.get_tracking_translation(track_id, camera)
                out["rot"].append(obj_rot.numpy().copy())
                out["trans"].append(obj_trans.numpy().copy())
                ego_pose_rot = ns["matrix_to_quaternion"](ego_pose[:3, :3].unsqueeze(0)).squeeze(0)
                obj_rot = ns["quaternion_raw_multiply"](ego_pose_rot.unsqueeze(0), obj_rot.unsqueeze(0)).squeeze(0)
                obj_trans = ego_pose[:3, :3] @ obj_trans + ego_pose[:3, 3]
                out["obj_rot"].append(obj_rot.numpy().copy())
                out["obj_trans"].append(obj_trans.numpy().copy())
        for k, v in out.items():
            a = np.stack(v)
            assert a.dtype == np.float32 and np.all(np.isfinite(a)), (name, k)
            arrays["%s/%s" % (name, k)] = a
        rows.append(dict(name=name, builder=builder, args=args, opt_seed=opt_seed, queries=queries, is_val=is_val, cam=cam,
                         note=note, active=active, sha256=case.sha256()))
        print("%-28s %s actors x %d queries -> %d poses" % (name, case.shape[2], len(ts), len(out["rot"])))
    worst = _check_standin()
    source = ("lib/models/actor_pose.py (%s) and lib/utils/general_utils.py (%s) of the reference, cut with ast and "
              "executed on CPU torch %s; roma.utils.unitquat_slerp is a stand-in (tests/tracks_truth.py unitquat_slerp, "
              "DESIGN.md section 21), the one step not executed from the reference; stand-in against "
              "scipy.spatial.transform.Slerp as rotations: %s" % (
                  ", ".join(METHODS), ", ".join(FUNCTIONS), torch.__version__.split("+")[0],
                  "not checked (scipy not installed where this was generated)" if worst is None
                  else "largest difference %.1e over 500 random pairs, s in [0, 1]" % worst))
    with open(os.path.join(HERE, "ref_tracks.json"), "w") as f:
        json.dump({"source": source, "cases": rows}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_tracks.npz"), **arrays)
    print("wrote %d cases, %d arrays" % (len(rows), len(arrays)))


if __name__ == "__main__":
    main(sys.argv[1])
