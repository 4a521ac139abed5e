"""CPU tests of the closed loop's tail (gaussianrpg_amd/closed_loop.py, csrc/ego_loop.hip): the numpy restatement
tests/loop_truth.py against what the reference's own lines gave (tests/golden/ref_ego_loop.npz, bit for bit), the camera
row's arithmetic against the host route's, planted errors, and the host half of the module.  No device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import loop_truth as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_ego_loop")
REF_COLUMNS = 13        # the columns of a log row the reference's objects hold


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    return meta, dict(np.load(GOLDEN + ".npz"))


@pytest.fixture(scope="module")
def C():
    return lt.Constants()


def _ranging_bytes(C, plant=()):
    out = {}
    for name, images in lt.ranging_cases().items():
        for b, rows in enumerate(images):
            out["ranging/%s/%d" % (name, b)] = lt.object_positions(rows, C, plant=plant)[0]
    return out


def _scenario_rows(plant=()):
    return {"scenario/%s" % s: lt.run_scenario(s, plant=plant)[0][:, :REF_COLUMNS] for s in lt.SCENARIOS}


def _equal_bits(got, want):
    return {k for k in got if got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()}


# ---- the restatement is the reference ----

def test_golden_file_says_what_was_executed(golden):
    meta, arrays = golden
    src = meta["source"]
    assert "ast" in src and "Stand-ins replace only the ROS message and node classes" in src
    for piece in ("simulator.py methods lines", "simulator.py next_frame lines", "simulator.py render lines",
                  "AEB_controller.py methods lines"):
        assert piece in src
    assert sorted(arrays) == sorted(list(_ranging_bytes(lt.Constants())) + ["scenario/%s" % s for s in lt.SCENARIOS])
    by_name = {s["name"]: s for s in meta["scenarios"]}
    assert by_name["brake"]["first_activated"] == 4 and by_name["brake"]["final_velocity"] == 0.0
    assert by_name["cruise"]["first_activated"] is None and by_name["cruise"]["final_idx"] == 13.0


def test_ranging_equals_the_reference_bit_for_bit(golden, C):
    _, arrays = golden
    got = _ranging_bytes(C)
    assert _equal_bits(got, arrays) == set()
    assert sum(len(v) for v in got.values()) > 90
    assert len(got["ranging/filtered_10/0"]) == 0 and len(got["ranging/below_above_10/0"]) == 3
    on = got["ranging/horizon_10/0"]
    assert on.shape == (3, 2) and not np.isfinite(on[1]).any() and np.isfinite(on[[0, 2]]).all()     # kept, non-finite


def test_scenarios_equal_the_reference_bit_for_bit(golden):
    _, arrays = golden
    got = _scenario_rows()
    assert _equal_bits(got, arrays) == set()
    brake = got["scenario/brake"]
    assert brake[:, 8].tolist() == [0.0] * 4 + [1.0] * 8                     # the brake latches at step 4
    assert brake[:, 3].tolist() == [0.0] * 4 + [-8.0] * 4 + [0.0] * 4        # and stays when the command goes back to 0
    assert brake[7, 4] > 0 and (brake[8:, 4] == 0).all() and brake[2, 2] == brake[1, 2]     # clamped at 0; CIPV persists
    fast = got["scenario/fast"]
    assert fast[4, 3] == -13.5 and fast[5, 3] == -10.0 and fast[4, 4] > 1.9 and fast[5, 4] == 0.0     # the zero-vector norm


@pytest.mark.parametrize("plant", ["v_minus_h", "no_reversed", "sign_c1", "release_on_zero", "cipv_reset", "no_clamp",
                                   "idx_unclamped"])
def test_planted_errors_are_rejected(golden, C, plant):
    _, arrays = golden
    got = dict(_ranging_bytes(C, (plant,)))
    got.update(_scenario_rows((plant,)))
    wrong = _equal_bits(got, arrays)
    assert wrong, "the recorded results do not tell %s from the restatement" % plant
    ranging_error = plant in ("v_minus_h", "no_reversed", "sign_c1")
    assert any(k.startswith("ranging/") for k in wrong) == ranging_error
    if not ranging_error:
        assert all(k.startswith("scenario/") for k in wrong)


def test_the_cases_keep_their_margins(C):
    """no comparison of a case lies near its edge: another atan / sin / cos cannot flip it"""
    for name, images in lt.ranging_cases().items():
        for rows in images:
            for row in rows:
                r = lt.range_row(row, C, lt.LD)
                if r is None or not np.isfinite(np.asarray(r[2], dtype=np.float64)).all():
                    continue
                assert abs(float(r[2][0])) > 1e-3, name            # the d[0] <= 0 rule
    for s in ("brake", "fast", "cruise"):
        sc = lt.scenario(s)
        loop = lt.Loop(sc["tape"], C, dtype=lt.LD, **sc["kw"])
        for dets in sc["steps"]:
            for rows in dets:
                for p in lt.object_positions(rows, C, lt.LD)[0]:
                    assert abs(abs(float(p[1])) - 1.2) > 1e-3 and float(p[0]) > 1e-3
            loop.step(dets)
            m = loop.margins()
            assert m["brake"] > 1e-3 and m["ladder"] > 2e-4, (s, m)


# ---- the camera row ----

def _poses():
    out = []
    for s in ("brake", "fast", "commanded"):
        out += lt.run_scenario(s)[1]
    rs = np.random.RandomState(5)
    for _ in range(40):
        a = rs.uniform(-0.4, 0.4, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        out.append((Rx @ Ry @ Rz, rs.uniform(-30, 30, 3)))
    return out


def test_camera_row_against_the_host_route():
    from gaussianrpg_amd import harness as hz
    from gaussianrpg_amd.session import _camera_row, camera_from_pose, default_K
    Wf, Hf = lt.W, lt.H
    s = Wf / hz.WAYMO_W
    proj_t = hz.projection_from_K(hz.WAYMO_FX * s, hz.WAYMO_FY * s, Wf / 2.0, Hf / 2.0, Hf, Wf).transpose(0, 1).contiguous().numpy()
    k_inv = np.linalg.inv(default_K(Wf, Hf))
    err_ours, err_host = {"proj": 0.0, "centre": 0.0}, {"proj": 0.0, "centre": 0.0}
    for R, T in _poses():
        ours = lt.camera_row(R, T, proj_t, k_inv)
        host = _camera_row(camera_from_pose(R, T, Wf, Hf), k_inv)
        assert ours[0:16].tobytes() == host[0:16].tobytes()                     # the view matrix
        assert ours[36:48].tobytes() == host[36:48].tobytes()                   # the ray matrix and its spare floats
        assert ours[35] == 0 and host[35] == 0
        _, full, centre, _ = lt.camera_parts(R, T, proj_t, k_inv, dtype=lt.LD)
        for key, sl, truth in (("proj", slice(16, 32), full.reshape(-1)), ("centre", slice(32, 35), centre)):
            err_ours[key] = max(err_ours[key], float(np.abs(ours[sl].astype(lt.LD) - truth).max()))
            err_host[key] = max(err_host[key], float(np.abs(host[sl].astype(lt.LD) - truth).max()))
    print("camera row, distance from the longdouble truth: ours %r, the host route %r" % (err_ours, err_host))
    assert err_ours["proj"] <= err_host["proj"] and err_ours["centre"] <= err_host["centre"]
    assert err_host["centre"] > 0


# ---- the module's host half ----

def test_ranging_constants_and_class_mask():
    from gaussianrpg_amd import closed_loop as cl
    C = lt.Constants()
    r = cl.Ranging(C.K, C.extrinsics, C.cam_height, C.H, C.W, names=lt.NAMES)
    assert r.class_ids == [0, 1, 2, 3, 5, 7, 9, 11] and r.nc == 12
    H_, W_, nc, lo, hi, params = r.args()
    assert (H_, W_, nc, lo, hi) == (96, 160, 12, sum(1 << c for c in r.class_ids), 0)
    assert params[0] == C.K[1, 1] and params[1] == 1.5
    assert np.array(params[2:11]).tobytes() == C.k_inv.tobytes() and np.array(params[11:]).tobytes() == C.p_inv.tobytes()
    big = cl.Ranging(C.K, C.extrinsics, 1.5, 96, 160, names={100: "car", 127: "bus"})
    assert big.args()[3:5] == (0, (1 << 36) | (1 << 63)) and big.nc == 128
    assert cl.Ranging(C.K, C.extrinsics, 1.5, 96, 160).class_ids == list(range(128))          # no names: no filter
    assert cl.Ranging(C.K, C.extrinsics, 1.5, 96, 160, keep=[2, 7]).class_ids == [2, 7]
    with pytest.raises(ValueError, match="at most 128 classes"):
        cl.Ranging(C.K, C.extrinsics, 1.5, 96, 160, names=["c%d" % i for i in range(129)])
    sim = cl.Ranging.for_simulator(np.array([[1, 0, 0, 1.544], [0, 1, 0, 0.0], [0, 0, 1, 2.1], [0, 0, 0, 1.0]]), 1600, 1066)
    assert sim.cam_height == 2.1 and sim.extrinsics[2, 3] == -1.544 and sim.K[1, 2] == 533 and (sim.W, sim.H) == (1600, 1066)


def test_refusals_on_the_host():
    from gaussianrpg_amd import closed_loop as cl
    C = lt.Constants()
    r = cl.Ranging(C.K, C.extrinsics, 1.5, 96, 160, names=lt.NAMES)
    with pytest.raises(ValueError, match=r"max_det must lie in \[1, 64\]"):
        cl.object_positions(torch.zeros(1, 65, 6), torch.zeros(1, dtype=torch.int32), r)
    with pytest.raises(ValueError, match="no CPU path"):
        cl.object_positions(torch.zeros(1, 10, 6), torch.zeros(1, dtype=torch.int32), r)
    with pytest.raises(ValueError, match="float32"):
        cl.object_positions(torch.zeros(1, 10, 6, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), r)
    with pytest.raises(ValueError, match="CameraRow"):
        from gaussianrpg_amd.session import CameraRow
        CameraRow(torch.zeros(48))


def test_host_loop_is_the_restatement(C):
    """closed_loop.HostLoop (the reference's numpy calls as they stand, BLAS included) against loop_truth: the same
    decisions, values to 1e-12 relative"""
    from gaussianrpg_amd import closed_loop as cl
    r = cl.Ranging(C.K, C.extrinsics, C.cam_height, C.H, C.W, names=lt.NAMES)
    for s in lt.SCENARIOS:
        sc = lt.scenario(s)
        host = cl.HostLoop(sc["tape"], r, **sc["kw"])
        for i, dets in enumerate(sc["steps"]):
            host.step(dets, None if sc["commands"] is None else sc["commands"][i])
        want = lt.run_scenario(s)[0]
        got = host.log()
        assert got.shape == want.shape == (12, 16)
        assert np.array_equal(got[:, [1, 3, 8, 11, 13, 14]], want[:, [1, 3, 8, 11, 13, 14]]), s
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)


def test_exports_build_flags_and_binding():
    text = open(HEADER).read()
    declared = set(re.findall(r"GRPG_API\s+[\w\s\*]+?\b(grpg_\w+)\s*\(", text))
    assert {"grpg_object_positions", "grpg_ego_loop_step"} <= declared
    assert re.search(r"#define\s+GRPG_ABI_VERSION\s+7\b", text)
    from gaussianrpg_amd import build
    assert "-ffp-contract=off" in build.HIP_UNITS["ego_loop.hip"]
    if not os.path.exists(LIB):
        build.build_native()
    lib = ctypes.CDLL(LIB)
    for name in ("grpg_object_positions", "grpg_ego_loop_step"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        assert fn(None) == (-1 if torch.cuda.is_available() else -2)      # refused, or no device: nothing enqueued
    from gaussianrpg_amd.rasterizer import _C
    assert hasattr(_C, "object_positions") and hasattr(_C, "ego_loop_step")
