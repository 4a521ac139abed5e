"""CPU checks of the pose correction: the float64 truth (tests/pose_correction_truth.py) against float64 autograd
through the reference's lines, against the reference's recorded results (tests/golden/ref_pose_correction.*), against
the kernel's operation order restated in float32 numpy and against planted errors; the module's state dicts, the
checkpoint loader's handling of the ``pose_correction`` entry and the declared exports.  The kernels run in
tests/test_gpu_pose_correction.py."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import pose_correction_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden():
    with open(os.path.join(GOLDEN, "ref_pose_correction.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "ref_pose_correction.npz"))


def golden_params(kind, num=3):
    rows = [T.build_row(kind, seed=n) for n in range(num)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def golden_inputs(c):
    return (T.build_xyz(**c["xyz"]), T.build_rotation(**c["rotation"]), T.build_grad(**c["grad_xyz"]),
            T.build_grad(**c["grad_rotation"]))


def case(N, kind, seed=0):
    rot, trans = T.build_row(kind, seed)
    return dict(rot=rot, trans=trans, xyz=T.build_xyz(N, seed), rotation=T.build_rotation(N, seed + 1),
                gx=T.build_grad(N, 3, seed + 2), gr=T.build_grad(N, 4, seed + 3))


# ---------------------------------------------------------------------------------------------------------------
# the truth itself: float64 autograd through the reference's lines, restated in torch
# ---------------------------------------------------------------------------------------------------------------
def _reference64(rot, trans, xyz, rotation):
    q = torch.nn.functional.normalize(rot.unsqueeze(0), dim=-1)
    n = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    r, x, y, z = (q / n[:, None])[0]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).view(3, 3)
    M = torch.cat([torch.cat([R, trans[:, None]], -1), torch.tensor([[0, 0, 0, 1.0]], dtype=R.dtype)], 0)
    out_xyz = (torch.cat([xyz, torch.ones_like(xyz[:, :1])], -1) @ M.T)[:, :3]
    aw, ax, ay, az = q[0]
    bw, bx, by, bz = rotation.unbind(-1)
    out_rot = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                           aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)
    return out_xyz, out_rot


@pytest.mark.parametrize("kind", T.ROWS)
def test_truth_is_autograd_of_the_references_lines(kind):
    c = case(257, kind)
    t = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(k in ("rot", "trans", "xyz", "rotation"))
         for k, v in c.items()}
    ox, orot = _reference64(t["rot"], t["trans"], t["xyz"], t["rotation"])
    (ox * t["gx"]).sum().backward(retain_graph=True)
    f = T.forward64(c["rot"], c["trans"], c["xyz"], c["rotation"])
    np.testing.assert_allclose(f["xyz"], ox.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f["rotation"], orot.detach().numpy(), rtol=1e-12, atol=1e-12)
    b = T.backward64(c["rot"], c["xyz"], None, c["gx"], None)
    scale = np.abs(t["rot"].grad.numpy()).max()
    np.testing.assert_allclose(b["g_rot"], t["rot"].grad.numpy(), rtol=0, atol=1e-11 * scale)
    np.testing.assert_allclose(b["g_trans"], t["trans"].grad.numpy(), rtol=1e-12)
    np.testing.assert_allclose(b["g_xyz"], t["xyz"].grad.numpy(), rtol=1e-12, atol=1e-13)
    for k in ("rot", "trans", "xyz"):
        t[k].grad = None
    (orot * t["gr"]).sum().backward()
    b = T.backward64(c["rot"], None, c["rotation"], None, c["gr"])
    scale = np.abs(t["rot"].grad.numpy()).max()
    np.testing.assert_allclose(b["g_rot"], t["rot"].grad.numpy(), rtol=0, atol=1e-11 * scale)
    np.testing.assert_allclose(b["g_rotation"], t["rotation"].grad.numpy(), rtol=1e-12, atol=1e-13)
    assert not b["g_trans"].any()


# ---------------------------------------------------------------------------------------------------------------
# float32 in the kernel's order stays inside the derived bounds
# ---------------------------------------------------------------------------------------------------------------
def _ratios(c, parts="both", plant=None, plant_b=None):
    use_x, use_r = parts in ("both", "xyz"), parts in ("both", "rotation")
    xyz, rotation = (c["xyz"] if use_x else None), (c["rotation"] if use_r else None)
    gx, gr = (c["gx"] if use_x else None), (c["gr"] if use_r else None)
    f = T.forward64(c["rot"], c["trans"], xyz, rotation)
    b = T.backward64(c["rot"], xyz, rotation, gx, gr)
    ox, orot = T.forward32(c["rot"], c["trans"], xyz, rotation, plant=plant)
    k = T.backward32(c["rot"], xyz, rotation, gx, gr, plant=plant_b)
    out = {}
    if use_x:
        out["xyz"] = T.ratio(ox, f["xyz"], f["tol_xyz"])
        out["g_xyz"] = T.ratio(k["g_xyz"], b["g_xyz"], b["tol_g_xyz"])
        out["g_trans"] = T.ratio(k["g_trans"], b["g_trans"], b["tol_g_trans"])
    if use_r:
        out["rotation"] = T.ratio(orot, f["rotation"], f["tol_rotation"])
        out["g_rotation"] = T.ratio(k["g_rotation"], b["g_rotation"], b["tol_g_rotation"])
    out["g_rot"] = T.ratio(k["g_rot"], b["g_rot"], b["tol_g_rot"])
    return out


@pytest.mark.parametrize("kind", T.ROWS)
@pytest.mark.parametrize("N", [1, 63, 65, 257, 1500])
@pytest.mark.parametrize("parts", ["both", "xyz", "rotation"])
def test_restatement_meets_the_truth(N, kind, parts):
    r = _ratios(case(N, kind, seed=N), parts)
    assert max(r.values()) <= 1.0, r


def test_restatement_second_partial():
    """the finishing workgroup's loop takes a second partial: the sums' chain grows by one"""
    N = T.SIZES[-2]
    assert T.chain_depth(N) == 20 and T.chain_depth(N - 1) == 19
    r = _ratios(case(N, "wide", seed=5))
    assert max(r.values()) <= 1.0, r


def test_one_hot_sums_are_the_rows_own_numbers():
    c = case(600, "wide", seed=9)
    for row in (0, 255, 256, 599):
        gx, gr = np.zeros_like(c["gx"]), np.zeros_like(c["gr"])
        gx[row], gr[row] = c["gx"][row], c["gr"][row]
        k = T.backward32(c["rot"], c["xyz"], c["rotation"], gx, gr)
        assert np.array_equal(k["g_trans"], gx[row])
        assert not np.delete(k["g_xyz"], row, 0).any() and not np.delete(k["g_rotation"], row, 0).any()


# ---------------------------------------------------------------------------------------------------------------
# planted one-line errors are rejected by the same bounds
# ---------------------------------------------------------------------------------------------------------------
PLANTS = [
    # F.normalize dropped at norm 3.  (With it in place quaternion_to_matrix's second division moves values by
    # roundings only; the normalisation a row of norm 3 cannot do without is the one the product sees.)
    ("norm3", "no_normalize", None, "rotation"),
    ("wide", "normalized_product", None, "rotation"),        # compose_one's form: the product normalised behind it
    ("wide", None, "R_for_RT", "g_xyz"),
    ("norm3", None, "no_projection", "g_rot"),
    ("wide", None, "trans_from_rotation", "g_trans"),
]


@pytest.mark.parametrize("kind,plant,plant_b,field", PLANTS)
def test_planted_errors_are_rejected(kind, plant, plant_b, field):
    c = case(257, kind, seed=3)
    if plant == "normalized_product":     # a rotation that is not unit: the normalisation behind the product shows
        c["rotation"] = (c["rotation"] * np.float32(1.25)).astype(np.float32)
    clean = _ratios(c)
    assert max(clean.values()) <= 1.0, clean
    bad = _ratios(c, plant=plant, plant_b=plant_b)
    assert bad[field] > 1.0, bad
    assert all(v <= 1.0 for k, v in bad.items() if k != field), bad


# ---------------------------------------------------------------------------------------------------------------
# the reference's recorded results lie inside the bounds
# ---------------------------------------------------------------------------------------------------------------
def test_golden_inputs_are_the_recorded_ones():
    meta, _ = golden()
    assert len(meta["cases"]) == 8
    for c in meta["cases"]:
        rots, trans = golden_params(c["kind"], c["num_poses"])
        assert T.sha256(*golden_inputs(c), rots, trans) == c["sha256"], c["name"]


def test_goldens_meet_the_truth():
    meta, arr = golden()
    for c in meta["cases"]:
        rots, trans = golden_params(c["kind"], c["num_poses"])
        xyz, rotation, gx, gr = golden_inputs(c)
        rot, tr, n = rots[c["id"]], trans[c["id"]], c["name"]
        f = T.forward64(rot, tr, xyz, rotation)
        assert T.ratio(arr[n + "/xyz"], f["xyz"], f["tol_xyz"]) <= 1.0, n
        assert T.ratio(arr[n + "/rotation"], f["rotation"], f["tol_rotation"]) <= 1.0, n
        p = T.row64(rot)
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = p["R"], tr
        tol_M = np.zeros((4, 4))
        tol_M[:3, :3] = p["tol_R"]
        assert T.ratio(arr[n + "/matrix"], M, tol_M) <= 1.0, n
        # the reference sums over the rows in its matmul backward, in an order PyTorch leaves open: depth N - 1
        b = T.backward64(rot, xyz, None, gx, None, depth=c["N"] - 1)
        assert T.ratio(arr[n + "/grad_xyz"], b["g_xyz"], b["tol_g_xyz"]) <= 1.0, n
        others = np.delete(np.arange(c["num_poses"]), c["id"])
        for key in ("xyz_grad_rots", "xyz_grad_trans", "rotation_grad_rots"):
            assert not arr[n + "/" + key][others].any(), (n, key)
        assert T.ratio(arr[n + "/xyz_grad_trans"][c["id"]], b["g_trans"], b["tol_g_trans"]) <= 1.0, n
        assert T.ratio(arr[n + "/xyz_grad_rots"][c["id"]], b["g_rot"], b["tol_g_rot"]) <= 1.0, n
        b = T.backward64(rot, None, rotation, None, gr, depth=c["N"] - 1)
        assert T.ratio(arr[n + "/grad_rotation"], b["g_rotation"], b["tol_g_rotation"]) <= 1.0, n
        assert T.ratio(arr[n + "/rotation_grad_rots"][c["id"]], b["g_rot"], b["tol_g_rot"]) <= 1.0, n


# ---------------------------------------------------------------------------------------------------------------
# the module on the CPU: parameters, ids, state dicts, the PyTorch parts
# ---------------------------------------------------------------------------------------------------------------
def _camera(id=0, frame_idx=0):
    return types.SimpleNamespace(id=id, meta=dict(frame_idx=frame_idx))


def test_module_parameters_and_state_dict_round_trip():
    from gaussianrpg_amd.pose_correction import PoseCorrection
    with pytest.raises(ValueError, match="Invalid mode"):
        PoseCorrection(3, mode="sensor")
    for mode in ("image", "frame"):
        pc = PoseCorrection(3, mode=mode)
        assert [k for k, _ in pc.named_parameters()] == ["pose_correction_trans", "pose_correction_rots"]
        assert torch.equal(pc.pose_correction_trans, torch.zeros(3, 3))
        assert torch.equal(pc.pose_correction_rots, torch.tensor([[1.0, 0, 0, 0]]).repeat(3, 1))
        assert pc.get_id(_camera(id=2, frame_idx=1)) == (2 if mode == "image" else 1)
        assert torch.equal(pc(_camera()), torch.eye(4))
        rots, trans = golden_params("wide")
        sd = {"params": {"pose_correction_trans": torch.from_numpy(trans), "pose_correction_rots": torch.from_numpy(rots)}}
        pc.load_state_dict(sd)                                 # the reference's layout
        back = pc.save_state_dict(is_final=True)
        assert sorted(back) == ["params"] and sorted(back["params"]) == sorted(sd["params"])
        assert torch.equal(back["params"]["pose_correction_rots"], torch.from_numpy(rots))
        assert torch.equal(back["params"]["pose_correction_trans"], torch.from_numpy(trans))


def test_module_matrix_and_regulariser_meet_the_goldens():
    from gaussianrpg_amd.pose_correction import PoseCorrection
    meta, arr = golden()
    for c in meta["cases"]:
        rots, trans = golden_params(c["kind"], c["num_poses"])
        pc = PoseCorrection(c["num_poses"], mode=c["mode"])
        pc.load_state_dict({"params": {"pose_correction_trans": torch.from_numpy(trans),
                                       "pose_correction_rots": torch.from_numpy(rots)}})
        cam = _camera(c["camera_id"], c["camera_frame_idx"])
        assert pc.get_id(cam) == c["id"]
        n = c["name"]
        # the same float32 operations on the same CPU: the same bits
        assert np.array_equal(pc(cam).detach().numpy(), arr[n + "/matrix"]), n
        loss = pc.regularization_loss()
        loss.backward()
        assert np.array_equal(loss.detach().numpy().reshape(1), arr[n + "/reg_loss"]), n
        assert np.array_equal(pc.pose_correction_rots.grad.numpy(), arr[n + "/reg_grad_rots"]), n
        assert np.array_equal(pc.pose_correction_trans.grad.numpy(), arr[n + "/reg_grad_trans"]), n


def test_inactive_module_returns_its_input():
    from gaussianrpg_amd.pose_correction import PoseCorrection
    pc = PoseCorrection(2, active=False)
    xyz, rotation = torch.randn(5, 3), torch.randn(5, 4)
    assert pc.correct_gaussian_xyz(_camera(), xyz) is xyz
    assert pc.correct_gaussian_rotation(_camera(), rotation) is rotation
    assert pc.correct(_camera(), xyz, rotation) == (xyz, rotation)
    table, flags = pc.table(_camera(1))
    assert list(table.row) == [-1] and list(table.posed) == [False] and flags == [False]
    table, flags = PoseCorrection(2).table(_camera(1))
    assert list(table.row) == [1] and list(table.posed) == [True] and flags == [False]


def test_no_cpu_path():
    from gaussianrpg_amd.pose_correction import pose_correct
    with pytest.raises(RuntimeError, match="ROCm/HIP device"):
        pose_correct(torch.zeros(2, 3), None, torch.tensor([1.0, 0, 0, 0]), torch.zeros(3))


# ---------------------------------------------------------------------------------------------------------------
# the checkpoint loader keeps the entry
# ---------------------------------------------------------------------------------------------------------------
def _models():
    from gaussianrpg_amd.composed import ModelParams
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen)                                              # noqa: E731
    return {"background": ModelParams(r(7, 3), r(7, 3), r(7, 4), r(7, 1), r(7, 1, 3), r(7, 3, 3))}


def test_checkpoint_loader_keeps_the_pose_correction_entry(tmp_path):
    from gaussianrpg_amd import checkpoint as ck
    rots, trans = golden_params("near")
    sd = ck.state_dict_of(_models())
    plain = str(tmp_path / "plain.pth")
    torch.save(sd, plain)
    assert ck.load_checkpoint(plain).pose_correction is None
    assert ck.load_checkpoint(plain).pose_correction_module() is None
    sd["pose_correction"] = {"params": {"pose_correction_trans": torch.from_numpy(trans),
                                        "pose_correction_rots": torch.from_numpy(rots)}}
    path = str(tmp_path / "pc.pth")
    torch.save(sd, path)
    loaded = ck.load_checkpoint(path)
    assert loaded.names() == ["background"]                    # the entry is no model
    assert loaded.color_correction is None
    assert sorted(loaded.pose_correction) == ["pose_correction_rots", "pose_correction_trans"]
    for mode in ("image", "frame"):
        pc = loaded.pose_correction_module(mode=mode)
        assert pc.mode == mode and pc.active
        assert torch.equal(pc.pose_correction_rots, torch.from_numpy(rots))
        assert torch.equal(pc.pose_correction_trans, torch.from_numpy(trans))
    assert not loaded.pose_correction_module(active=False).active
    ply = str(tmp_path / "scene.ply")
    ck.write_ply(ply, _models())
    assert ck.load_checkpoint(ply).pose_correction is None
    # the existing positional arguments keep their places
    scene = ck.LoadedScene(loaded.models, "x", None)
    assert scene.color_correction is None and scene.pose_correction is None


# ---------------------------------------------------------------------------------------------------------------
# exports
# ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "grpg_rasterizer.h")) as f:
        header = f.read()
    for name in ("grpg_pose_correct_forward", "grpg_pose_correct_backward", "grpg_pose_correct_workspace_bytes",
                 "grpg_pose_rows_forward", "grpg_pose_rows_backward"):
        assert re.search(r"GRPG_API\s+\w+\s+%s\(" % name, header), name
    assert re.search(r"#define\s+GRPG_ABI_VERSION\s+7\b", header)
    from gaussianrpg_amd import build
    assert "-ffp-contract=off" in build.HIP_UNITS["pose_correction.hip"]
