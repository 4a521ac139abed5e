"""CPU checks of the use_mlp colour correction: the float64 truth and its bounds (tests/color_mlp_truth.py) against the
reference's recorded results (tests/golden/ref_color_mlp.*), against the kernel's operation order restated in float32
numpy and against planted errors; the condition every gradient case must meet; the module's state dicts, the
checkpoint loader and the declared exports.  The kernels run in tests/test_gpu_color_mlp.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import color_mlp_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden():
    with open(os.path.join(GOLDEN, "ref_color_mlp.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "ref_color_mlp.npz"))


def ref_distance(pose):
    """The reference's own recorded float32 distance of the 6-vector from the truth."""
    _, arrays = golden()
    return float(np.abs(arrays[pose + "/x"].astype(np.float64) - T.truth(pose)["fws"][0]["x"]).max())


def restated(batch, zero_last=False, **planted):
    """The float32 restatement of a whole batch: dict(x, A, hidden, reg, grads)."""
    t = T.truth(batch, zero_last=zero_last)
    pose_kw = {k: planted.pop(k) for k in ("standardise", "last_on_tie", "drop_translation", "small_below")
               if k in planted}
    mask_ge = planted.pop("mask_ge", False)
    n = t["ego"].shape[0]
    xs = [T.pose_vector(t["ego"][i], t["ext"][i if t["ext"].shape[0] > 1 else 0], np.float32, **pose_kw)
          for i in range(n)]
    fw = [T.forward32(t["params"], x, **planted) for x in xs]
    grads = T.backward32(t["params"], xs, [f[1] for f in fw], [f[0] for f in fw], t["grad_affine"], t["grad_reg"],
                         mask_ge=mask_ge)
    return dict(x=np.stack(xs), A=np.stack([f[0] for f in fw]), reg=np.array([f[2] for f in fw]), grads=grads)


def ratios(batch, got, zero_last=False):
    """The worst ratio of every output group against the truth's derived bounds."""
    t = T.truth(batch, zero_last=zero_last)
    fws = t["fws"]
    return dict(
        x=max(T.ratio(got["x"][i], fw["x"], fw["e_x"]) for i, fw in enumerate(fws)),
        A=max(T.ratio(got["A"][i], fw["A"], fw["e_A"]) for i, fw in enumerate(fws)),
        reg=max(T.ratio(got["reg"][i], fw["reg"], fw["e_reg"]) for i, fw in enumerate(fws)),
        grads=max(T.ratio(got["grads"][k], t["grads"][k], t["tols"][k]) for k in T.KEYS))


def yardstick(pose, x):
    """distance of a float32 6-vector from the truth over the 4x yardstick (module docstring of the truth)."""
    x64 = T.truth(pose)["fws"][0]["x"]
    return float(np.abs(np.asarray(x, np.float64) - x64).max()) / T.tol_x(x64, ref_distance(pose))


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_branch():
    got = {}
    for name in T.POSES:
        fw = T.truth(name)["fws"][0]
        got[name] = fw["x"][:3]
        assert 50.0 < np.abs(fw["x"][3:]).max() < 400.0          # a few hundred metres
    assert np.all(got["identity"] == 0.0)
    assert 0 < np.linalg.norm(got["small_2.5e-7"]) < 1e-6 < np.linalg.norm(got["above_4e-6"]) < 1e-5
    assert np.allclose(np.linalg.norm(got["small_2.5e-7"]), 2.5e-7, rtol=1e-5)      # clear of the threshold
    assert np.allclose(np.linalg.norm(got["above_4e-6"]), 4e-6, rtol=1e-5)
    assert np.allclose(got["tie_all_120"], 2 * np.pi / 3 / np.sqrt(3))
    assert np.allclose(got["tie_all_m120"], -2 * np.pi / 3 / np.sqrt(3))
    assert np.allclose(got["half_turn_x"], [np.pi, 0, 0])
    assert np.linalg.norm(got["negative_real"]) > np.pi and got["negative_real"][0] > 0      # -160 deg comes out +200
    for name, best in (("dominant_r", 0), ("dominant_i", 1), ("dominant_j", 2), ("dominant_k", 3)):
        ego, ext = T.build_pose(name)
        d = np.diag((ego.astype(np.float64) @ ext.astype(np.float64))[:3, :3])
        s = 1.0 + np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) @ d
        order = np.argsort(-s)
        assert order[0] == best and np.sqrt(s[order[0]]) - np.sqrt(max(s[order[1]], 0)) > 0.5      # by a margin


@pytest.mark.parametrize("batch", list(T.BATCHES))
def test_every_gradient_case_is_clear_of_the_relu_and_sign_discontinuities(batch):
    for fw in T.truth(batch)["fws"]:
        assert T.mask_margin(fw) > 4.0           # every unit of both networks, none exempted
        assert T.sign_margin(fw) > 2.0


# ---------------------------------------------------------------------------------------------------------------
# the reference's recorded results and the float32 restatement lie inside the bounds
# ---------------------------------------------------------------------------------------------------------------
def test_the_golden_inputs_are_the_builders():
    meta, _ = golden()
    assert "cut with ast" in meta["source"]
    assert [c["name"] for c in meta["cases"]] == list(T.POSES) + ["fresh_dominant_r"]
    for c in meta["cases"]:
        params = T.build_params(c["seed"], c["zero_last"])
        ego, ext = T.build_pose(c["pose"])
        ga, gr = T.build_grad_affine(**c["grad_affine"]), T.build_grad_reg(**c["grad_reg"])
        assert T.sha256(ego, ext, ga, gr, *[params[k] for k in T.KEYS]) == c["sha256"], c["name"]


def test_the_reference_lies_inside_the_bounds():
    meta, arrays = golden()
    for c in meta["cases"]:
        name = c["name"]
        got = dict(x=arrays[name + "/x"][None], A=arrays[name + "/affine"].reshape(1, 2, 12),
                   reg=arrays[name + "/reg"], grads={k: arrays["%s/grad/%s" % (name, k)] for k in T.KEYS})
        r = ratios(c["pose"], got, zero_last=c["zero_last"])
        assert max(r.values()) <= 1.0, (name, r)
        assert yardstick(c["pose"], got["x"][0]) <= 0.25          # its own distance, by construction


@pytest.mark.parametrize("batch", list(T.BATCHES))
def test_the_float32_restatement_lies_inside_the_bounds(batch):
    got = restated(batch)
    r = ratios(batch, got)
    assert max(r.values()) <= 1.0, r
    for i, pose in enumerate(T.BATCHES[batch][0]):
        assert yardstick(pose, got["x"][i]) <= 1.0


def test_a_fresh_module_is_the_identity_with_gradient_in_the_last_layer_only():
    meta, arrays = golden()
    for got in (restated("dominant_r", zero_last=True),
                dict(A=arrays["fresh_dominant_r/affine"].reshape(1, 2, 12), reg=arrays["fresh_dominant_r/reg"],
                     grads={k: arrays["fresh_dominant_r/grad/" + k] for k in T.KEYS})):
        assert np.array_equal(got["A"][0], np.stack([T.EYE, T.EYE]).astype(np.float32))
        assert got["reg"][0] == 0.0
        for k in T.KEYS:
            assert (np.abs(got["grads"][k]).max() > 0) == (".6." in k), k


# ---------------------------------------------------------------------------------------------------------------
# planted errors: each is rejected on the case where it shows
# ---------------------------------------------------------------------------------------------------------------
def test_a_standardised_quaternion_sign_is_rejected():
    assert yardstick("negative_real", restated("negative_real")["x"][0]) <= 1.0
    bad = restated("negative_real", standardise=True)
    assert yardstick("negative_real", bad["x"][0]) > 1e3 and ratios("negative_real", bad)["x"] > 1e3


@pytest.mark.parametrize("pose", ["tie_all_m120", "tie_ij_180_opposed"])
def test_the_last_index_on_a_tie_is_rejected(pose):
    bad = restated(pose, last_on_tie=True)
    assert yardstick(pose, bad["x"][0]) > 1e3 and ratios(pose, bad)["x"] > 1e3


@pytest.mark.parametrize("pose", ["tie_all_120", "tie_ij_180"])
def test_ties_whose_rows_agree_cannot_show_the_pick(pose):
    # 120 deg about (1,1,1) and 180 deg about (1,1,0): every tied candidate row is the same quaternion, sign
    # included, so these two pin the tie's VALUE; the pick itself shows on the two rotations above
    assert np.array_equal(restated(pose, last_on_tie=True)["x"], restated(pose)["x"])


@pytest.mark.parametrize("planted,group", [
    (dict(swap=True), "A"), (dict(no_identity=True), "A"), (dict(transpose_last=True), "A"),
    (dict(mask_ge=True), "grads"), (dict(drop_translation=True), "x"), (dict(small_below=np.inf), "x")])
def test_planted_errors_are_rejected(planted, group):
    # networks swapped / missing + I / last layer transposed / mask >= 0 / translation dropped / the small-angle
    # divisor above the threshold (0.5 - angle^2 / 48 agrees with sin(half) / angle to O(angle^4): it shows on a
    # generic angle, not next to the threshold)
    assert max(ratios("dominant_r", restated("dominant_r")).values()) <= 1.0
    assert ratios("dominant_r", restated("dominant_r", **planted))[group] > 10.0


# ---------------------------------------------------------------------------------------------------------------
# the module: state dicts, no CPU path
# ---------------------------------------------------------------------------------------------------------------
def _independent():
    def net():
        return nn.Sequential(nn.Linear(6, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(),
                             nn.Linear(64, 12))

    class Reference(nn.Module):
        def __init__(self):
            super().__init__()
            self.affine_trans, self.affine_trans_sky = net(), net()
    return Reference()


def test_state_dicts_interchange_with_an_independent_sequential():
    from gaussianrpg_amd.appearance import MLP_KEYS, ColorCorrection, ColorCorrectionMLP
    assert MLP_KEYS == T.KEYS
    cc = ColorCorrectionMLP()
    sd = cc.save_state_dict(is_final=True)
    assert list(sd) == ["params"] and tuple(sd["params"]) == T.KEYS             # identity_matrix is not persistent
    assert tuple(_independent().state_dict()) == T.KEYS
    for net in T.NETS:
        assert not sd["params"][net + ".6.weight"].any() and not sd["params"][net + ".6.bias"].any()
        assert sd["params"][net + ".0.weight"].any() and sd["params"][net + ".4.bias"].any()
    assert torch.equal(cc.identity_matrix, torch.eye(4)[:3])
    ref = _independent()
    ref.load_state_dict(sd["params"])                                            # ours -> theirs
    theirs = _independent()
    cc.load_state_dict({"params": theirs.state_dict()})                          # theirs -> ours
    for k, v in theirs.state_dict().items():
        assert torch.equal(cc.state_dict()[k], v)
    with pytest.raises(ValueError, match="explicit variant"):
        cc.load_state_dict(ColorCorrection(2).save_state_dict())
    with pytest.raises(ValueError, match="use_mlp"):                             # unchanged
        ColorCorrection(2).load_state_dict(sd)
    with pytest.raises(ValueError, match="Invalid mode"):
        ColorCorrectionMLP(mode="frame")


def test_a_copy_of_the_module_leaves_the_cache_behind():
    import copy
    from gaussianrpg_amd.appearance import ColorCorrectionMLP
    cc = ColorCorrectionMLP()
    cc._cached = ("key", object(), None, None, {"consumed": False}, cc.affine_trans[0].weight * 2.0, None)   # non-leaf
    twin = copy.deepcopy(cc)
    assert twin._cached is None and cc._cached is not None
    assert all(torch.equal(a, b) and a is not b for a, b in zip(cc.parameters(), twin.parameters()))


def test_no_cpu_path():
    from gaussianrpg_amd.appearance import ColorCorrectionMLP
    cc = ColorCorrectionMLP()
    with pytest.raises(RuntimeError, match="no CPU path"):
        cc.affines(torch.eye(4)[None], torch.eye(4)[None])


# ---------------------------------------------------------------------------------------------------------------
# the checkpoint loader
# ---------------------------------------------------------------------------------------------------------------
def _models():
    from gaussianrpg_amd.composed import ModelParams
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen)                                              # noqa: E731
    return {"background": ModelParams(r(7, 3), r(7, 3), r(7, 4), r(7, 1), r(7, 1, 3), r(7, 3, 3))}


def test_checkpoint_loader_builds_the_module_from_a_use_mlp_entry(tmp_path):
    from gaussianrpg_amd import checkpoint as ck
    params = {k: torch.from_numpy(v) for k, v in T.build_params().items()}
    sd = ck.state_dict_of(_models())
    plain = str(tmp_path / "plain.pth")
    torch.save(sd, plain)
    assert ck.load_checkpoint(plain).color_correction_mlp() is None
    sd["color_correction"] = {"params": params}
    path = str(tmp_path / "mlp.pth")
    torch.save(sd, path)
    loaded = ck.load_checkpoint(path)
    assert loaded.names() == ["background"]
    for mode in ("image", "sensor"):
        cc = loaded.color_correction_mlp(mode=mode)
        assert cc.mode == mode and tuple(cc.state_dict()) == T.KEYS
        for k in T.KEYS:
            assert torch.equal(cc.state_dict()[k], params[k])
    with pytest.raises(ValueError, match="use_mlp"):                             # the explicit loader, unchanged
        loaded.color_correction_module()
    # an incomplete entry names what is missing
    gone = ["affine_trans.4.bias", "affine_trans_sky.6.weight"]
    sd["color_correction"] = {"params": {k: v for k, v in params.items() if k not in gone}}
    torch.save(sd, path)
    with pytest.raises(ValueError) as e:
        ck.load_checkpoint(path).color_correction_mlp()
    assert all(k in str(e.value) for k in gone) and "affine_trans.0.weight" not in str(e.value)
    # the explicit variant is incomplete for this loader
    eye = torch.eye(4)[:3].repeat(2, 1, 1)
    sd["color_correction"] = {"params": {"affine_trans": eye, "affine_trans_sky": eye.clone()}}
    torch.save(sd, path)
    with pytest.raises(ValueError, match="affine_trans.0.weight"):
        ck.load_checkpoint(path).color_correction_mlp()
    assert ck.load_checkpoint(path).color_correction_module() is not None
    ply = str(tmp_path / "scene.ply")
    ck.write_ply(ply, _models())
    assert ck.load_checkpoint(ply).color_correction_mlp() is None


# ---------------------------------------------------------------------------------------------------------------
# exports and build
# ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_the_abi_version_stays():
    from gaussianrpg_amd import build
    with open(os.path.join(ROOT, "include", "grpg_rasterizer.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in ("grpg_color_mlp_forward", "grpg_color_mlp_backward"):
        assert re.search(r"GRPG_API\s+\w+\s+%s\(" % name, header), name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+GRPG_ABI_VERSION\s+7\b", header)
    assert "-ffp-contract=off" in build.HIP_UNITS["color_mlp.hip"]


def test_the_kernels_use_no_scratch():
    from gaussianrpg_amd import build
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    res = build.kernel_resources("color_mlp.hip")
    for tag in ("color_mlp_forward_kernel", "color_mlp_backward_kernel"):
        hits = [k for k in res if tag in k]
        assert len(hits) == 1, (tag, sorted(res))
        assert res[hits[0]]["scratch"] == 0, res[hits[0]]
