"""CPU tests (-m "not gpu") of the colour correction: the float64 truth and its bounds (tests/color_correction_truth.py)
against what the reference itself returned (tests/golden/ref_color_correction.*), against the kernel's arithmetic
restated in float32 numpy and against planted errors; the module's state dicts, the checkpoint loader's handling of
the ``color_correction`` entry and the declared exports.  The kernels run in tests/test_gpu_color_correction.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import color_correction_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
EXPORTS = ("grpg_color_correct_forward", "grpg_color_correct_backward", "grpg_color_correct_workspace_bytes")


def _golden():
    with open(os.path.join(GOLDEN, "ref_color_correction.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "ref_color_correction.npz"))


def golden_params(kind, n=3):
    a = np.stack([T.build_affine(kind, seed=k) for k in range(n)])
    s = np.stack([T.build_affine(kind, seed=100 + k) for k in range(n)])
    return a, s


GOLDEN_NAMES = [c["name"] for c in _golden()[0]["cases"]]


# ---------------------------------------------------------------------------------------------------------------
# the reference's own float32 results lie inside the bounds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_reference_results_lie_inside_the_bounds(name):
    meta, arrays = _golden()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    image, g = T.build_case("image", c["image"]), T.build_case("grad", c["grad"])
    a, s = golden_params(c["kind"], c["num_corrections"])
    assert T.sha256(image, g, a, s) == c["sha256"], "the builders no longer give the fixture's inputs"
    assert c["id"] == (c["camera_id"] if c["mode"] == "image" else c["camera_cam"])
    A = (s if c["use_sky"] else a)[c["id"]]
    y64, tol = T.forward64(A, image)
    b = T.backward64(A, image, g)
    r = dict(out=T.ratio(arrays[name + "/out"], y64, tol),
             g_x=T.ratio(arrays[name + "/grad_image"], b["g_x"], b["tol_g_x"]),
             grad_A=T.ratio(arrays[name + "/grad_param"][c["id"]], b["grad_A"], b["tol_A"]))
    print(name, r)
    assert max(r.values()) <= 1.0, r
    other = np.delete(arrays[name + "/grad_param"], c["id"], axis=0)
    assert (other == 0).all(), "the gradient reaches a row the camera does not use"
    eye = np.eye(4)[:3]
    reg64 = (np.abs(a[c["id"]].astype(np.float64) - eye) + np.abs(s[c["id"]].astype(np.float64) - eye)).mean()
    assert abs(float(arrays[name + "/reg_loss"][0]) - reg64) <= 32 * T.U * max(reg64, 1e-30) + 1e-45
    if c["kind"] != "identity":
        sign = np.sign(a[c["id"]].astype(np.float64) - eye) / 12.0
        np.testing.assert_allclose(arrays[name + "/reg_grad"][c["id"]], sign, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy lies inside the bounds; CPU torch's einsum too
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", T.MATRICES)
def test_float32_restatement_lies_inside_the_bounds(shape, kind):
    H, W = shape
    A, x, g = T.build_affine(kind, seed=H), T.build_image(H, W, seed=1), T.build_grad(H, W, seed=2)
    y64, tol = T.forward64(A, x)
    b = T.backward64(A, x, g)
    y32 = T.forward32(A, x)
    g_x32, grad_A32 = T.backward32(A, x, g)
    r = dict(out=T.ratio(y32, y64, tol), g_x=T.ratio(g_x32, b["g_x"], b["tol_g_x"]),
             grad_A=T.ratio(grad_A32, b["grad_A"], b["tol_A"]))
    print(shape, kind, r, "d =", T.chain_depth(H, W))
    assert max(r.values()) <= 1.0, r
    if kind == "identity":
        assert np.array_equal(y32, x) and np.array_equal(g_x32, g)
    # the reference's own line on CPU torch
    At, xt = torch.from_numpy(A), torch.from_numpy(x).requires_grad_(True)
    At.requires_grad_(True)
    yt = torch.einsum('ij, jhw -> ihw', At[:3, :3], xt) + At[:3, 3].unsqueeze(-1).unsqueeze(-1)
    yt.backward(torch.from_numpy(g))
    rt = dict(out=T.ratio(yt.detach().numpy(), y64, tol), g_x=T.ratio(xt.grad.numpy(), b["g_x"], b["tol_g_x"]),
              grad_A=T.ratio(At.grad.numpy(), b["grad_A"], b["tol_A"]))
    print(shape, kind, "torch", rt)
    assert max(rt.values()) <= 1.0, rt


def test_chain_depth_follows_the_workgroup_count():
    assert T.blocks(1, 1) == 1 and T.blocks(5, 67) == 4 and T.blocks(9, 130) == 9
    assert T.blocks(373, 707) == 12 * 94 > 1024
    assert [T.chain_depth(*s) for s in T.SHAPES] == [19, 19, 19, 20]
    assert T.chain_depth(1280, 1920) == 28 and T.chain_depth(4 * 1024, 64) == 19 and T.chain_depth(4 * 1025, 64) == 20


# ---------------------------------------------------------------------------------------------------------------
# planted errors are rejected
# ---------------------------------------------------------------------------------------------------------------
def test_planted_errors_are_rejected():
    H, W = 9, 130
    A, x, g = T.build_affine("wide", seed=3), T.build_image(H, W, seed=1), T.build_grad(H, W, seed=2)
    y64, tol = T.forward64(A, x)
    b = T.backward64(A, x, g)
    assert T.ratio(T.forward32(A, x), y64, tol) <= 1.0
    At = A.copy()
    At[:, :3] = A[:, :3].T
    assert T.ratio(T.forward32(At, x), y64, tol) > 1e3, "a transposed matrix passes"
    A0 = A.copy()
    A0[:, 3] = 0
    assert T.ratio(T.forward32(A0, x), y64, tol) > 1e3, "a missing translation column passes"
    g_x_wrong = np.einsum("ij,jhw->ihw", A[:, :3], g).astype(np.float32)          # A in place of A^T
    assert T.ratio(g_x_wrong, b["g_x"], b["tol_g_x"]) > 1e3
    # the clamp in front of the affine map instead of behind it
    yc64, tolc = T.forward64(A, x, clamp=True)
    wrong = T.forward32(A, np.clip(x, 0, 1))
    assert T.ratio(np.clip(T.forward32(A, x), 0, 1), yc64, tolc) <= 1.0
    assert T.ratio(wrong, yc64, tolc) > 1e3, "clamping before the affine map passes"
    # near-identity too: the two differ wherever x leaves [0,1]
    An = T.build_affine("near", seed=3)
    yn64, toln = T.forward64(An, x, clamp=True)
    assert T.ratio(T.forward32(An, np.clip(x, 0, 1)), yn64, toln) > 1e3


@pytest.mark.parametrize("where", ["first", "last", "row_end", "partial_block"])
def test_one_hot_sum_rejects_a_dropped_pixel(where):
    H, W = 9, 130
    A, x = T.build_affine("near", seed=4), T.build_image(H, W, seed=5)
    py, px = {"first": (0, 0), "last": (H - 1, W - 1), "row_end": (0, W - 1), "partial_block": (8, 128)}[where]
    g = np.zeros((3, H, W), np.float32)
    g[:, py, px] = (0.75, -1.25, 2.5)
    b = T.backward64(A, x, g)
    g_x32, grad_A32 = T.backward32(A, x, g)
    assert np.array_equal(grad_A32[:, 3], g[:, py, px])                     # adding zeros is exact
    assert np.array_equal(grad_A32[:, :3], np.outer(g[:, py, px], x[:, py, px]).astype(np.float32))
    assert T.ratio(grad_A32, b["grad_A"], b["tol_A"]) <= 1.0
    dropped = np.zeros((3, 4), np.float32)                                   # the pixel never reaches the sum
    assert T.ratio(dropped, b["grad_A"], b["tol_A"]) > 1e3
    assert T.ratio(2 * grad_A32, b["grad_A"], b["tol_A"]) > 1e3              # ... or reaches it twice


# ---------------------------------------------------------------------------------------------------------------
# bytes at the simulator's frame size: the reference's float32 route differs from the truth only at fragile values
# ---------------------------------------------------------------------------------------------------------------
def test_reference_bytes_differ_from_the_truth_only_at_fragile_values():
    """The GPU test of harness.simulator_frame_corrected asks the same of both routes, with the same matrix, on a
    rendered frame of this size; a frame cannot be rendered here, so the planes are the builder's."""
    H, W = 375, 1242
    A, x = T.build_affine("near", seed=9), T.build_image(H, W, seed=9)
    y64, tol = T.forward64(A, x)
    At, xt = torch.from_numpy(A), torch.from_numpy(x)
    y = torch.einsum('ij, jhw -> ihw', At[:3, :3], xt) + At[:3, 3].unsqueeze(-1).unsqueeze(-1)
    got = (torch.clamp(y, 0.0, 1.0).numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    fragile = T.fragile_bytes(y64, tol).transpose(1, 2, 0)
    share = float(fragile.any(axis=2).mean())
    differ = got != T.bytes64(y64)
    print("fragile pixels: %.3g of the frame; bytes that differ: %d" % (share, int(differ.sum())))
    assert not (differ & ~fragile).any()
    assert share < 1e-3


# ---------------------------------------------------------------------------------------------------------------
# the module: state dicts with the reference's key names; no CPU path
# ---------------------------------------------------------------------------------------------------------------
def test_module_state_dicts_round_trip_with_the_reference_key_names():
    from gaussianrpg_amd.appearance import ColorCorrection
    cc = ColorCorrection(3, mode="sensor")
    assert list(cc.state_dict()) == ["affine_trans", "affine_trans_sky"]          # color_correction.py:52-53
    eye = torch.eye(4)[:3]
    for p in (cc.affine_trans, cc.affine_trans_sky):
        assert p.shape == (3, 3, 4) and p.requires_grad and all(torch.equal(p[k], eye) for k in range(3))
    a, s = golden_params("wide")
    ref_sd = {"params": {"affine_trans": torch.from_numpy(a), "affine_trans_sky": torch.from_numpy(s)}}
    cc.load_state_dict(ref_sd)                                                    # what the reference saved
    saved = cc.save_state_dict(is_final=True)
    assert list(saved) == ["params"] and list(saved["params"]) == ["affine_trans", "affine_trans_sky"]
    cc2 = ColorCorrection(3, mode="sensor")
    cc2.load_state_dict(saved)
    assert torch.equal(cc2.affine_trans, torch.from_numpy(a)) and torch.equal(cc2.affine_trans_sky, torch.from_numpy(s))

    class Cam:
        id, meta = 2, {"cam": 1}
    assert cc.get_id(Cam) == 1 and ColorCorrection(3, mode="image").get_id(Cam) == 2
    assert torch.equal(cc.get_affine_trans(Cam, use_sky=True), torch.from_numpy(s[1]))
    assert cc.cur_affine_trans is not None
    reg = cc.regularization_loss(Cam)
    want = (np.abs(a[1].astype(np.float64) - np.eye(4)[:3]) + np.abs(s[1].astype(np.float64) - np.eye(4)[:3])).mean()
    assert reg.requires_grad and abs(float(reg.detach()) - want) < 1e-6
    with pytest.raises(ValueError, match="Invalid mode"):
        ColorCorrection(3, mode="frame")
    with pytest.raises(ValueError, match="use_mlp"):
        cc.load_state_dict({"params": {"affine_trans.0.weight": torch.zeros(64, 6)}})


def test_no_cpu_path():
    from gaussianrpg_amd.appearance import ColorCorrection, color_correct
    with pytest.raises(RuntimeError, match="no CPU path"):
        color_correct(torch.zeros(3, 4, 4), torch.eye(4)[:3])

    class Cam:
        id, meta = 0, {"cam": 0}
    with pytest.raises(RuntimeError, match="no CPU path"):
        ColorCorrection(1)(Cam, torch.zeros(3, 4, 4))


# ---------------------------------------------------------------------------------------------------------------
# the checkpoint loader keeps the entry
# ---------------------------------------------------------------------------------------------------------------
def _models():
    from gaussianrpg_amd.composed import ModelParams
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen)                                              # noqa: E731
    return {"background": ModelParams(r(7, 3), r(7, 3), r(7, 4), r(7, 1), r(7, 1, 3), r(7, 3, 3))}


def test_checkpoint_loader_keeps_the_color_correction_entry(tmp_path):
    from gaussianrpg_amd import checkpoint as ck
    a, s = golden_params("near")
    sd = ck.state_dict_of(_models())
    plain = str(tmp_path / "plain.pth")
    torch.save(sd, plain)
    assert ck.load_checkpoint(plain).color_correction is None
    assert ck.load_checkpoint(plain).color_correction_module() is None
    sd["color_correction"] = {"params": {"affine_trans": torch.from_numpy(a), "affine_trans_sky": torch.from_numpy(s)}}
    path = str(tmp_path / "cc.pth")
    torch.save(sd, path)
    loaded = ck.load_checkpoint(path)
    assert loaded.names() == ["background"]                    # the entry is no model
    assert list(loaded.color_correction) == ["affine_trans", "affine_trans_sky"]
    cc = loaded.color_correction_module(mode="sensor")
    assert cc.mode == "sensor" and torch.equal(cc.affine_trans.detach(), torch.from_numpy(a))
    assert torch.equal(cc.affine_trans_sky.detach(), torch.from_numpy(s))
    assert ck.load_checkpoint(path, color_correction=False).color_correction is None       # withheld on request
    # the use_mlp variant: the models load, the module says what it cannot build
    sd["color_correction"] = {"params": {"affine_trans.0.weight": torch.zeros(64, 6),
                                         "affine_trans.0.bias": torch.zeros(64),
                                         "affine_trans_sky.0.weight": torch.zeros(64, 6)}}
    mlp = str(tmp_path / "mlp.pth")
    torch.save(sd, mlp)
    loaded = ck.load_checkpoint(mlp)
    assert loaded.num_gaussians() == 7 and loaded.color_correction is not None
    with pytest.raises(ValueError, match="use_mlp"):
        loaded.color_correction_module()
    ply = str(tmp_path / "m.ply")
    ck.write_ply(ply, _models())
    assert ck.load_checkpoint(ply).color_correction is None


# ---------------------------------------------------------------------------------------------------------------
# the declared exports
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    import torch  # noqa: F401  (loads the same libamdhip64 the extension will use)
    return ctypes.CDLL(LIB)


def test_exports_are_declared_built_and_bound(lib):
    text = open(HEADER).read()
    declared = set(re.findall(r"GRPG_API\s+[\w\s\*]+?\b(grpg_\w+)\s*\(", text))
    for name in EXPORTS:
        assert name in declared and hasattr(lib, name)
    assert re.search(r"#define\s+GRPG_ABI_VERSION\s+7\b", text)
    from gaussianrpg_amd import build
    assert "-ffp-contract=off" in build.HIP_UNITS["color_correction.hip"]
    from gaussianrpg_amd.rasterizer import _C
    assert hasattr(_C, "color_correct") and hasattr(_C, "color_correct_backward")
    assert _C.color_correct_workspace_bytes(373, 707) == 12 * 4 * T.blocks(373, 707)


def test_workspace_query_needs_no_device_and_entries_fail_loudly_without_one(lib):
    q = lib.grpg_color_correct_workspace_bytes
    q.restype = ctypes.c_size_t
    for (H, W) in T.SHAPES + [(1280, 1920)]:
        assert q(W, H) == 12 * 4 * T.blocks(H, W)
    assert q(0, 4) == 0 and q(4, 0) == 0 and q(-3, 4) == 0
    if torch.cuda.is_available():
        return                                             # the no-device path cannot be exercised here
    lib.grpg_last_error.restype = ctypes.c_char_p
    f, b = lib.grpg_color_correct_forward, lib.grpg_color_correct_backward
    f.restype = b.restype = ctypes.c_int
    z = ctypes.c_float(0.0)
    assert f(4, 4, None, None, None, 0, None, 0, z, None, None, None, 0, None, None, 1, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert b(4, 4, None, None, None, 0, None, 0, z, None, None, None, None, None, None, None, None) == -2
