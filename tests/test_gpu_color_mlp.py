"""-m gpu: the use_mlp colour correction's kernels (csrc/color_mlp.hip) through ``appearance.ColorCorrectionMLP``.

Every batch of tests/color_mlp_truth.py -- the pose cases that reach each branch of the axis-angle, alone and as T = 2
and T = 5 calls, with one extrinsic shared or one per camera -- against the float64 truth's derived bounds (ratio <= 1;
for the 6-vector also the 4x yardstick against the reference's recorded distance), forward and backward; the layers bit
for bit against the float32 numpy restatement fed the kernel's own ``x``; batching, repeatability, the fresh module,
the regulariser, the per-camera cache, the unfused route, and the matrix going from device memory into
``forward_frame``.  The parity ratios are collected in bench_out/color_mlp_parity.json (committed copy:
profiles/color_mlp_parity.json)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import color_mlp_truth as T
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _record(name, figures):
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "color_mlp_parity.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[name] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def _module(dev, zero_last=False):
    from gaussianrpg_amd.appearance import ColorCorrectionMLP
    cc = ColorCorrectionMLP()
    cc.load_state_dict({"params": {k: torch.from_numpy(v) for k, v in T.build_params(zero_last=zero_last).items()}})
    return cc.to(dev)


_RUNS = {}


def run(dev, batch, zero_last=False):
    """One forward and one backward launch of a batch with the truth's upstream gradients: numpy outputs; computed
    once -- read-only."""
    key = (batch, zero_last)
    if key not in _RUNS:
        t = T.truth(batch, zero_last=zero_last)
        cc = _module(dev, zero_last)
        ego, ext = torch.from_numpy(t["ego"]).to(dev), torch.from_numpy(t["ext"]).to(dev)
        affine, reg, x = cc.affines_and_reg(ego, ext)
        assert affine.shape == (len(ego), 2, 3, 4) and reg.shape == (len(ego),) and x.shape == (len(ego), 6)
        assert not x.requires_grad
        loss = (affine * torch.from_numpy(t["grad_affine"]).to(dev)).sum() + \
            (reg * torch.from_numpy(t["grad_reg"]).to(dev)).sum()
        loss.backward()
        sd = dict(cc.named_parameters())
        _RUNS[key] = dict(x=x.cpu().numpy(), A=affine.detach().cpu().numpy().reshape(-1, 2, 12),
                          reg=reg.detach().cpu().numpy(), grads={k: sd[k].grad.cpu().numpy() for k in T.KEYS})
    return _RUNS[key]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(name, a, b):
    assert np.shape(a) == np.shape(b), (name, np.shape(a), np.shape(b))
    assert np.array_equal(_bits(a), _bits(b)), "%s: %d of %d values differ" % (
        name, int((_bits(a) != _bits(b)).sum()), np.size(a))


def _ref_distance(pose):
    arrays = np.load(os.path.join(ROOT, "tests", "golden", "ref_color_mlp.npz"))
    return float(np.abs(arrays[pose + "/x"].astype(np.float64) - T.truth(pose)["fws"][0]["x"]).max())


@pytest.mark.parametrize("batch", list(T.BATCHES))
def test_forward_and_backward_lie_inside_the_bounds(dev, batch):
    t, got = T.truth(batch), run(dev, batch)
    fws = t["fws"]
    r = dict(x=max(T.ratio(got["x"][i], fw["x"], fw["e_x"]) for i, fw in enumerate(fws)),
             x_yardstick=max(float(np.abs(got["x"][i] - fw["x"]).max()) / T.tol_x(fw["x"], _ref_distance(pose))
                             for i, (fw, pose) in enumerate(zip(fws, T.BATCHES[batch][0]))),
             affine=max(T.ratio(got["A"][i], fw["A"], fw["e_A"]) for i, fw in enumerate(fws)),
             reg=max(T.ratio(got["reg"][i], fw["reg"], fw["e_reg"]) for i, fw in enumerate(fws)))
    for k in T.KEYS:
        r["grad/" + k] = T.ratio(got["grads"][k], t["grads"][k], t["tols"][k])
    print(batch, json.dumps(r))
    _record(batch, r)
    assert max(r.values()) <= 1.0, r


def test_special_poses_come_out_as_the_branch_table_says(dev):
    assert np.all(run(dev, "identity")["x"][0, :3] == 0.0)                         # exactly zero
    x = run(dev, "negative_real")["x"][0]
    assert x[0] > np.pi and x[1] == 0 and x[2] == 0                                # no sign standardisation
    assert run(dev, "tie_all_m120")["x"][0, 0] < 0 and run(dev, "tie_ij_180_opposed")["x"][0, 1] < 0    # first index
    assert abs(run(dev, "half_turn_x")["x"][0, 0] - np.pi) < 1e-6


@pytest.mark.parametrize("batch", ["dominant_r", "small_2.5e-7", "negative_real", "T5_mixed", "T5_shared"])
def test_layers_are_bit_identical_to_the_restatement(dev, batch):
    t, got = T.truth(batch), run(dev, batch)
    fw = [T.forward32(t["params"], x) for x in got["x"]]
    _same("affine", got["A"], np.stack([f[0] for f in fw]))
    _same("reg", got["reg"], np.array([f[2] for f in fw]))
    grads = T.backward32(t["params"], got["x"], [f[1] for f in fw], got["A"], t["grad_affine"], t["grad_reg"])
    for k in T.KEYS:
        _same(k, got["grads"][k], grads[k])


def test_hidden_output_is_the_restatement(dev):
    from gaussianrpg_amd.rasterizer import _C
    t = T.truth("T2_shared")
    cc = _module(dev)
    p = cc._params()
    affine, x, reg, hidden = _C.color_mlp_forward(p[:8], p[8:], torch.from_numpy(t["ego"]).to(dev),
                                                  torch.from_numpy(t["ext"]).to(dev), True, True)
    for i in range(2):
        _same("hidden", hidden[i].cpu().numpy(), T.forward32(t["params"], x[i].cpu().numpy())[1])
    only, _, none_reg, none_hidden = _C.color_mlp_forward(p[:8], p[8:], torch.from_numpy(t["ego"]).to(dev),
                                                          torch.from_numpy(t["ext"]).to(dev), False, False)
    assert none_reg is None and none_hidden is None
    _same("affine without reg / hidden", only.cpu().numpy(), affine.cpu().numpy())


@pytest.mark.parametrize("batch", ["T5_mixed", "T5_shared", "T2_shared"])
def test_a_row_of_a_batch_is_the_single_call(dev, batch):
    got = run(dev, batch)
    for i, pose in enumerate(T.BATCHES[batch][0]):
        one = run(dev, pose)
        for k in ("x", "A", "reg"):
            _same("%s %s" % (pose, k), got[k][i], one[k][0])


def test_identical_calls_give_identical_bits(dev):
    first = run(dev, "T5_mixed")
    _RUNS.pop(("T5_mixed", False))
    second = run(dev, "T5_mixed")
    for k in ("x", "A", "reg"):
        _same(k, first[k], second[k])
    for k in T.KEYS:
        _same(k, first["grads"][k], second["grads"][k])


def test_a_fresh_module_is_the_identity_with_gradient_in_the_last_layer_only(dev):
    got = run(dev, "dominant_r", zero_last=True)
    _same("affine", got["A"][0], np.stack([T.EYE, T.EYE]).astype(np.float32))
    assert got["reg"][0] == 0.0
    for k in T.KEYS:
        assert (np.abs(got["grads"][k]).max() > 0) == (".6." in k), k
    t = T.truth("dominant_r", zero_last=True)
    assert max(T.ratio(got["grads"][k], t["grads"][k], t["tols"][k]) for k in T.KEYS) <= 1.0


def test_regulariser_alone_and_matrix_alone(dev):
    """the two upstream gradients one at a time (the other pointer NULL in the backward) add up to both"""
    t = T.truth("dominant_k")
    cc = _module(dev)
    ego, ext = torch.from_numpy(t["ego"]).to(dev), torch.from_numpy(t["ext"]).to(dev)
    ga, gr = torch.from_numpy(t["grad_affine"]).to(dev), torch.from_numpy(t["grad_reg"]).to(dev)
    params = list(cc.parameters())
    affine, reg, _ = cc.affines_and_reg(ego, ext)
    g_reg = torch.autograd.grad((reg * gr).sum(), params, retain_graph=True)
    g_aff = torch.autograd.grad((affine * ga).sum(), params)
    t_reg = T.backward64(t["params"], t["fws"], None, t["grad_reg"])
    t_aff = T.backward64(t["params"], t["fws"], t["grad_affine"], None)
    for (k, _), a, b in zip(cc.named_parameters(), g_reg, g_aff):
        assert T.ratio(a.cpu().numpy(), t_reg[0][k], t_reg[1][k]) <= 1.0, k
        assert T.ratio(b.cpu().numpy(), t_aff[0][k], t_aff[1][k]) <= 1.0, k
    assert abs(float(reg.detach()[0]) - t["fws"][0]["reg"]) <= t["fws"][0]["e_reg"]


def _camera(dev, pose):
    ego, ext = T.build_pose(pose)
    return types.SimpleNamespace(ego_pose=torch.from_numpy(ego).to(dev), extrinsic=torch.from_numpy(ext).to(dev),
                                 id=0, meta=dict(cam=0))


def test_one_training_iteration_is_one_launch_each_way(dev, monkeypatch):
    from gaussianrpg_amd import appearance
    calls = dict(fwd=0, bwd=0)
    real = appearance._C

    class Counting:
        def __getattr__(self, name):
            if name == "color_mlp_forward":
                calls["fwd"] += 1
            if name == "color_mlp_backward":
                calls["bwd"] += 1
            return getattr(real, name)
    monkeypatch.setattr(appearance, "_C", Counting())
    cc = _module(dev)
    cam = _camera(dev, "dominant_i")
    image = torch.rand(3, 5, 7, device=dev)

    def iteration():
        out = cc(cam, image) + cc(cam, image, use_sky=True)
        loss = out.sum() + cc.regularization_loss(cam)
        loss.backward()
        return {k: p.grad.clone() for k, p in cc.named_parameters()}
    grads = iteration()
    assert calls == dict(fwd=1, bwd=1)
    # the same again without an optimizer step: the spent node is not handed out a second time
    for p in cc.parameters():
        p.grad = None
    again = iteration()
    assert calls == dict(fwd=2, bwd=2)
    for k in grads:
        assert torch.equal(grads[k], again[k]), k
    # an in-place parameter update, another pose tensor, another camera or no_grad: a new launch
    A0 = cc.get_affine_trans(cam)
    assert calls["fwd"] == 3 and cc.get_affine_trans(cam, use_sky=True) is not None and calls["fwd"] == 3
    with torch.no_grad():
        cc.affine_trans[6].bias.add_(1.0)
    A1 = cc.get_affine_trans(cam)
    assert calls["fwd"] == 4 and float((A1.detach() - A0.detach() - 1.0).abs().max()) < 1e-4
    cam.ego_pose[0, 3] += 1.0
    assert not torch.equal(cc.get_affine_trans(cam), A1) and calls["fwd"] == 5
    cc.get_affine_trans(_camera(dev, "dominant_i"))
    assert calls["fwd"] == 6
    with torch.no_grad():
        assert not cc.get_affine_trans(cam).requires_grad
    assert calls["fwd"] == 7 and cc.get_affine_trans(cam).requires_grad and calls["fwd"] == 8
    # the cached and the uncached route agree bit for bit
    cached = cc.get_affine_trans(cam, use_sky=True).detach().cpu().numpy()
    assert calls["fwd"] == 8
    cc.cache = False
    _same("uncached", cc.get_affine_trans(cam, use_sky=True).detach().cpu().numpy(), cached)
    assert calls["fwd"] == 9
    before = calls["fwd"]
    cc.regularization_loss(cam)
    assert calls["fwd"] == before + 1


def test_the_unfused_route_lies_inside_the_bounds_too(dev):
    cc = _module(dev)
    for pose in ("dominant_j", "small_2.5e-7", "tie_all_m120", "negative_real"):
        fw = T.truth(pose)["fws"][0]
        cam = _camera(dev, pose)
        for n, use_sky in enumerate((False, True)):
            A = hz.camera_affine(cc, cam, fused=False, use_sky=use_sky)
            assert T.ratio(A.detach().cpu().numpy().reshape(12), fw["A"][n], fw["e_A"][n]) <= 1.0
            fused = hz.camera_affine(cc, cam, fused=True, use_sky=use_sky)
            assert T.ratio(fused.detach().cpu().numpy().reshape(12), fw["A"][n], fw["e_A"][n]) <= 1.0


def test_the_matrix_goes_from_device_memory_into_the_frame(dev):
    """forward_frame(affine=affines[0,0]) -- a view into the [T,2,3,4] output -- gives the bytes of the row cloned, and
    simulator_frame_corrected takes the module in place of a matrix."""
    W, H = 200, 136                       # the smallest frame of tests/test_gpu_frame_corrected.py
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    scene = hz.toy_scene(P=2000).to(dev)
    cam = hz.trajectory_camera(1, W=W, H=H, device=dev)
    rast = GaussianRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(
        cam, scene.sh_degree, bg=torch.zeros(3, device=dev))))
    cc = _module(dev)
    camera = _camera(dev, "dominant_r")
    kw = dict(shs=scene.shs, scales=scene.scales, rotations=scene.rotations)
    with torch.no_grad():
        A = cc.affines(camera.ego_pose[None], camera.extrinsic[None])
        view = rast.forward_frame(scene.means3D, scene.opacity, affine=A[0, 0], **kw)["rgb8"]
        clone = rast.forward_frame(scene.means3D, scene.opacity, affine=A[0, 0].clone(), **kw)["rgb8"]
        plain = rast.forward_frame(scene.means3D, scene.opacity, **kw)["rgb8"]
        sky = rast.forward_frame(scene.means3D, scene.opacity, affine=A[0, 1], **kw)["rgb8"]
    assert view.shape == (H, W, 3) and torch.equal(view, clone)
    assert not torch.equal(view, plain) and not torch.equal(view, sky)          # the correction, and the right row
    for one_call in (True, False):
        got = hz.simulator_frame_corrected(scene, cam, cc, camera=camera, one_call=one_call)
        want = hz.simulator_frame_corrected(scene, cam, A[0, 0].clone(), one_call=one_call)
        assert np.array_equal(got, want)
        if one_call:
            assert np.array_equal(got, view.cpu().numpy())
    with pytest.raises(ValueError, match="camera"):
        hz.simulator_frame_corrected(scene, cam, cc)
