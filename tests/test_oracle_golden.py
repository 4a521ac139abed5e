"""CPU tests (-m "not gpu"): pin the oracle.

* against the reference-derived vectors (tests/golden/ref_*.npz, made by importing
  /root/reference/lib/utils/{sh_utils,graphics_utils}.py -- see make_golden.py);
* against the committed oracle regression fixtures;
* the two independent restatements (gs_oracle.c vs torch_splat.py) against each other;
* oracle backward against fp64 autograd through the torch splat.
"""
import math
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import torch_splat as ts
from gaussianrpg_amd import harness as hz
from helpers import GOLDEN, assert_image_close, fixture_oracle_inputs, load_fixture, oracle_kwargs


def _identity_cam(W=64, H=48):
    return hz.make_camera(np.eye(3), np.zeros(3), W=W, H=H, fx=60.0, fy=60.0, cx=W / 2, cy=H / 2)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_matches_reference_eval_sh(deg):
    z = np.load(os.path.join(GOLDEN, "ref_sh.npz"))
    means, campos, shs = z["means3D"], z["campos"], z["shs"]
    M = (deg + 1) ** 2
    cam = _identity_cam(W=8192, H=8192)   # wide enough that every point lands on a tile
    kw = oracle_kwargs(cam, deg)
    kw["campos"] = campos      # SH direction only depends on campos (forward.cu:25-27)
    P = means.shape[0]
    o = oracle.forward(means, np.full((P, 1), 0.5, np.float32), shs=shs[:, :M, :].copy(),
                       scales=np.full((P, 3), 0.05, np.float32),
                       rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (P, 1)),
                       render=False, **kw)
    vis = o["radii"] > 0
    assert vis.sum() > 80
    ref = z["eval_sh_deg%d" % deg] + 0.5
    np.testing.assert_allclose(o["rgb"][vis], np.maximum(ref, 0.0)[vis], rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(o["clamped"][vis].astype(bool)[np.abs(ref[vis]) > 1e-5],
                                  (ref[vis] < 0)[np.abs(ref[vis]) > 1e-5])
    r = ts.sh_to_rgb(deg, torch.tensor(shs[:, :M, :]), torch.tensor(z["dirs"])).numpy()
    np.testing.assert_allclose(r, z["eval_sh_deg%d" % deg], rtol=2e-6, atol=2e-6)


def test_camera_conventions_match_reference_graphics_utils():
    z = np.load(os.path.join(GOLDEN, "ref_camera.npz"))
    for i in range(4):
        np.testing.assert_allclose(hz.world2view(z["R%d" % i], z["T%d" % i]), z["w2v%d" % i],
                                   rtol=1e-5, atol=1e-6)
    K = z["K"]
    np.testing.assert_allclose(
        hz.projection_from_K(K[0, 0], K[1, 1], K[0, 2], K[1, 2], 1280, 1920).numpy(),
        z["projK_1920x1280"], rtol=1e-6, atol=1e-7)
    K2 = z["K2"]
    np.testing.assert_allclose(
        hz.projection_from_K(K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2], 360, 640).numpy(),
        z["projK_640x360"], rtol=1e-6, atol=1e-7)
    cam = hz.make_camera(np.eye(3), np.zeros(3))
    np.testing.assert_allclose([2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)],
                               z["focal2fov"], rtol=1e-6)


def test_oracle_projection_uses_reference_matrices():
    """means2D of the oracle == pixel of (Proj @ W2C) applied in fp64 with the reference's own
    getWorld2View2 / getProjectionMatrixK outputs (ndc2Pix: ((v+1)*S-1)/2)."""
    z = np.load(os.path.join(GOLDEN, "ref_camera.npz"))
    R, T = z["R1"], z["T1"]
    W, H = 640, 360
    K2 = z["K2"]
    cam = hz.make_camera(R, T, W=W, H=H, fx=K2[0, 0], fy=K2[1, 1], cx=K2[0, 2], cy=K2[1, 2])
    w2c = z["w2v1"].astype(np.float64)
    full = z["projK_640x360"].astype(np.float64) @ w2c
    rng = np.random.RandomState(3)
    pc = rng.randn(400, 3) * np.array([1.0, 0.6, 1.0]) + np.array([0, 0, 5.0])   # camera space
    pw = (np.linalg.inv(w2c) @ np.c_[pc, np.ones(400)].T).T[:, :3].astype(np.float32)
    o = oracle.forward(pw, np.full((400, 1), 0.5, np.float32), colors_precomp=np.ones((400, 3), np.float32),
                       scales=np.full((400, 3), 0.02, np.float32),
                       rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (400, 1)),
                       render=False, **oracle_kwargs(cam, 0))
    hom = (full @ np.c_[pw.astype(np.float64), np.ones(400)].T).T
    ndc = hom[:, :2] / hom[:, 3:4]
    pix = ((ndc + 1.0) * np.array([W, H]) - 1.0) * 0.5
    vis = o["radii"] > 0
    assert vis.sum() > 100
    np.testing.assert_allclose(o["means2D"][vis], pix[vis], rtol=0, atol=2e-2)
    np.testing.assert_allclose(o["depths"][vis], (w2c @ np.c_[pw, np.ones(400)].T).T[vis, 2], rtol=1e-5)


@pytest.mark.parametrize("name", ["toy_deg1", "toy_deg3_sem", "smoke_deg0", "street_small"])
def test_oracle_regression_fixture(name):
    fx = load_fixture(name)
    S = fx["semantics"].shape[1]
    o = oracle.forward(fx["means3D"], fx["opacity"], shs=fx["shs"], scales=fx["scales"],
                       rotations=fx["rotations"], semantics=fx["semantics"] if S else None,
                       **fixture_oracle_inputs(fx))
    assert o["num_rendered"] == int(fx["num_rendered"])
    for k in ["radii", "keys_sorted", "point_list", "ranges"]:
        np.testing.assert_array_equal(o[k], fx[k], err_msg=k)
    frag = fx["fragile"] | o["fragile"]
    for k in ["color", "depth", "alpha", "semantic"]:
        if fx[k].size:
            assert_image_close(k, o[k], fx[k], frag)
    g = oracle.backward(o, fx["grad_color"], fx["grad_depth"], fx["grad_alpha"], fx["grad_semantic"])
    if not frag.any() or np.array_equal(o["n_contrib"], fx["n_contrib"]):
        for k in ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]:
            scale = np.abs(fx[k]).max() + 1e-12
            assert np.abs(g[k] - fx[k]).max() <= 2e-3 * scale, k


@pytest.mark.parametrize("case", ["toy", "smoke", "street"])
def test_oracle_vs_torch_splat(case):
    if case == "toy":
        sc, cam, S = hz.toy_scene(2500, seed=7, sh_degree=3), hz.trajectory_camera(0, W=200, H=120), 3
    elif case == "smoke":
        sc, cam, S = hz.smoke_scene(1500, seed=3), hz.smoke_camera(128, 96), 0
    else:
        sc, cam, S = hz.street_scene(20000, seed=3), hz.trajectory_camera(3, W=480, H=320), 0
    kw = oracle_kwargs(cam, sc.sh_degree, bg=torch.tensor([0.1, 0.2, 0.3]))
    sem = torch.rand(sc.means3D.shape[0], S, generator=torch.Generator().manual_seed(5)) if S else None
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                       semantics=sem, **kw)
    r = ts.rasterize(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                     semantics=sem, **kw)
    assert o["num_rendered"] == r["num_rendered"]
    np.testing.assert_array_equal(o["radii"], r["radii"].numpy())
    np.testing.assert_array_equal(o["point_list"].astype(np.int64), r["binning"]["point_list"].numpy())
    np.testing.assert_array_equal(o["ranges"].astype(np.int64), r["binning"]["ranges"].numpy())
    for k in ["color", "depth", "alpha", "semantic"]:
        if o[k].size:
            # two CPU restatements with different exp / summation order; a flipped far splat moves
            # the alpha-weighted depth SUM by up to alpha*T*z, hence the wider fragile bound here
            assert_image_close(k, r[k].numpy(), o[k], o["fragile"], max_fragile_frac=0.2,
                               fragile_atol=2e-2)
    nf = o["fragile"] == 0
    assert np.array_equal(o["n_contrib"][nf].astype(np.int64), r["n_contrib"].numpy()[nf].astype(np.int64))


def _fp64_autograd_grads(sc, cam, bg, sem, gc, gd, ga, gs, colors_precomp=None, cov3D=None):
    d = torch.float64
    leaves = dict(means3D=sc.means3D.to(d), opacity=sc.opacity.to(d), scales=sc.scales.to(d),
                  rotations=sc.rotations.to(d), shs=sc.shs.to(d))
    for v in leaves.values():
        v.requires_grad_(True)
    semd = sem.to(d).requires_grad_(True) if sem is not None else None
    kw = oracle_kwargs(cam, sc.sh_degree, bg=bg)
    r = ts.rasterize(leaves["means3D"], leaves["opacity"], shs=leaves["shs"], scales=leaves["scales"],
                     rotations=leaves["rotations"], semantics=semd, **kw)
    loss = (r["color"] * gc.to(d)).sum() + (r["depth"] * gd.to(d)).sum() + (r["alpha"] * ga.to(d)).sum()
    if sem is not None:
        loss = loss + (r["semantic"] * gs.to(d)).sum()
    loss.backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    if sem is not None:
        out["semantics"] = semd.grad.numpy()
    return out, r


@pytest.mark.parametrize("S", [0, 2])
def test_oracle_backward_vs_fp64_autograd(S):
    sc = hz.toy_scene(700, seed=11, sh_degree=2, scale=0.12)
    cam = hz.trajectory_camera(0, W=72, H=56)
    g = torch.Generator().manual_seed(21)
    bg = torch.tensor([0.3, 0.1, 0.6])
    P = sc.means3D.shape[0]
    sem = torch.rand(P, S, generator=g) if S else None
    H, W = cam.image_height, cam.image_width
    gc, gd, ga = torch.randn(3, H, W, generator=g), 0.1 * torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    gs = torch.randn(S, H, W, generator=g)
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                       semantics=sem, **oracle_kwargs(cam, sc.sh_degree, bg=bg))
    go = oracle.backward(o, gc, gd, ga, gs)
    ref, r = _fp64_autograd_grads(sc, cam, bg, sem, gc, gd, ga, gs)
    # decisions can differ between fp32 and fp64 on fragile pixels; require the same contributor
    # sets before comparing gradients tightly
    same = np.array_equal(o["n_contrib"].astype(np.int64), r["n_contrib"].numpy().astype(np.int64))
    tol = 2e-3 if same else 5e-2
    pairs = [("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacity"), ("dL_dscales", "scales"),
             ("dL_drotations", "rotations"), ("dL_dsh", "shs")]
    if S:
        pairs.append(("dL_dsemantic", "semantics"))
    # The reference drops d(t.x)/d(t.z) for Gaussians whose t.x/t.z was clamped to 1.3*tanfov
    # (backward.cu:175-176,258-260 zero dL_dtx but add nothing to dL_dtz), so its mean gradient
    # is knowingly inexact there; autograd is exact.  Compare means only on unclamped Gaussians.
    m = sc.means3D.numpy()
    unclamped = ((np.abs(m[:, 0] / m[:, 2]) < 1.3 * cam.tanfovx)
                 & (np.abs(m[:, 1] / m[:, 2]) < 1.3 * cam.tanfovy))
    assert unclamped.sum() > 300 and (~unclamped).sum() > 5
    for ko, kr in pairs:
        a, b = go[ko].reshape(ref[kr].shape), ref[kr]
        if kr == "means3D":
            a, b = a[unclamped], b[unclamped]
        scale = np.abs(b).max() + 1e-12
        err = np.abs(a - b).max() / scale
        assert err <= tol, (ko, err, same)


def test_scale_modifier_gradient_is_taken_at_the_modified_scale():
    """The op's dL/dscales is the derivative with respect to the MODIFIED scale modifier * s (backward.cu computeCov3D
    differentiates Sigma = (S R)^T (S R) with S = diag(modifier * s) and stops there); oracle.backward restates that.
    float64 autograd (helpers.float64_truth_gradients) differentiates with respect to s itself, so
    oracle dL/dscales = truth dL/dscales / modifier, and every other array agrees as it stands.  The float64 blend
    arbiter keeps the comparison at the float32 preprocess's rounding (2e-5, the bar of the test below)."""
    from helpers import float64_truth_gradients
    modifier = 0.6
    sc = hz.toy_scene(400, seed=12, sh_degree=1, scale=0.15)
    cam = hz.trajectory_camera(0, W=64, H=48)
    g = torch.Generator().manual_seed(22)
    H, W = cam.image_height, cam.image_width
    gc, gd, ga = torch.randn(3, H, W, generator=g), 0.1 * torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    okw = oracle_kwargs(cam, sc.sh_degree, bg=torch.tensor([0.3, 0.1, 0.6]), scale_modifier=modifier)
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, **okw)
    assert int((o["radii"] > 0).sum()) > 200
    go = oracle.backward(o, gc, gd, ga, blend_f64=True)
    truth = float64_truth_gradients(sc, okw, gc, gd, ga)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64).reshape(b.shape) - b) / np.linalg.norm(b))   # noqa: E731
    assert rel(go["dL_dscales"], truth["dL_dscales"] / modifier) <= 2e-5
    assert rel(go["dL_dscales"], truth["dL_dscales"]) > 0.3          # and not the derivative at the raw scale
    for k in ("dL_dopacity", "dL_dsh", "dL_drotations"):
        assert rel(go[k], truth[k]) <= 2e-5, k


def test_oracle_f64_arbiter_vs_fp64_autograd():
    """oracle.backward(blend_f64=True) -- gs_oracle.c gso_render_backward_f64, the arbiter of HIP-vs-oracle
    disagreements at sizes float64 autograd does not reach (tests/test_gpu_smoke_script.py) -- against that very
    autograd where it does fit: the blend stage in float64 from the exact final transmittance must reproduce the
    float64 gradient to the rounding of the float32 preprocess backward behind it (measured 6e-7 .. 2e-6
    relative L2; the float32 restatement of the reference sits at 5e-5 .. 7e-5 on this scene)."""
    sc = hz.toy_scene(700, seed=11, sh_degree=2, scale=0.12)
    cam = hz.trajectory_camera(0, W=72, H=56)
    g = torch.Generator().manual_seed(21)
    bg = torch.tensor([0.3, 0.1, 0.6])
    P, S = sc.means3D.shape[0], 2
    sem = torch.rand(P, S, generator=g)
    H, W = cam.image_height, cam.image_width
    gc, gd, ga = torch.randn(3, H, W, generator=g), 0.1 * torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    gs = torch.randn(S, H, W, generator=g)
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                       semantics=sem, **oracle_kwargs(cam, sc.sh_degree, bg=bg))
    g32 = oracle.backward(o, gc, gd, ga, gs)
    g64 = oracle.backward(o, gc, gd, ga, gs, blend_f64=True)
    ref, r = _fp64_autograd_grads(sc, cam, bg, sem, gc, gd, ga, gs)
    if not np.array_equal(o["n_contrib"].astype(np.int64), r["n_contrib"].numpy().astype(np.int64)):
        pytest.skip("float32 and float64 forwards took different accept decisions on this draw")
    m = sc.means3D.numpy()
    unclamped = ((np.abs(m[:, 0] / m[:, 2]) < 1.3 * cam.tanfovx) & (np.abs(m[:, 1] / m[:, 2]) < 1.3 * cam.tanfovy))
    for ko, kr in [("dL_dmeans3D", "means3D"), ("dL_dopacity", "opacity"), ("dL_dscales", "scales"),
                   ("dL_drotations", "rotations"), ("dL_dsh", "shs"), ("dL_dsemantic", "semantics")]:
        a64, a32, b = g64[ko].reshape(ref[kr].shape), g32[ko].reshape(ref[kr].shape), ref[kr]
        if kr == "means3D":     # the reference's knowingly inexact mean gradient of clamped Gaussians (see above)
            a64, a32, b = a64[unclamped], a32[unclamped], b[unclamped]
        n = np.linalg.norm(b) + 1e-30
        e64, e32 = np.linalg.norm(a64 - b) / n, np.linalg.norm(a32 - b) / n
        assert e64 <= 2e-5, (ko, e64)
        assert e64 <= e32 + 1e-7, (ko, e64, e32)     # never further from the truth than the float32 restatement


def test_p_zero_and_nothing_visible():
    cam = _identity_cam()
    kw = oracle_kwargs(cam, 0, bg=torch.tensor([0.5, 0.25, 0.125]))
    o = oracle.forward(np.zeros((0, 3), np.float32), np.zeros((0, 1), np.float32),
                       colors_precomp=np.zeros((0, 3), np.float32), scales=np.zeros((0, 3), np.float32),
                       rotations=np.zeros((0, 4), np.float32), **kw)
    assert o["num_rendered"] == 0 and float(np.abs(o["color"]).max()) == 0.0   # black, not bg
    behind = np.array([[0, 0, -5.0], [0.1, 0.1, 0.1]], np.float32)
    o = oracle.forward(behind, np.ones((2, 1), np.float32), colors_precomp=np.ones((2, 3), np.float32),
                       scales=np.full((2, 3), 0.1, np.float32),
                       rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (2, 1)), **kw)
    assert o["num_rendered"] == 0 and (o["radii"] == 0).all()
    np.testing.assert_allclose(o["color"][:, 3, 5], [0.5, 0.25, 0.125])
    assert float(o["alpha"].max()) == 0.0 and int(o["n_contrib"].max()) == 0


def test_higher_msb():
    # rasterizer_impl.cu:35-50: sort covers bits [0, 32+getHigherMsb(T))
    assert oracle.higher_msb(9600) == 14
    assert oracle.higher_msb(256) == 9
    assert oracle.higher_msb(1) == 1


def test_config0_at_stated_size_both_restatements_agree():
    """BASELINE configs[0] at its stated size (script/test_gaussian_rasterization.py:44-53:
    P = 10 000 uniform-random Gaussians, un-normalised quaternions, sh_degree 0, @256x256): the
    C restatement and the pure-PyTorch splat agree within 1e-5, integers exactly, and reproduce
    the counts SURVEY.md §8(d) probed on the reference's own preprocess (V = 10 000,
    R ~= 2.36 M: an overdraw stress, ~236 of 256 tiles per splat)."""
    sc, cam = hz.smoke_scene(10000, seed=0), hz.smoke_camera(256, 256)
    kw = oracle_kwargs(cam, 0)
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, **kw)
    assert int((o["radii"] > 0).sum()) == 10000
    assert o["num_rendered"] == 2359552
    with torch.no_grad():
        r = ts.rasterize(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, **kw)
    assert int(r["num_rendered"]) == o["num_rendered"]
    np.testing.assert_array_equal(np.asarray(r["radii"]), o["radii"])
    for k in ("color", "depth", "alpha"):
        a, b = np.asarray(r[k], np.float64), np.asarray(o[k], np.float64)
        assert np.abs(a - b).max() <= 1e-5 * (1.0 + np.abs(b).max()), k
        nf = o["fragile"] == 0
        assert (np.abs(a - b) <= 1e-5 * (1.0 + np.abs(b)))[..., nf].all(), k


def test_openmp_oracle_build_is_bit_identical():
    """bench.py's multi-core CPU baseline (libgs_oracle_omp.so: the same source with OpenMP over
    Gaussians and pixel rows) returns exactly what the scalar build returns."""
    sc, cam = hz.street_scene(20000, seed=3), hz.trajectory_camera(3, W=480, H=320)
    kw = oracle_kwargs(cam, 1)
    a = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, **kw)
    try:
        oracle.use_openmp(True)
        assert oracle.num_threads() >= 1
        b = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, **kw)
    finally:
        oracle.use_openmp(False)
    for k in ("color", "depth", "alpha", "n_contrib", "radii", "point_list", "ranges", "keys_sorted",
              "fragile"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # backward: pixel rows in parallel, the same fp32 terms added atomically into the fp64
    # accumulators -- only the order of the fp64 sums differs, i.e. the float32 results agree to
    # the last bit or, rarely, one ulp
    H, W = cam.image_height, cam.image_width
    g = torch.Generator().manual_seed(8)
    gc, gd, ga = torch.randn(3, H, W, generator=g), 0.1 * torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)
    ga_ = oracle.backward(a, gc, gd, ga)
    try:
        oracle.use_openmp(True)
        gb_ = oracle.backward(b, gc, gd, ga)
    finally:
        oracle.use_openmp(False)
    for k in ga_:
        np.testing.assert_allclose(gb_[k], ga_[k], rtol=3e-7, atol=0, err_msg=k)
