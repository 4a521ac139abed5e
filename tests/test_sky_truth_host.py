"""CPU checks of tests/sky_truth.py, the float64 truth the sky cube map's backward is held to on the GPU
(tests/test_gpu_sky_backward.py): the truth against autograd and against central differences, the oracle's neighbour
table against itself, the float32 restatement of the kernel inside half of every bar, and the conditions each case of
the shared table has to meet -- so that a bad seed or view is found without a GPU."""
import math

import numpy as np
import pytest
import torch

import sky_truth as T
from oracle import sky_torch as st

SMALL = [c.name for c in T.CASES if c.H <= 61 and c.W <= 67]


def _np(t):
    return None if t is None else t.numpy()


@pytest.mark.parametrize("name", SMALL)
def test_backward64_equals_autograd(name):
    case = T.CASES[T.CASE_NAMES.index(name)]
    i, t = T.case_truth(name)
    H, W = case.H, case.W
    cube = i["cube"].double().clone().requires_grad_(True)
    acc = None if i["acc"] is None else i["acc"].double().clone().requires_grad_(True)
    rgb = torch.zeros(3, H, W, dtype=torch.float64, requires_grad=True)
    out = T.composite_torch64(cube, rgb, acc, _np(i["M"]), H, W, mask=_np(i["mask"]), jitter=_np(i["jitter"]),
                              fill=case.fill)
    ins = [cube, rgb] + ([] if acc is None else [acc])
    grads = torch.autograd.grad(out, ins, grad_outputs=i["g"].double(), allow_unused=True)
    gc = np.zeros_like(t["grad_cube"]) if grads[0] is None else grads[0].numpy()
    assert np.abs(gc - t["grad_cube"]).max() <= 1e-12 * max(np.abs(t["grad_cube"]).max(), 1e-300)
    assert torch.equal(grads[1], i["g"].double())
    if acc is not None:
        ga = grads[2].numpy().reshape(H, W)
        assert np.isfinite(ga).all()
        assert np.abs(ga - t["grad_acc"]).max() <= 1e-12 * max(np.abs(t["grad_acc"]).max(), 1e-300)


@pytest.mark.parametrize("name", [n for n in T.CASE_NAMES if "61x67" in n])
def test_composite_is_linear_in_the_cube_where_the_gate_passes(name):
    """Central differences on 20 random hit texel-channels.  The step is as large as the texel's readers allow (a
    quarter of the distance of the nearest reader's sample to a clamp bound, at most 1e-3): no gate moves inside
    the step, the composite is linear there, and the difference quotient is exact up to float64 rounding, which
    is about 2^-53 B / h for the loss over the readers -- texel-channels where that exceeds a tenth of the bar are
    passed over."""
    case = T.CASES[T.CASE_NAMES.index(name)]
    i, t = T.case_truth(name)
    N = case.H * case.W
    idx, w = t["idx"], t["w"]
    fetch = t["fetch"].reshape(N)
    g = _np(i["g"]).astype(np.float64).reshape(3, N).T
    tr = np.ones(N) if i["acc"] is None else 1.0 - _np(i["acc"]).astype(np.float64).reshape(N)
    s = t["s"].reshape(3, N).T
    texels = _np(i["cube"]).astype(np.float64).reshape(-1, 3)
    A, B = t["A"].reshape(-1, 3), t["B"].reshape(-1, 3)
    rng = np.random.default_rng(5)
    hit = np.argwhere(t["n"].reshape(-1, 3) > 0)
    done = 0
    for tex, c in hit[rng.permutation(len(hit))]:
        rows = np.nonzero(fetch & (idx == tex).any(axis=1))[0]
        h = min(1e-3, 0.25 * float(np.minimum(np.abs(s[rows, c]), np.abs(s[rows, c] - 1.0)).min()))
        if 2.0 ** -53 * B[tex, c] / max(h, 1e-300) > 1e-10 * A[tex, c]:
            continue

        def loss(delta):
            v = np.where(idx[rows] >= 0, texels[np.maximum(idx[rows], 0), c] + delta * (idx[rows] == tex), 0.0)
            return math.fsum(tr[rows] * g[rows, c] * np.clip((w[rows] * v).sum(axis=1), 0.0, 1.0))
        fd = (loss(h) - loss(-h)) / (2 * h)
        want = t["grad_cube"].reshape(-1, 3)[tex, c]
        assert abs(fd - want) <= 1e-9 * A[tex, c], (tex, c, fd, want, h)
        done += 1
        if done == 20:
            break
    assert done == min(20, len(hit)), (done, len(hit))


@pytest.mark.parametrize("res", [1, 2, 3, 16])
def test_neighbour_relation_is_symmetric(res):
    """Every edge step (f, iu, iv) -> (g, ju, jv): stepping back out of (g, ju, jv) across the shared edge lands on
    the boundary texel the step came from, and across no other edge of g does."""
    adj = st._edge_table(res)
    for f in range(6):
        for side in range(4):
            for k in range(res):
                bu, bv = ((0, k), (res - 1, k), (k, 0), (k, res - 1))[side]
                g, ju, jv = (int(x) for x in adj[f, side, k])
                assert g != f and 0 <= ju < res and 0 <= jv < res
                back = []
                if ju == 0:
                    back.append(adj[g, 0, jv])
                if ju == res - 1:
                    back.append(adj[g, 1, jv])
                if jv == 0:
                    back.append(adj[g, 2, ju])
                if jv == res - 1:
                    back.append(adj[g, 3, ju])
                assert sum(tuple(int(x) for x in b) == (f, bu, bv) for b in back) == 1, (f, side, k, g, ju, jv)


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_case_meets_its_conditions_and_float32_stays_inside_half_the_bars(name):
    case = T.CASES[T.CASE_NAMES.index(name)]
    i, t = T.case_truth(name)
    T.check_case_conditions(case, t)
    # every tap row's weights sum to 1, dropped taps carry none
    assert np.abs(t["w"].sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -53
    assert (t["w"][t["idx"] < 0] == 0.0).all() and (t["w"] >= 0.0).all()
    # texture_cube is the same lookup
    d = T.rays64(_np(i["M"]), case.H, case.W, _np(i["jitter"]))
    direct = st.texture_cube(_np(i["cube"]), d)
    fetch = t["fetch"].reshape(-1)
    assert np.abs(direct - t["s"].reshape(3, -1).T)[fetch].max(initial=0.0) <= 1e-14
    # float32 alone: weights (matched by texel id) within half the allowance, gradients within half the bars
    e = T.backward32(_np(i["cube"]), _np(i["M"]), case.H, case.W, _np(i["g"]), acc=_np(i["acc"]), mask=_np(i["mask"]),
                     jitter=_np(i["jitter"]), fill=case.fill)
    werr = T.max_weight_error(t["idx"], t["w"], e["idx"], e["w"], fetch)
    assert werr <= 0.5 * t["dw"], (werr / t["dw"])
    rc, zeros_ok = T.cube_ratio(e["grad_cube"], t)
    ra = T.acc_ratio(e["grad_acc"], t)
    assert zeros_ok and rc <= 0.5 and ra <= 0.5, (rc, ra, zeros_ok)


def test_table_covers_what_it_has_to():
    cs = T.CASES
    assert {c.res for c in cs} == {1, 2, 3, 16, 64}
    assert {(c.H, c.W) for c in cs} == {(1, 1), (5, 7), (4, 64), (61, 67), (72, 120), (130, 257)}
    assert {c.view for c in cs} == {"face", "corner", "wide"}
    assert {c.mode for c in cs} == {"composite", "lookup", "mask_jitter", "acc_jitter", "acc_edge"}
    assert {c.fill for c in cs} == {0.0, 1.0} and {c.mdev for c in cs} == {False, True}
    assert len(set(T.CASE_NAMES)) == len(cs)
    for res in (1, 2, 3, 16, 64):                 # every resolution looks along a corner, wide, and at a face
        assert {c.view for c in cs if c.res == res} == {"face", "corner", "wide"}
    assert all(0.2 <= c.focal <= 0.3 for c in cs if c.view == "wide")
    assert max(len(T.case_truth(c.name)[1]["faces"]) for c in cs if c.view == "wide") >= 5
    # the acc rule's edge rows: only acc 0 fetches, and the gradient there is -fill * sum g, finite
    for c in cs:
        if c.mode != "acc_edge":
            continue
        i, t = T.case_truth(c.name)
        acc = i["acc"][0].numpy()
        for row, v in zip((3, 5, 7, 9), T.ACC_EDGE_VALUES):
            assert (acc[row] == np.float32(v)).all() and t["fetch"][row].all() == (v == 0.0)
            assert t["fetch"][row].any() == (v == 0.0)
        nan = np.isnan(acc)
        assert nan.sum() >= 10 and not t["fetch"][nan].any() and np.isfinite(t["grad_acc"]).all()
        off = ~t["fetch"]
        gsum = i["g"].double().numpy().sum(axis=0)
        assert np.array_equal(t["grad_acc"][off], -c.fill * gsum[off])


def test_rays64_agree_with_the_pinned_get_rays_to_float32_rounding():
    from test_sky import _camera
    from gaussianrpg_amd.sky import ray_matrix
    H, W = 61, 67
    K, w2c = _camera(W, H, 0.9, -0.4, 0.3)
    jit = torch.rand(2, H, W, generator=torch.Generator().manual_seed(2))
    for j in (None, jit):
        _, rd = st.get_rays(H, W, K, w2c[:3, :3], w2c[:3, 3], jitter=j)
        d = T.rays64(ray_matrix(K, w2c).numpy(), H, W, _np(j))
        assert np.abs(d - rd.double().numpy().reshape(-1, 3)).max() < 2e-6
        assert np.abs(T.rays32(ray_matrix(K, w2c).numpy(), H, W, _np(j)).astype(np.float64) - d).max() < 4 * 2.0 ** -24
