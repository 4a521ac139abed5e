"""CPU checks of tests/compose_truth.py, the float64 truth and the bars that tests/test_gpu_composed_backward_truth.py
holds the composed backward's raw-parameter chain rule to: the scenes reach the paths they are built for, the truth
is the plain float64 autograd gradient, an honest float32 route passes every bar with a factor 2 to spare, and every
planted error fails them where it lands.  Visibility comes from the C oracle's preprocess on the restatement's
output; the upstream g_act is random (zero where the classic op returns zero: culled rows, inactive SH bands)."""
import functools

import numpy as np
import pytest
import torch

import compose_truth as tr
import oracle
from helpers import oracle_kwargs
from oracle import compose_torch as ct

F64, F32 = torch.float64, torch.float32


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(graph, radii, g_act, groups, culled, hidden, T, Y): computed once per case, shared, never modified"""
    sg = tr.scene(case)
    with torch.no_grad():
        means, scales, rots, opac, shs = ct.compose(sg.models, tr.ct_poses(sg.poses))
    o = oracle.forward(means, opac, shs=shs, scales=scales, rotations=rots, render=False,
                       **oracle_kwargs(sg.cam, sg.active, scale_modifier=sg.scale_modifier))
    radii = torch.from_numpy(o["radii"].astype(np.int64))
    g = torch.Generator().manual_seed(77)
    vis = (radii > 0).float()
    g_act = [torch.randn(t.shape, generator=g) * vis.reshape(-1, *([1] * (t.dim() - 1))) for t in (means, scales, rots, opac, shs)]
    g_act[4][:, (sg.active + 1) ** 2:] = 0.0
    grps, culled, hidden = tr.groups(sg.models, radii)
    T = tr.vjp(sg.models, sg.poses, g_act, F64)
    Y = tr.vjp(sg.models, sg.poses, g_act, F32)
    return sg, radii, g_act, grps, culled, hidden, T, Y


def test_compose_defaults_are_unchanged_and_the_new_arguments_agree_with_them():
    sg = tr.scene("1of1")
    poses = tr.ct_poses(sg.poses)
    base = ct.compose(sg.models, poses)
    assert all(t.dtype == F32 for t in base)
    for a, b in zip(base, ct.compose(sg.models, poses, dtype=F32)):
        assert torch.equal(a, b)
    rows = [None if p is None else (torch.tensor(p[0]).repeat(m.xyz.shape[0], 1), torch.tensor(p[1]).repeat(m.xyz.shape[0], 1), p[2])
            for m, p in zip(sg.models, poses)]
    for a, b in zip(base, ct.compose(sg.models, rows)):
        assert torch.equal(a, b)
    for a, b in zip(base, ct.compose(sg.models, poses, dtype=F64)):
        assert b.dtype == F64
        torch.testing.assert_close(a.double(), b, rtol=2e-6, atol=2e-6)
    # the IDFT row is the float32 constants cast up, not recomputed: a model of one row with unit colours shows them
    k = 3
    w = ct.compose([sg.models[k]], [poses[k]], dtype=F64)[4][:, 0]
    want = (sg.models[k].features_dc.double() * ct.idft(poses[k][2], tr.FOURIER[k])[0].double()[None, :, None]).sum(1)
    torch.testing.assert_close(w, want, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_scene_reaches_the_paths_it_is_built_for(case):
    sg, radii, g_act, grps, culled, hidden, T, Y = _setup(case)
    st = tr.starts(sg.models)
    assert [m.xyz.shape[0] for m in sg.models] == list(tr.ROWS) and st[-1] == 1846
    assert [m.features_dc.shape[1] for m in sg.models] == list(tr.FOURIER)
    assert sg.models[0].features_rest.shape[1] == (sg.max_degree + 1) ** 2 - 1
    vis = [radii[st[i]:st[i + 1]] > 0 for i in range(len(sg.models))]
    # every actor but E is seen, E not at all; the background has both kinds
    assert hidden == [tr.HIDDEN] and not bool(vis[tr.HIDDEN].any())
    assert all(bool(v.any()) for i, v in enumerate(vis) if i != tr.HIDDEN)
    assert bool(vis[2].all()) and bool(vis[3].all())            # the tiny actors, every row
    assert 32 <= int(vis[0].sum()) <= 700 - 32
    # workgroup layout: the third workgroup holds rows of the background and A, the fourth of A, B, C and D
    bnd = tr.boundary_rows(sg.models)
    assert not bool(bnd[:512].any()) and bool(bnd[512:1024].all())
    assert not bool(bnd[1024:1792].any()) and bool(bnd[1792:].all())      # D: three workgroups of its own
    assert st[1] == 700 and st[2] == 1000 and st[4] == 1006 and st[5] == 1806
    assert tr.workgroups_of(sg.models) == [3, 2, 1, 1, 5, 1]
    # flips and the pose they sit under
    A, D = sg.models[1], sg.models[4]
    assert bool(A.flip.any()) and not bool(A.flip.all()) and bool(D.flip.all())
    assert abs(float(torch.tensor(sg.poses[1].obj_rot).norm()) - 1.01) < 1e-6
    flipped = int((vis[1] & A.flip).sum()) + int(vis[4].sum())
    not_flipped = int((vis[1] & ~A.flip).sum())
    boundary = int(vis[1].sum()) + int((vis[4] & bnd[st[4]:st[5]]).sum())
    assert min(flipped, not_flipped, boundary) >= tr.MIN_ROWS
    # no group the GPU test takes a bar over is thin (the merged tiny actors apart: six rows, all visible)
    names = [g.name for g in grps]
    assert len(set(names)) == len(names)
    for want in ("background/all (not flipped)", "background/boundary workgroup", "background/single-segment workgroups",
                 "A/all (mixed)", "A/flipped", "A/not flipped", "D/all (flipped)", "D/boundary workgroup",
                 "D/single-segment workgroups", "tiny actors"):
        assert want in names, want
    assert len(names) == 10
    for g in grps:
        if g.name == "tiny actors":
            assert [i for i, _ in g.members] == [2, 3] and tr.group_rows(g) == 6
        else:
            assert tr.group_rows(g) >= tr.MIN_ROWS, (g.name, tr.group_rows(g))


@pytest.mark.parametrize("case", ["1of1", "2of3"])
def test_truth_is_plain_float64_autograd_and_the_rows_sum_to_the_poses(case):
    sg, radii, g_act, grps, culled, hidden, T, Y = _setup(case)
    plain = tr.vjp(sg.models, sg.poses, g_act, F64, per_row=False)
    hand = tr.chain(sg.models, sg.poses, g_act, F64)
    for i, m in enumerate(sg.models):
        for f in tr.FIELDS:
            assert torch.equal(T["params"][i][f], plain["params"][i][f]), (i, f)
            torch.testing.assert_close(hand["params"][i][f], T["params"][i][f], rtol=1e-11, atol=1e-13, msg=lambda s, i=i, f=f: "%d %s: %s" % (i, f, s))
        if sg.poses[i] is None:
            assert T["rot"][i] is None
            continue
        n = m.xyz.shape[0]
        assert T["rows_rot"][i].shape == (n, 4) and T["rows_trans"][i].shape == (n, 3)
        for key in ("rot", "trans"):
            S = T["S_" + key][i]
            assert bool((S + 1e-300 >= T[key][i].abs()).all())
            # the sum of the rows' contributions is the pose gradient (to the rounding of n float64 additions)
            assert bool(((T[key][i] - plain[key][i]).abs() <= 1e-13 * S).all()), (i, key)
            assert bool(((hand[key][i] - T[key][i]).abs() <= 1e-11 * S).all()), (i, key)
            torch.testing.assert_close(hand["rows_" + key][i], T["rows_" + key][i], rtol=1e-10, atol=1e-12)
    # culled rows contribute nothing; the hidden actor's pose gradient is exactly zero
    for i, rows in enumerate(culled):
        for f in tr.FIELDS:
            assert not bool(T["params"][i][f][rows].any())
    assert not bool(T["rot"][tr.HIDDEN].any()) and not bool(T["trans"][tr.HIDDEN].any())


@pytest.mark.parametrize("case", list(tr.CASES))
def test_float32_routes_pass_every_bar_with_a_factor_two_to_spare(case):
    """Y (float32 autograd through the restatement) against the bars built on the other honest float32 route -- the
    hand-written chain in the kernel's order of operations -- as the yardstick, and the other way round.  No
    run-to-run term here: the bars are at their tightest."""
    sg, radii, g_act, grps, culled, hidden, T, Y = _setup(case)
    hand = tr.chain(sg.models, sg.poses, g_act, F32)
    for cand, yard in ((Y, hand), (hand, Y)):
        rep = tr.compare(cand, T, yard, None, grps, sg.models, sg.poses, sg.active)
        assert len(rep) >= 10 * 5 + 4 * 7
        tight = {k: v for k, v in rep.items() if not 2.0 * v["err"] <= v["bar"]}
        assert not tight, tight


@pytest.mark.parametrize("case", list(tr.CASES))
def test_tiny_actors_pose_gradients_are_well_conditioned_on_the_frames_own_gradients(case):
    """The scene's side of the pose bars (compose_truth.SEEDS): with the upstream gradients of THIS frame -- the C
    oracle's backward of the GPU test's loss, the CPU stand-in for the classic op -- both float32 routes put every
    pose component of the one-row and the five-row actor within 0.6 K 2^-24 S of the truth, so neither the bar's
    floor nor four times a yardstick that happened to round well is at the mercy of one cancelling sum."""
    sg = tr.scene(case)
    with torch.no_grad():
        means, scales, rots, opac, shs = ct.compose(sg.models, tr.ct_poses(sg.poses))
    o = oracle.forward(means, opac, shs=shs, scales=scales, rotations=rots,
                       **oracle_kwargs(sg.cam, sg.active, bg=torch.tensor([0.2, 0.1, 0.3]), scale_modifier=sg.scale_modifier))
    g = torch.Generator().manual_seed(3)      # the planes of tests/test_gpu_composed_backward_truth.py
    gc, gd, ga = torch.randn(3, tr.H, tr.W, generator=g), 0.1 * torch.randn(1, tr.H, tr.W, generator=g), torch.randn(1, tr.H, tr.W, generator=g)
    b = oracle.backward(o, gc, gd, ga)
    g_act = [torch.from_numpy(b[k]) for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dsh")]
    T = tr.vjp(sg.models, sg.poses, g_act, F64)
    K = tr.pose_K(sg.models)
    for X in (tr.vjp(sg.models, sg.poses, g_act, F32), tr.chain(sg.models, sg.poses, g_act, F32)):
        for i in (2, 3):
            for key in ("rot", "trans"):
                rel = (X[key][i].double() - T[key][i]).abs() / T["S_" + key][i]
                assert bool((rel <= 0.6 * K[i] * tr.EPS32).all()), (i, key, rel / (K[i] * tr.EPS32))


@pytest.mark.parametrize("case", list(tr.CASES))
def test_every_planted_error_is_rejected_where_it_lands(case):
    sg, radii, g_act, grps, culled, hidden, T, Y = _setup(case)
    clean = tr.compare(T, T, Y, None, grps, sg.models, sg.poses, sg.active)
    assert not tr.failures(clean)
    planted = tr.planted_errors(sg.models, sg.poses, g_act, T)
    assert len(planted) == 7
    expect = tr.expected_rejections(grps)   # keys every one of them must at least fail
    for name, bad in planted.items():
        rep = tr.compare(bad, T, Y, None, grps, sg.models, sg.poses, sg.active)
        failed = tr.failures(rep)
        touched = {k for k, v in rep.items() if v["err"] > 1e-12}       # (beyond the float64 rounding of chain())
        assert touched, name
        assert set(failed) == touched, (name, touched - set(failed))     # rejected wherever it lands, nowhere else
        missing = [k for k in expect[name] if k not in failed]
        assert not missing, (name, missing)
    # an error on the flipped rows leaves the groups without a flipped row alone
    rep = tr.compare(planted["flip: sign of dL/dy not mirrored"], T, Y, None, grps, sg.models, sg.poses, sg.active)
    assert rep[("A/not flipped", "xyz")]["err"] == 0.0 and rep[("background/all (not flipped)", "xyz")]["err"] == 0.0
