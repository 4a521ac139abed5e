"""-m gpu: the composed training backward's chain rule from the activated values to the RAW parameters and the poses
(preprocess_backward_composed_kernel, pose_finish_kernel, rotation_chain_backward) against a float64 truth, group by
group (tests/compose_truth.py; its CPU side is checked in tests/test_compose_truth_host.py).

The blend is NOT part of the comparison.  Per case the classic op runs on grpg_compose's own activated tensors and is
taken backward twice (g_B, g_C: two orders of the blend's float atomics); the fused route renders the same frame --
colour, depth, alpha and radii torch.equal -- and its backward gives A.  T = vjp(g_B, float64) is the truth, Y =
vjp(g_C, float32) the yardstick: the float32 PyTorch route the kernel replaces, one atomic order away like A is.

  per group and field, relative L2 over the group's rows:   err(A, T) <= max(4 err(Y, T), 2^-20, 4 err(vjp(g_C, float64), T))
  poses, per component:     |A - T| / S <= max(4 |Y - T| / S, K 2^-24), S = sum |c_i| of the float64 per-row contributions,
                            K = 6 butterfly levels + 3 LDS adds + one global add per workgroup of the actor
  means2D:                  the same rule with run C against run B as the yardstick
  exactly zero:             every field of a culled row (every row of actor E), E's pose gradients, SH coefficients
                            above the active degree
The factor 4 is the margin the fused ops here get over a float32 yardstick (densify, sky); nothing in a bar comes from
the code under test.  A's own blend run is a THIRD atomic order, which one sample of the spread (C against B) bounds
only loosely, so the scene keeps the blend quiet -- splats of a pixel or two, none close to the camera -- and gives the
one-row and the five-row actor poses whose gradient is well conditioned (compose_truth.scene / SEEDS say why and how
much it mattered).  Every figure is printed before it is asserted and collected in bench_out/composed_backward_parity.json
(committed copy: profiles/composed_backward_parity.json).
"""
import json
import os

import pytest
import torch

import compose_truth as tr
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32


def _record(key, value):
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "composed_backward_parity.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _key(k):
    return "/".join(str(x) for x in k)


def _rel(x, t):
    x, t = x.detach().cpu().double(), t.detach().cpu().double()
    den = float(t.norm())
    assert den > 0.0
    return float((x - t).norm()) / den


@pytest.mark.parametrize("case", list(tr.CASES))
def test_composed_backward_matches_float64_truth_group_by_group(case):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussianrpg_amd.composed import ActorPose, ComposedRasterizer, ModelParams, compose
    dev = torch.device("cuda:0")
    sg = tr.scene(case)
    st = tr.starts(sg.models)
    P = st[-1]
    cam = hz.trajectory_camera(0, W=tr.W, H=tr.H, device=dev)
    rs = GaussianRasterizationSettings(**hz.settings_kwargs(cam, sg.active, bg=torch.tensor([0.2, 0.1, 0.3], device=dev),
                                                            scale_modifier=sg.scale_modifier))
    g = torch.Generator().manual_seed(3)
    gc = torch.randn(3, tr.H, tr.W, generator=g).to(dev)
    gd = (0.1 * torch.randn(1, tr.H, tr.W, generator=g)).to(dev)
    ga = torch.randn(1, tr.H, tr.W, generator=g).to(dev)

    def loss_of(color, depth, alpha):     # the test loss of tests/test_compose.py
        return (color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()

    def on_device(grad):
        return [ModelParams(*(t.to(dev).clone().requires_grad_(grad) for t in m[:6]), None if m.flip is None else m.flip.to(dev))
                for m in sg.models]

    # 1, 2: the classic op on the HIP activated tensors, backward twice
    with torch.no_grad():
        act = compose(on_device(False), sg.poses)
    act = [t.detach().clone().requires_grad_(True) for t in act]        # means3D, scales, rotations, opacity, shs
    m2c = torch.zeros(P, 3, device=dev, requires_grad=True)
    c2, r2, d2, a2, _ = GaussianRasterizer(rs)(means3D=act[0], means2D=m2c, opacities=act[3], shs=act[4], scales=act[1],
                                               rotations=act[2])
    loss = loss_of(c2, d2, a2)
    runs = []
    for _ in range(2):
        grads = torch.autograd.grad(loss, act + [m2c], retain_graph=True)
        torch.cuda.synchronize()
        runs.append([t.detach().cpu().clone() for t in grads])
    (g_B, m2_B), (g_C, m2_C) = ((r[:5], r[5]) for r in runs)

    # 3: the fused route on the same frame
    ms = on_device(True)
    ps = [None if p is None else ActorPose(torch.tensor(p.obj_rot, device=dev, requires_grad=True),
                                           torch.tensor(p.obj_trans, device=dev, requires_grad=True), p.fourier_time)
          for p in sg.poses]
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = ComposedRasterizer(rs)(ms, ps, means2D=m2d)
    assert torch.equal(radii, r2) and torch.equal(color, c2) and torch.equal(depth, d2) and torch.equal(alpha, a2)
    loss_of(color, depth, alpha).backward()
    torch.cuda.synchronize()
    A = dict(params=[{f: getattr(m, f).grad.detach().cpu() for f in tr.FIELDS} for m in ms],
             rot=[None if p is None else p.obj_rot.grad.detach().cpu() for p in ps],
             trans=[None if p is None else p.obj_trans.grad.detach().cpu() for p in ps])
    m2_A = m2d.grad.detach().cpu()

    # 4: truth, yardstick, the classic op's own spread
    T = tr.vjp(sg.models, sg.poses, g_B, F64)
    Y = tr.vjp(sg.models, sg.poses, g_C, F32)
    spread = tr.vjp(sg.models, sg.poses, g_C, F64, per_row=False)

    grps, culled, hidden = tr.groups(sg.models, radii)
    assert hidden == [tr.HIDDEN] and len(grps) == 10      # the scene of tests/test_compose_truth_host.py, nothing dropped
    for grp in grps:
        assert tr.group_rows(grp) >= (6 if grp.name == "tiny actors" else tr.MIN_ROWS), (grp.name, tr.group_rows(grp))
    report = tr.compare(A, T, Y, spread, grps, sg.models, sg.poses, sg.active)
    assert len([k for k in report if k[0] == "pose"]) == 4 * 7
    for grp in grps:      # means2D (x, y and the |.| statistic): run C against run B is the yardstick
        rows = torch.cat([st[i] + r for i, r in grp.members])
        ey = _rel(m2_C[rows], m2_B[rows])
        report[(grp.name, "means2D")] = dict(err=_rel(m2_A[rows], m2_B[rows]), yardstick=ey, spread=ey,
                                             bar=max(4.0 * ey, tr.FLOOR))
    for k, v in sorted(report.items(), key=lambda kv: _key(kv[0])):
        print("%-60s err %.3e  yardstick %.3e  spread %.3e  bar %.3e%s" % (
            _key(k), v["err"], v["yardstick"], v["spread"], v["bar"], "" if v["err"] <= v["bar"] else "   <-- MISS"))
    _record(case, {_key(k): v for k, v in report.items()})

    # the bars still tell a wrong chain rule from a right one with this frame's g_act and run-to-run spread in them
    expect = tr.expected_rejections(grps)
    for name, bad in tr.planted_errors(sg.models, sg.poses, g_B, T).items():
        rep = tr.compare(bad, T, Y, spread, grps, sg.models, sg.poses, sg.active)
        missing = [k for k in expect[name] if rep[k]["err"] <= rep[k]["bar"]]
        assert not missing, (name, missing)

    # exact zeros
    nact = (sg.active + 1) ** 2
    for i, m in enumerate(ms):
        for f in tr.FIELDS:
            assert not bool(A["params"][i][f][culled[i]].any()), (i, f)
        assert not bool(A["params"][i]["features_rest"][:, nact - 1:].any()), i
        assert not bool(m2_A[st[i] + culled[i]].any()), i
    assert culled[tr.HIDDEN].numel() == tr.ROWS[tr.HIDDEN] and culled[0].numel() >= tr.MIN_ROWS
    assert not bool(A["rot"][tr.HIDDEN].any()) and not bool(A["trans"][tr.HIDDEN].any())

    missed = tr.failures(report)
    assert not missed, {_key(k): v for k, v in missed.items()}
