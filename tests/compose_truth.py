"""Float64 truth of the composed backward's LAST step -- TEST INFRASTRUCTURE (CPU only, no GPU needed).

The fused training route (gaussianrpg_amd/composed.py, csrc/preprocess_bwd.hip: preprocess_backward_composed_kernel,
pose_finish_kernel; csrc/compose_math.h: rotation_chain_backward) ends by taking the per-Gaussian gradients of the
ACTIVATED values -- g_act = (dL/dmeans3D, dL/dscales, dL/drotations, dL/dopacity, dL/dshs), what the classic op
returns -- down to every model's raw parameters and to the actors' poses.  This module states that step alone:

  scene(case)       the small scene graphs of CASES: a workgroup across a model boundary, workgroups holding
                    several tiny actors, an actor with every row culled, M = 1 / 4 / 16, an active SH degree below
                    the maximum, fourier_dim 1 .. MAX_FOURIER, flipped rows under a non-unit obj_rot, a scale modifier
  groups(...)       the row sets the bars are taken over: visible / culled, flipped / not flipped, rows of a
                    workgroup owned by one segment / of a workgroup across a boundary
  vjp(...)          autograd through oracle/compose_torch.compose in a dtype: float64 = the truth T (with per-row
                    poses: every row's contribution c_i to the pose gradients, and S = sum |c_i|), float32 = the
                    yardstick Y (the PyTorch route the fused kernel replaces)
  chain(...)        the same chain rule written out by hand in the kernel's order of operations (any dtype): an
                    independent route to T, a float32 stand-in for the kernel on the CPU, and the place where the
                    planted errors that autograd cannot express are made
  planted_errors()  corrupted copies of T
  compare(...)      the bars of tests/test_gpu_composed_backward_truth.py; nothing in them comes from the code under test
"""
import math
from typing import NamedTuple

import torch

from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.composed import MAX_FOURIER, ActorPose, ModelParams
from oracle import compose_torch as ct

FIELDS = ModelParams._fields[:6]
W, H = 160, 96
WG = 256                 # rows per workgroup of preprocess_backward_composed_kernel
MIN_ROWS = 32            # visible rows a group needs (the merged tiny actors apart)
FLOOR = 2.0 ** -20       # a few float32 roundings, for paths on which the yardstick is exact
EPS32 = 2.0 ** -24

# name -> (active SH degree, maximum SH degree, scale_modifier)
CASES = {"0of0": (0, 0, 1.0), "1of1": (1, 1, 1.0), "0of1": (0, 1, 1.0), "2of3": (2, 3, 1.0), "3of3": (3, 3, 1.0),
         "1of1-modifier0.6": (1, 1, 0.6)}
# model: rows, fourier_dim.  700 = 2 * 256 + 188: the third workgroup is shared with actor A; A, B, C and the head of D
# share the fourth; D then owns three workgroups and shares its last with E.
NAMES = ("background", "A", "B", "C", "D", "E")
ROWS = (700, 300, 1, 5, 800, 40)
FOURIER = (1, 5, 1, MAX_FOURIER, 3, 2)
HIDDEN = 5               # actor E stands behind the camera


class Graph(NamedTuple):
    models: list
    poses: list
    active: int
    max_degree: int
    scale_modifier: float
    cam: object


# One generator per model: the geometry is the same in every case.  B's and C's seeds are CHOSEN: with one row S is
# |c_i| itself, and a component of dL/d obj_rot that the two paths (through R and through the Hamilton product) nearly
# cancel in carries the float32 rounding of the larger terms -- over 16 seeds the float32 PyTorch routes sat between
# 0.3 and 1200 times K 2^-24 from the truth.  These two keep both routes within 0.6 K 2^-24 on the frame's own
# upstream gradients (tests/test_compose_truth_host.py asserts it on the C oracle's backward), so the pose bars of
# the tiny actors measure the kernel's sum and not one unlucky rounding.
SEEDS = (2024, 2025, 112, 162, 2028, 2029)


def scene(case):
    active, max_degree, modifier = CASES[case]
    M = (max_degree + 1) ** 2
    models, poses = [], []
    # actor boxes (full extents) and where they stand; the camera looks down +z from the origin
    box = {1: (1.5, 0.8, 1.0), 2: (0.1, 0.1, 0.1), 3: (0.4, 0.3, 0.3), 4: (2.0, 1.0, 1.5), 5: (1.0, 1.0, 1.0)}
    trans = {1: (-0.8, 0.1, 5.0), 2: (0.8, -0.5, 4.0), 3: (1.2, 0.5, 5.0), 4: (0.5, 0.2, 8.0), 5: (0.0, 0.0, -5.0)}
    # Splats of a pixel or two: the blend is not what this scene is for.  The loss planes are random, so a splat's
    # upstream gradient is a cancelling sum over its pixels, and the order of the blend's float atomics moves it by
    # about 2^-24 sqrt(pixels) -- with splats of hundreds of pixels (and a few close ones covering the frame) the
    # run-to-run spread of g_act, 1e-6 of a group's norm in one run and 1e-7 in the next, decided the comparison
    # instead of the chain rule.
    for k, (n, F) in enumerate(zip(ROWS, FOURIER)):
        g = torch.Generator().manual_seed(SEEDS[k])
        if k == 0:
            # a cloud wider than the view, one row in eight mirrored behind the camera: visible and culled rows
            xyz = torch.randn(n, 3, generator=g) * torch.tensor([4.0, 2.0, 1.5]) + torch.tensor([0.0, 0.0, 7.0])
            xyz[:, 2] = torch.where(torch.rand(n, generator=g) < 0.125, -xyz[:, 2], xyz[:, 2].clamp_min(2.5))
            scaling = math.log(0.03) + 0.3 * torch.randn(n, 3, generator=g)
        else:
            xyz = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor(box[k])
            scaling = math.log(0.02) + 0.3 * torch.randn(n, 3, generator=g)
        rotation = torch.randn(n, 4, generator=g) * (0.5 + torch.rand(n, 1, generator=g))
        opacity = 1.0 + 2.0 * torch.randn(n, 1, generator=g)
        flip = None
        if k == 1:
            flip = torch.rand(n, generator=g) < 0.5
        elif k == 4:
            flip = torch.ones(n, dtype=torch.bool)
        q = torch.randn(4, generator=g)
        q = q / q.norm() * (1.0 + 0.01 * k)      # ||obj_rot|| = 1.01 for A: tracked poses are not exactly unit
        fdc = 0.5 * torch.randn(n, F, 3, generator=g)
        frest = 0.15 * torch.randn(n, M - 1, 3, generator=g)
        models.append(ModelParams(xyz, scaling, rotation, opacity, fdc, frest, flip))
        poses.append(None if k == 0 else ActorPose(q.tolist(), list(trans[k]), 0.15 + 0.2 * k))
    return Graph(models, poses, active, max_degree, modifier, hz.trajectory_camera(0, W=W, H=H))


def ct_poses(poses):
    return [None if p is None else (p.obj_rot, p.obj_trans, p.fourier_time) for p in poses]


def starts(models):
    out, s = [], 0
    for m in models:
        out.append(s)
        s += m.xyz.shape[0]
    return out + [s]


def boundary_rows(models):
    """bool [P]: the row lies in a workgroup (rows 256 k .. 256 k + 255 of the concatenated index) that holds rows of
    more than one model -- the kernel's `uniform` test, negated."""
    st = starts(models)
    P = st[-1]
    seg = torch.zeros(P, dtype=torch.long)
    for i in range(len(models)):
        seg[st[i]:st[i + 1]] = i
    out = torch.zeros(P, dtype=torch.bool)
    for b in range(0, P, WG):
        e = min(b + WG, P)
        out[b:e] = seg[b] != seg[e - 1]
    return out


def workgroups_of(models):
    """per model: how many workgroups hold some of its rows"""
    st = starts(models)
    return [(st[i + 1] - 1) // WG - st[i] // WG + 1 for i in range(len(models))]


class Group(NamedTuple):
    name: str
    members: tuple      # ((model index, LongTensor of the model's own row numbers), ...)


def groups(models, radii):
    """-> (groups, culled, hidden).  groups: the visible rows of every model that has any, split -- where the model has
    rows on both sides -- into flipped / not flipped and into rows of single-segment workgroups / of workgroups across a
    boundary, plus the model's visible rows as a whole; models too small for a group of their own (fewer than MIN_ROWS
    rows: the tiny actors) are merged into one.  culled: per model the rows with radius 0.  hidden: the models without
    a single visible row."""
    radii = torch.as_tensor(radii).cpu()
    st = starts(models)
    bnd = boundary_rows(models)
    out, culled, hidden, tiny = [], [], [], []
    for i, m in enumerate(models):
        n = m.xyz.shape[0]
        vis = radii[st[i]:st[i + 1]] > 0
        culled.append(torch.nonzero(~vis).flatten())
        if not bool(vis.any()):
            hidden.append(i)
            continue
        if n < MIN_ROWS:
            tiny.append((i, torch.nonzero(vis).flatten()))
            continue
        name = NAMES[i] if len(models) == len(NAMES) else "model%d" % i
        flip = m.flip if m.flip is not None else torch.zeros(n, dtype=torch.bool)
        b = bnd[st[i]:st[i + 1]]
        tag = ("flipped" if bool(flip.all()) else "not flipped" if not bool(flip.any()) else "mixed")
        out.append(Group("%s/all (%s)" % (name, tag), ((i, torch.nonzero(vis).flatten()),)))
        for mask, yes, no in ((flip, "flipped", "not flipped"), (b, "boundary workgroup", "single-segment workgroups")):
            if bool(mask.any()) and not bool(mask.all()):
                out.append(Group("%s/%s" % (name, yes), ((i, torch.nonzero(vis & mask).flatten()),)))
                out.append(Group("%s/%s" % (name, no), ((i, torch.nonzero(vis & ~mask).flatten()),)))
    if tiny:
        out.append(Group("tiny actors", tuple(tiny)))
    return out, culled, hidden


def group_rows(g):
    return sum(int(r.numel()) for _, r in g.members)


def _qmul(a, b):
    return ct.quaternion_raw_multiply(a, b)


def vjp(models, poses, g_act, dtype, per_row=None):
    """Gradients of the raw parameters and the poses from the upstream g_act = (dL/dmeans3D, dL/dscales, dL/drotations,
    dL/dopacity, dL/dshs) by autograd through ct.compose in `dtype`.  -> dict: params (per model: field -> tensor), rot /
    trans (per model: None or the pose gradient); with per_row (default: in float64) each actor's pose enters once per
    row, so that rows_rot / rows_trans hold every row's contribution c_i, rot / trans their sums and S_rot / S_trans
    sum |c_i|."""
    if per_row is None:
        per_row = dtype == torch.float64
    leaves, ms, ps = [], [], []
    for m, p in zip(models, poses):
        n = m.xyz.shape[0]
        lv = [m[f].detach().cpu().to(dtype).requires_grad_(True) for f in range(6)]
        leaves.append(lv)
        ms.append(ModelParams(*lv, None if m.flip is None else m.flip.cpu()))
        if p is None:
            ps.append(None)
            continue
        rot = torch.as_tensor(p.obj_rot).detach().cpu().to(dtype).reshape(1, 4)
        tr = torch.as_tensor(p.obj_trans).detach().cpu().to(dtype).reshape(1, 3)
        rot, tr = (rot.repeat(n, 1), tr.repeat(n, 1)) if per_row else (rot.reshape(4), tr.reshape(3))
        ps.append((rot.requires_grad_(True), tr.requires_grad_(True), p.fourier_time))
    out = ct.compose(ms, ps, dtype=dtype)
    flat = [t for lv in leaves for t in lv] + [t for p in ps if p is not None for t in p[:2]]
    grads = list(torch.autograd.grad(out, flat, [g.detach().cpu().to(dtype).reshape(o.shape) for g, o in zip(g_act, out)],
                                     allow_unused=True))
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, flat)]
    res = dict(params=[], rot=[], trans=[], rows_rot=[], rows_trans=[], S_rot=[], S_trans=[])
    for i in range(len(models)):
        res["params"].append(dict(zip(FIELDS, grads[6 * i:6 * i + 6])))
    k = 6 * len(models)
    for p in poses:
        if p is None:
            for key in ("rot", "trans", "rows_rot", "rows_trans", "S_rot", "S_trans"):
                res[key].append(None)
            continue
        gr, gt = grads[k], grads[k + 1]
        k += 2
        if per_row:
            res["rows_rot"].append(gr); res["rows_trans"].append(gt)
            res["rot"].append(gr.sum(0)); res["trans"].append(gt.sum(0))
            res["S_rot"].append(gr.abs().sum(0)); res["S_trans"].append(gt.abs().sum(0))
        else:
            res["rot"].append(gr); res["trans"].append(gt)
            for key in ("rows_rot", "rows_trans", "S_rot", "S_trans"):
                res[key].append(None)
    return res


def chain(models, poses, g_act, dtype, world_projection=True):
    """The same gradients by the chain rule written out, in the order of composed_backward_one / rotation_chain_backward /
    pose_finish_kernel (one model at a time, every row at once; the pose sums are plain sums over the rows).  Beside
    vjp()'s keys: gn (per model, dL/d of the normalised local quaternion BEFORE the projection of the raw rotation's
    normalisation -- the quantity autograd never shows) and rows_rot_product (the Hamilton-product share of rows_rot).
    world_projection=False leaves out the projection at an actor's q = p / |p| (a planted error)."""
    gm_, gs_, gq_, go_, gsh_ = [g.detach().cpu().to(dtype) for g in g_act]
    go_ = go_.reshape(-1, 1)
    st = starts(models)
    res = dict(params=[], rot=[], trans=[], rows_rot=[], rows_trans=[], S_rot=[], S_trans=[], gn=[], rows_rot_product=[])
    dot = lambda a, b: (a * b).sum(1, keepdim=True)   # noqa: E731
    for i, (m, p) in enumerate(zip(models, poses)):
        n = m.xyz.shape[0]
        sl = slice(st[i], st[i + 1])
        gm, gs, gq, go, gsh = gm_[sl], gs_[sl], gq_[sl], go_[sl], gsh_[sl]
        c = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
        r = c(m.rotation)
        rn = r.norm(dim=1, keepdim=True).clamp_min(1e-12)
        qn = r / rn
        flip = torch.zeros(n, dtype=torch.bool) if (m.flip is None or p is None) else m.flip.cpu()
        f = flip[:, None]
        ql = torch.where(f, torch.stack((-qn[:, 2], qn[:, 3], qn[:, 0], -qn[:, 1]), 1), qn)
        o = torch.sigmoid(c(m.opacity)).reshape(n, 1)
        out = dict(scaling=gs * torch.exp(c(m.scaling)), opacity=(go * (o * (1 - o))).reshape(m.opacity.shape))
        if p is None:
            gql, out["xyz"] = gq, gm
            w = torch.ones(1, dtype=dtype)
            rows_rot = rows_trans = prod = None
        else:
            a = torch.as_tensor(p.obj_rot).detach().cpu().to(dtype).reshape(1, 4)
            pq = _qmul(a.expand(n, 4), ql)
            pn = pq.norm(dim=1, keepdim=True).clamp_min(1e-12)
            q = pq / pn
            g = (gq - q * dot(q, gq)) / pn if world_projection else gq / pn
            aw, ax, ay, az = a[0]
            gw, gx, gy, gz = g.unbind(1)
            gql = torch.stack((aw * gw + ax * gx + ay * gy + az * gz, -ax * gw + aw * gx + az * gy - ay * gz,
                               -ay * gw - az * gx + aw * gy + ax * gz, -az * gw + ay * gx - ax * gy + aw * gz), 1)
            lw, lx, ly, lz = ql.unbind(1)
            prod = torch.stack((lw * gw + lx * gx + ly * gy + lz * gz, -lx * gw + lw * gx - lz * gy + ly * gz,
                                -ly * gw + lz * gx + lw * gy - lx * gz, -lz * gw - ly * gx + lx * gy + lw * gz), 1)
            on = a.norm()
            u = a / on
            R = ct.quaternion_to_matrix(u)[0]
            x = c(m.xyz) * torch.where(f, torch.tensor([1.0, -1.0, 1.0], dtype=dtype), torch.ones(3, dtype=dtype))
            gl = gm @ R                                  # R^T g per row
            out["xyz"] = gl * torch.where(f, torch.tensor([1.0, -1.0, 1.0], dtype=dtype), torch.ones(3, dtype=dtype))
            G = gm[:, :, None] * x[:, None, :]           # per row dL/dR = g x^T
            rr, ux, uy, uz = u[0]
            G00, G01, G02, G10, G11, G12, G20, G21, G22 = (G[:, a_, b_] for a_ in range(3) for b_ in range(3))
            g_r = 2 * (-uz * G01 + uy * G02 + uz * G10 - ux * G12 - uy * G20 + ux * G21)
            g_x = 2 * (uy * G01 + uz * G02 + uy * G10 - 2 * ux * G11 - rr * G12 + uz * G20 + rr * G21 - 2 * ux * G22)
            g_y = 2 * (-2 * uy * G00 + ux * G01 + rr * G02 + ux * G10 + uz * G12 - rr * G20 + uz * G21 - 2 * uy * G22)
            g_z = 2 * (-2 * uz * G00 - rr * G01 + ux * G02 + rr * G10 - 2 * uz * G11 + uy * G12 + ux * G20 + uy * G21)
            gu = torch.stack((g_r, g_x, g_y, g_z), 1)
            rows_rot = (gu - u * dot(u.expand(n, 4), gu)) / on + prod
            rows_trans = gm
            w = c(ct.idft(p.fourier_time, m.features_dc.shape[1])[0])
        gn = torch.where(f, torch.stack((gql[:, 2], -gql[:, 3], -gql[:, 0], gql[:, 1]), 1), gql)
        out["rotation"] = (gn - qn * dot(qn, gn)) / rn
        out["features_dc"] = gsh[:, 0:1, :] * w[None, :, None]
        out["features_rest"] = gsh[:, 1:, :]
        res["params"].append(out)
        res["gn"].append(gn)
        res["rows_rot_product"].append(prod)
        res["rows_rot"].append(rows_rot); res["rows_trans"].append(rows_trans)
        res["rot"].append(None if p is None else rows_rot.sum(0))
        res["trans"].append(None if p is None else rows_trans.sum(0))
        res["S_rot"].append(None if p is None else rows_rot.abs().sum(0))
        res["S_trans"].append(None if p is None else rows_trans.abs().sum(0))
    return res


def _copy(T):
    return dict(params=[{k: v.clone() for k, v in d.items()} for d in T["params"]],
                rot=[None if t is None else t.clone() for t in T["rot"]],
                trans=[None if t is None else t.clone() for t in T["trans"]])


def planted_errors(models, poses, g_act, T):
    """name -> a copy of the float64 truth T (vjp(..., torch.float64), per-row poses) with one mistake of the kind the
    kernel could make.  Each is what the WHOLE route would return had that one line been wrong, in the arrays it
    reaches (the raw-parameter array or the pose gradient named)."""
    st = starts(models)
    C = chain(models, poses, g_act, torch.float64)
    g64 = [g.detach().cpu().double() for g in g_act]
    out = {}
    # (1) dL/dy of a flipped row not mirrored back (go.xyz[3 j + 1] without its sign)
    e = _copy(T)
    for i, (m, p) in enumerate(zip(models, poses)):
        if m.flip is not None and p is not None:
            e["params"][i]["xyz"][m.flip.cpu(), 1] *= -1
    out["flip: sign of dL/dy not mirrored"] = e
    # (2) the raw rotation's normalisation without its projection: gn / |r| instead of (gn - q (q . gn)) / |r|.  Seen on
    # static models only: under a pose gn comes through q = p / |p|, p = a (x) ql, and is orthogonal to ql already
    # (gn . ql = g . p = 0), so there the projection changes nothing but the rounding
    e = _copy(T)
    for i, m in enumerate(models):
        rn = m.rotation.detach().cpu().double().norm(dim=1, keepdim=True)
        e["params"][i]["rotation"] = C["gn"][i] / rn
    out["rotation: projection - q (q . g) dropped"] = e
    # (2b) the same mistake at an actor's q = p / |p|: its _rotation is still right (the stray radial part maps onto ql
    # and the raw normalisation's projection removes it -- either projection alone would do), dL/d obj_rot is not
    e = _copy(T)
    W = chain(models, poses, g_act, torch.float64, world_projection=False)
    for i, p in enumerate(poses):
        if p is not None:
            e["params"][i]["rotation"] = W["params"][i]["rotation"]
            e["rot"][i] = W["rot"][i]
    out["actor rotation: projection at q = p / |p| dropped"] = e
    # (3) pose_acc[12..15], the Hamilton-product share of dL/d obj_rot, not added
    e = _copy(T)
    for i, p in enumerate(poses):
        if p is not None:
            e["rot"][i] = T["rot"][i] - C["rows_rot_product"][i].sum(0)
    out["obj_rot: product path dropped"] = e
    # (4) dL/d_features_dc[c] = dL/dsh_0 for every c, without the IDFT weight
    e = _copy(T)
    for i, m in enumerate(models):
        F = m.features_dc.shape[1]
        e["params"][i]["features_dc"] = g64[4][st[i]:st[i + 1], 0:1, :].expand(-1, F, -1).clone()
    out["features_dc: IDFT weight dropped"] = e
    # (5) dL/d_scaling = dL/ds, without exp(r)
    e = _copy(T)
    for i in range(len(models)):
        e["params"][i]["scaling"] = g64[1][st[i]:st[i + 1]].clone()
    out["scaling: factor exp(r) dropped"] = e
    # (6) a workgroup across a boundary adds all its lanes' pose sums to the segment of its FIRST row
    e = _copy(T)
    bnd = boundary_rows(models)
    seg_of = torch.zeros(st[-1], dtype=torch.long)
    for i in range(len(models)):
        seg_of[st[i]:st[i + 1]] = i
    for i, p in enumerate(poses):
        if p is None:
            continue
        for key, rows in (("rot", T["rows_rot"][i]), ("trans", T["rows_trans"][i])):
            for j in torch.nonzero(bnd[st[i]:st[i + 1]]).flatten().tolist():
                first = int(seg_of[((st[i] + j) // WG) * WG])
                if first == i:
                    continue
                e[key][i] = e[key][i] - rows[j]
                if poses[first] is not None:
                    e[key][first] = e[key][first] + rows[j]
    out["boundary workgroup: pose sums credited to the neighbour"] = e
    return out


def expected_rejections(grps):
    """planted error -> keys of compare() that must at least fail for it (scene of CASES)"""
    poses = [("pose", i, k, c) for i in (1, 2, 3, 4) for k, n in (("rot", 4), ("trans", 3)) for c in range(n)]
    return {
        "flip: sign of dL/dy not mirrored": [("A/flipped", "xyz"), ("A/all (mixed)", "xyz"), ("D/all (flipped)", "xyz"),
                                             ("D/boundary workgroup", "xyz"), ("D/single-segment workgroups", "xyz")],
        "rotation: projection - q (q . g) dropped": [(g.name, "rotation") for g in grps if g.name.startswith("background")],
        "actor rotation: projection at q = p / |p| dropped": [k for k in poses if k[2] == "rot"],
        "obj_rot: product path dropped": [k for k in poses if k[2] == "rot"],
        "features_dc: IDFT weight dropped": [(n, "features_dc") for n in ("A/all (mixed)", "D/all (flipped)", "tiny actors")],
        "scaling: factor exp(r) dropped": [(g.name, "scaling") for g in grps],
        "boundary workgroup: pose sums credited to the neighbour": poses,
    }


def _active_rest(t, active):
    return t[:, :(active + 1) ** 2 - 1]


def group_error(X, T, group, field, active):
    """relative L2 of X against T over the group's rows of one field (features_rest: the active coefficients)"""
    num = den = 0.0
    for i, rows in group.members:
        x, t = X["params"][i][field].detach().cpu().double(), T["params"][i][field].double()
        if field == "features_rest":
            x, t = _active_rest(x, active), _active_rest(t, active)
        num += float(((x[rows] - t[rows]) ** 2).sum())
        den += float((t[rows] ** 2).sum())
    assert den > 0.0, "the truth is all zero on %s / %s: the scene does not exercise it" % (group.name, field)
    return math.sqrt(num / den)


def pose_K(models):
    """float32 additions on the longest path of the kernel's pose sum: 6 butterfly levels, 3 LDS adds, and one global add
    per workgroup that holds rows of the actor"""
    return [9 + w for w in workgroups_of(models)]


def compare(cand, T, Y, spread, grps, models, poses, active):
    """The bars.  cand: the gradients under test; T: the float64 truth with per-row poses; Y: the float32 yardstick;
    spread: None or the truth's own route fed with ANOTHER run's g_act (the classic op's run-to-run spread).
    -> {key: dict(err, yardstick, spread, bar)}; a key passes when err <= bar.
      (group, field):                  err = relative L2 over the group's rows, bar = max(4 err(Y), FLOOR, 4 err(spread))
      ("pose", model, "rot"|"trans", component):   err = |cand - T| / S,  bar = max(4 |Y - T| / S, K 2^-24)"""
    out = {}
    for g in grps:
        for field in FIELDS:
            if field == "features_rest" and (active == 0 or T["params"][0][field].shape[1] == 0):
                continue    # no active coefficient beyond the DC one: the exact-zero check covers the rest
            ey = group_error(Y, T, g, field, active)
            es = 0.0 if spread is None else group_error(spread, T, g, field, active)
            out[(g.name, field)] = dict(err=group_error(cand, T, g, field, active), yardstick=ey, spread=es,
                                        bar=max(4.0 * ey, FLOOR, 4.0 * es))
    K = pose_K(models)
    for i, p in enumerate(poses):
        if p is None or T["S_rot"][i] is None or float(T["S_rot"][i].max()) == 0.0:
            continue
        for key, n in (("rot", 4), ("trans", 3)):
            S = T["S_" + key][i]
            for c in range(n):
                assert float(S[c]) > 0.0
                d = lambda X: abs(float(X[key][i].detach().cpu().double().reshape(-1)[c]) - float(T[key][i][c])) / float(S[c])   # noqa: E731
                out[("pose", i, key, c)] = dict(err=d(cand), yardstick=d(Y), spread=0.0 if spread is None else d(spread),
                                                bar=max(4.0 * d(Y), K[i] * EPS32))
    return out


def failures(report):
    return {k: v for k, v in report.items() if not v["err"] <= v["bar"]}
