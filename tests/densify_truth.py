"""Float64 statement of what gaussianrpg_amd.optim.densify_and_prune computes for one model, written from the rules
(not from the kernels), with the random draws as inputs.

Per row i of P rows:
    g = accum[i, grad_column] / denom[i], NaN -> 0 (inf stays);  smax = max(exp(scaling[i]))
    clone = g >= max_grad and smax <= percent_dense * extent
    split = g >= max_grad and smax >  percent_dense * extent
Candidates: the original (slot 0), its clone (slot 1, the same values), the children c = 0, 1 of a split row (slots 2, 3)
    xyz_c = R(q / |q|) (split_noise[i, c] * exp(scaling_i)) + xyz_i,   scaling_c = log(exp(scaling_i) / 1.6)
A candidate is pruned when
    sigmoid(opacity) < min_opacity, or
    prune_big and its own smax > extent * percent_big_ws   (sphere rule: unless |xyz - centre| > 2 radius), or
    prune_big, box rule: a sample R (box_noise[i, slot, j] * exp(scaling)) + xyz, j = 0, 1, outside [box_min, box_max]
and a split original never survives.  Output rows: surviving originals, clones, children 0, children 1, each ascending
in i.  Moments follow surviving originals and are zero for new rows.

The statement also reports how far every compared quantity of every row is from its threshold, relative to the
magnitudes that enter it; build_inputs() redraws every row that comes closer than MARGIN, so that float32 and float64
agree on every decision and structure can be compared exactly, with no row exempted.
"""
import numpy as np

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic")
# per-row shapes: the reference's set at SH degree 1 with no semantic channels, and a wide set (f_rest at degree 3)
WIDTHS = {
    "deg1": {"xyz": (3,), "f_dc": (1, 3), "f_rest": (3, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,),
             "semantic": (0,)},
    "wide": {"xyz": (3,), "f_dc": (2, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,),
             "semantic": (3,)},
}
# 1e-4 is about 100 x the worst float32 evaluation error of the compared expressions (a few 1e-7 relative each)
MARGIN = 1e-4


def quat_matrix(q):
    """[n,4] (real part first) -> [n,3,3], normalised first."""
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _f64(a):
    return np.asarray(a, dtype=np.float64)


class Truth:
    """clone, split [P]; exists, pruned, survive [4,P] (slot, row); src_index, stream [n_out]; counts (dict);
    values {name: [n_out, ...]}; exp_avg / exp_avg_sq {name: [n_out, ...]} for the names given; child_xyz,
    child_scaling [2,P,3] (every row, as if split); margin [P] (see the module docstring)."""


def evaluate(params, accum, denom, split_noise, box_noise, rule, exp_avg=None, exp_avg_sq=None):
    """params: {name: [P, ...]}; rule: an object with DensifyRule's fields."""
    p = {k: _f64(v) for k, v in params.items()}
    xyz, scaling, rot = p["xyz"], p["scaling"], p["rotation"]
    op = p["opacity"].reshape(-1)
    P = xyz.shape[0]
    accum, denom = _f64(accum).reshape(P, 2), _f64(denom).reshape(P)
    split_noise = _f64(split_noise).reshape(P, 2, 3)
    has_sphere, has_box = rule.sphere_center is not None, rule.box_min is not None
    prune_big = bool(rule.prune_big)
    if has_box and prune_big:
        box_noise = _f64(box_noise).reshape(P, 4, 2, 3)
    margins = [np.full(P, np.inf)]

    def near(q, thr, scale):
        """records |q - thr| / scale per row (q: [P] or [P, ...])"""
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.abs(q - thr) / scale
        d = np.where(np.isnan(d), np.inf, d).reshape(P, -1).min(axis=1) if P else np.zeros(0)
        margins.append(d)

    with np.errstate(invalid="ignore", divide="ignore"):
        g = accum[:, rule.grad_column] / denom
    g = np.where(np.isnan(g), 0.0, g)
    near(g, rule.max_grad, rule.max_grad)
    s = np.exp(scaling)
    smax = s.max(axis=1) if P else np.zeros(0)
    dense = rule.percent_dense * rule.extent
    near(smax, dense, dense)
    sel = g >= rule.max_grad
    clone, split = sel & (smax <= dense), sel & (smax > dense)
    sig = 1.0 / (1.0 + np.exp(-op))
    near(sig, rule.min_opacity, rule.min_opacity)
    low = sig < rule.min_opacity
    R = quat_matrix(rot)

    def place(noise, scales, origin):
        """R (noise * scales) + origin, and the magnitude of the terms that enter each coordinate"""
        v = noise * scales
        out = np.einsum("nkj,nj->nk", R, v) + origin
        mag = np.einsum("nkj,nj->nk", np.abs(R), np.abs(v)) + np.abs(origin)
        return out, mag

    child_xyz = np.empty((2, P, 3))
    child_s = s / 1.6
    child_scaling = np.broadcast_to(np.log(child_s), (2, P, 3)).copy()
    for c in range(2):
        child_xyz[c], _ = place(split_noise[:, c], s, xyz)
    cand_xyz = [xyz, xyz, child_xyz[0], child_xyz[1]]
    cand_s = [s, s, child_s, child_s]
    exists = np.stack([~split, clone, split, split])
    pruned = np.zeros((4, P), dtype=bool)
    big_all = np.zeros((4, P), dtype=bool)
    big_thr = rule.extent * rule.percent_big_ws
    for slot in range(4):
        pr = low.copy()
        if prune_big:
            cmax = cand_s[slot].max(axis=1) if P else np.zeros(0)
            near(cmax, big_thr, big_thr)
            big = cmax > big_thr
            if has_sphere:
                centre = _f64(rule.sphere_center)
                diff = cand_xyz[slot] - centre
                dist = np.sqrt((diff * diff).sum(axis=1))
                near(dist, 2 * rule.sphere_radius,
                     np.maximum(2 * rule.sphere_radius, np.abs(cand_xyz[slot]).max(axis=1, initial=0) +
                                np.abs(centre).max()))
                big = big & ~(dist > 2 * rule.sphere_radius)
            big_all[slot] = big
            pr |= big
            if has_box:
                lo, hi = _f64(rule.box_min), _f64(rule.box_max)
                inside = np.ones(P, dtype=bool)
                for j in range(2):
                    pts, mag = place(box_noise[:, slot, j], cand_s[slot], cand_xyz[slot])
                    near(pts, lo, np.maximum(np.abs(lo), mag))
                    near(pts, hi, np.maximum(np.abs(hi), mag))
                    inside &= (pts >= lo).all(axis=1) & (pts <= hi).all(axis=1)
                pr |= ~inside
        pruned[slot] = pr
    survive = exists & ~pruned
    src = [np.nonzero(survive[slot])[0] for slot in range(4)]
    t = Truth()
    t.clone, t.split, t.exists, t.pruned, t.survive = clone, split, exists, pruned, survive
    t.src_index = np.concatenate(src).astype(np.int64)
    t.stream = np.concatenate([np.full(len(a), slot) for slot, a in enumerate(src)]).astype(np.int64)
    t.child_xyz, t.child_scaling = child_xyz, child_scaling
    t.values = {}
    for name, a in p.items():
        v = a[t.src_index].copy()
        for c in range(2):
            rows = t.stream == 2 + c
            if name == "xyz":
                v[rows] = child_xyz[c][t.src_index[rows]]
            elif name == "scaling":
                v[rows] = child_scaling[c][t.src_index[rows]]
        t.values[name] = v
    t.exp_avg, t.exp_avg_sq = {}, {}
    for out, moments in ((t.exp_avg, exp_avg), (t.exp_avg_sq, exp_avg_sq)):
        for name, a in (moments or {}).items():
            v = _f64(a)[t.src_index].copy()
            v[t.stream != 0] = 0.0
            out[name] = v
    t.counts = {
        "n_out": int(survive.sum()), "stream": [int(survive[slot].sum()) for slot in range(4)],
        "points_total": P, "points_clone": int(clone.sum()), "points_split": int(split.sum()),
        "points_below_min_opacity": int((exists & low).sum()), "points_big_ws": int((exists & big_all).sum()),
        "points_pruned": int((exists & pruned).sum()),
    }
    t.margin = np.min(np.stack(margins), axis=0) if P else np.zeros(0)
    return t


def default_rule_values():
    """Thresholds with the reference's defaults (config.py:57-67) and an extent that puts them inside the drawn
    scales: dense threshold 0.1, big threshold 1.0."""
    return dict(max_grad=0.0002, min_opacity=0.005, extent=10.0, percent_dense=0.01, percent_big_ws=0.1)


def _draw_rows(rng, n, widths, xyz_scale, special):
    """n rows of float32 inputs: ~20 % clone, ~20 % split, 15 % low opacity, 5 % big rows; with `special`, 3 % rows
    0 / 0 and 3 % rows accum > 0, denom = 0."""
    f = np.float32
    rows = {}
    for name, tail in widths.items():
        rows[name] = rng.standard_normal((n,) + tail).astype(f)
    rows["xyz"] = (rng.uniform(-20.0, 20.0, (n, 3)) * xyz_scale).astype(f)
    base = np.exp(rng.uniform(np.log(0.02), np.log(0.5), (n, 1)))
    big = rng.random((n, 1)) < 0.05
    base = np.where(big, np.exp(rng.uniform(np.log(1.1), np.log(3.0), (n, 1))), base)
    rows["scaling"] = np.log(base * rng.uniform(0.5, 1.0, (n, 3))).astype(f)
    low = rng.random((n, 1)) < 0.15
    rows["opacity"] = np.where(low, rng.uniform(-8.0, -5.6, (n, 1)), rng.uniform(-4.0, 4.0, (n, 1))).astype(f)
    rows["rotation"] = (rng.standard_normal((n, 4)) * rng.uniform(0.3, 3.0, (n, 1))).astype(f)
    denom = rng.integers(1, 20, (n, 1)).astype(np.float64)
    g = 0.0002 * np.exp(rng.normal(-0.3, 1.0, (n, 2)))
    accum = g * denom
    if special:
        kind = rng.random(n)
        accum[kind < 0.03] = 0.0
        denom[kind < 0.06] = 0.0
    rows["accum"], rows["denom"] = accum.astype(f), denom.astype(f)
    rows["split_noise"] = rng.standard_normal((n, 2, 3)).astype(f)
    rows["box_noise"] = rng.standard_normal((n, 4, 2, 3)).astype(f)
    return rows


def build_inputs(P, widths, rule, seed, xyz_scale=1.0, special=True):
    """Float32 inputs of one model whose every decision keeps MARGIN from its threshold under `rule` and under the
    same rule with the other grad_column.  Returns the dict of arrays (the seven tensors, accum, denom, split_noise,
    box_noise) and the number of rows that had to be redrawn."""
    import copy
    rng = np.random.default_rng(seed)
    rows = _draw_rows(rng, P, widths, xyz_scale, special)
    other = copy.copy(rule)
    other.grad_column = 1 - rule.grad_column
    redrawn = 0

    def margin():
        params = {k: rows[k] for k in GROUPS}
        m = [evaluate(params, rows["accum"], rows["denom"], rows["split_noise"], rows["box_noise"], r).margin
             for r in (rule, other)]
        return np.minimum(m[0], m[1])

    for _ in range(50):
        bad = np.nonzero(margin() < MARGIN)[0]
        if len(bad) == 0:
            break
        redrawn += len(bad)
        fresh = _draw_rows(rng, len(bad), widths, xyz_scale, special)
        for k in rows:
            rows[k][bad] = fresh[k]
    fragile = int((margin() < MARGIN).sum()) if P else 0
    assert fragile == 0, "%d rows within %g of a threshold after 50 redraws" % (fragile, MARGIN)
    return rows, redrawn


def rel_l2(a, b):
    """|a - b| / |b| over all elements, in float64; 0 when both are zero."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = float(np.linalg.norm(b))
    d = float(np.linalg.norm(a - b))
    return d / n if n > 0 else d
