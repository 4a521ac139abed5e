"""float64 restatement of the detector head -> prediction -> detections contract of
gaussianrpg_amd.perception.decode_heads / detections_from_heads (csrc/nms.hip), the input builders of its tests and
of tests/golden/ref_detect.* (tests/golden/make_golden_detect.py records what the reference's own ``Detect.forward``
and ``non_max_suppression`` returned for them), and the comparator.

The decode is written from the text of the inference branch of the reference's ``Detect.forward``
(models/yolo.py:53-70): per level ``view(bs, na, no, ny, nx).permute(0, 1, 3, 4, 2)``, a sigmoid,
``xy = (s*2 - 0.5 + grid) * stride``, ``wh = (s*2)**2 * anchor_grid``, and ``cat`` over the levels.  The float32
logits are taken as exact and everything after them is float64: this is the truth both the reference's float32 result
and the kernel's are measured against.  torch.sigmoid is not pinned bit for bit, so decode_heads is held to the
project's rule for float32 formulas (MARGIN, FLOOR_ULPS of tests/tracks_truth.py): at most MARGIN times the
reference's own distance from the truth, per column group, or FLOOR_ULPS float32 ulps where that is more.

The detections of the truth are the reference's rule (utils/general.py:1005-1116, greedy NMS as torchvision documents
it) in float64.  They equal a float32 evaluation only where no decision is close: planted() builds such inputs and
margins() says how far every decision is from its threshold.
"""
import numpy as np

from tracks_truth import EPS32, FLOOR_ULPS, MARGIN

MAX_WH = 7680.0
DECISION_MARGIN = 1e-3
YOLO_ANCHORS = (((10, 13), (16, 30), (33, 23)), ((30, 61), (62, 45), (59, 119)), ((116, 90), (156, 198), (373, 326)),
                ((436, 615), (739, 380), (925, 792)))
GROUPS = {"xy": slice(0, 2), "wh": slice(2, 4), "obj": slice(4, 5), "cls": slice(5, None)}


class Geometry:
    """anchor_grid [nl, na, 2] in pixels, stride [nl], nc: the arguments of perception.DetectGeometry."""

    def __init__(self, anchor_grid, stride, nc):
        self.anchor_grid = np.asarray(anchor_grid, dtype=np.float32)
        self.stride = np.asarray(stride, dtype=np.float32)
        self.nc = int(nc)
        self.nl, self.na = self.anchor_grid.shape[:2]
        self.no = self.nc + 5


def geometry(nc, strides=(8, 16, 32), na=3):
    """The YOLOv5 anchors of each stride (8, 16, 32, 64); an anchor beyond the third is an earlier one, 25 % larger."""
    ag = [[[v * (1 + 0.25 * (a // 3)) for v in YOLO_ANCHORS[{8: 0, 16: 1, 32: 2, 64: 3}[int(s)]][a % 3]]
           for a in range(na)] for s in strides]
    return Geometry(ag, strides, nc)


def level_shapes(hw, strides):
    return [(int(hw[0]) // int(s), int(hw[1]) // int(s)) for s in strides]


def n_rows(geom, shapes):
    return sum(geom.na * ny * nx for ny, nx in shapes)


def sigmoid64(v):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def decode(heads, geom, dtype=np.float64):
    """heads: list of float32 [bs, na*no, ny, nx] -> [bs, N, no] in ``dtype``: float64 is the truth; float32 is the
    same steps one float32 operation each (numpy's exp: a restatement, pinned to nothing)."""
    T = dtype
    z = []
    for l, h in enumerate(heads):
        bs, _, ny, nx = h.shape
        x = h.reshape(bs, geom.na, geom.no, ny, nx).transpose(0, 1, 3, 4, 2).astype(T)
        with np.errstate(all="ignore"):
            y = (T(1) / (T(1) + np.exp(-x))).astype(T)
            gx, gy = np.meshgrid(np.arange(nx, dtype=T), np.arange(ny, dtype=T))
            grid = np.stack([gx, gy], axis=-1)[None, None]
            xy = ((y[..., 0:2] * T(2) - T(0.5)) + grid) * T(geom.stride[l])
            t = y[..., 2:4] * T(2)
            wh = (t * t) * geom.anchor_grid[l].astype(T)[None, :, None, None, :]
        y = np.concatenate([xy, wh, y[..., 4:]], axis=-1)
        assert y.dtype == T
        z.append(y.reshape(bs, -1, geom.no))
    return np.ascontiguousarray(np.concatenate(z, axis=1))


def row_index(geom, shapes, level, a, y, x):
    """The row of (level, anchor, y, x) inside an image."""
    r = sum(geom.na * ny * nx for ny, nx in shapes[:level])
    ny, nx = shapes[level]
    return r + (a * ny + y) * nx + x


# ---- float64 detections ----

def detections_image64(x, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, max_det=300):
    """x float64 [N, no] -> (rows kept in order, [n, 6] float64 x1, y1, x2, y2, conf, cls, number of candidates
    suppressed)."""
    cand = np.nonzero(x[:, 4] > conf_thres)[0]
    cj = x[cand, 5:] * x[cand, 4:5]
    cls = np.argmax(cj, axis=1) if len(cand) else np.zeros(0, np.int64)
    conf = cj[np.arange(len(cand)), cls] if len(cand) else np.zeros(0)
    stays = conf > conf_thres
    if classes is not None:
        stays &= np.isin(cls, np.asarray(list(classes), dtype=np.int64))
    cand, conf, cls = cand[stays], conf[stays], cls[stays]
    order = np.argsort(-conf, kind="stable")
    cand, conf, cls = cand[order], conf[order], cls[order]
    b = x[cand, :4]
    box = np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], axis=1)
    sh = box + (cls * (0.0 if agnostic else MAX_WH))[:, None]
    area = (sh[:, 2] - sh[:, 0]) * (sh[:, 3] - sh[:, 1])
    kept, suppressed = [], 0
    for i in range(len(sh)):
        if len(kept):
            k = np.asarray(kept)
            iw = np.clip(np.minimum(sh[k, 2], sh[i, 2]) - np.maximum(sh[k, 0], sh[i, 0]), 0, None)
            ih = np.clip(np.minimum(sh[k, 3], sh[i, 3]) - np.maximum(sh[k, 1], sh[i, 1]), 0, None)
            inter = iw * ih
            if (inter / (area[k] + area[i] - inter) > iou_thres).any():
                suppressed += 1
                continue
        kept.append(i)
    full = len(kept)
    kept = np.asarray(kept[:max_det], dtype=np.int64)
    out = np.concatenate([box[kept], conf[kept, None], cls[kept, None].astype(np.float64)], axis=1)
    return cand[kept], out.reshape(-1, 6), suppressed if full <= max_det else None


def margins(x, conf_thres=0.25, iou_thres=0.45):
    """How far every decision of detections_image64(x) on the float64 prediction x [N, no] is from its threshold:
    the five distances the planted inputs keep above DECISION_MARGIN."""
    out = {"objectness": float(np.abs(x[:, 4] - conf_thres).min())}
    cand = np.nonzero(x[:, 4] > conf_thres)[0]
    cj = np.sort(x[cand, 5:] * x[cand, 4:5], axis=1)
    out["confidence"] = float(np.abs(cj[:, -1] - conf_thres).min()) if len(cand) else np.inf
    stays = cj[:, -1] > conf_thres
    out["class_gap"] = float((cj[stays, -1] - cj[stays, -2]).min()) if cj.shape[1] > 1 and stays.any() else np.inf
    conf = np.sort(cj[stays, -1])
    out["confidence_gap"] = float(np.diff(conf).min()) if len(conf) > 1 else np.inf
    rows = cand[stays]
    cls = np.argmax(x[rows, 5:] * x[rows, 4:5], axis=1)
    b = x[rows, :4]
    sh = np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], axis=1)
    sh = sh + (cls * MAX_WH)[:, None]
    area = (sh[:, 2] - sh[:, 0]) * (sh[:, 3] - sh[:, 1])
    iw = np.clip(np.minimum(sh[:, None, 2], sh[None, :, 2]) - np.maximum(sh[:, None, 0], sh[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(sh[:, None, 3], sh[None, :, 3]) - np.maximum(sh[:, None, 1], sh[None, :, 1]), 0, None)
    inter = iw * ih
    iou = inter / (area[:, None] + area[None, :] - inter)
    nz = iou[(inter > 0) & ~np.eye(len(rows), dtype=bool)]
    out["iou"] = float(np.abs(nz - iou_thres).min()) if len(nz) else np.inf
    return out


# ---- inputs ----

def dense_heads(nc, hw, bs, seed, strides=(8, 16, 32), na=3, scale=3.0):
    """Random logits, normal with deviation ``scale`` and clipped to +-10 (a float32 sigmoid keeps a relative
    accuracy there): (heads, geometry)."""
    geom = geometry(nc, strides, na)
    rng = np.random.RandomState(seed)
    heads = [np.clip(rng.normal(0.0, scale, (bs, geom.na * geom.no, ny, nx)), -10, 10).astype(np.float32)
             for ny, nx in level_shapes(hw, strides)]
    return heads, geom


def _logit(p):
    return np.log(p / (1.0 - p))


def _plant(heads, geom, shapes, b, level, a, y, x, box, k, obj, cls_p):
    """Write the logits of row (level, a, y, x) of image b: decode inverted for the box (cx, cy, w, h)."""
    s = float(geom.stride[level])
    aw, ah = (float(v) for v in geom.anchor_grid[level, a])
    sig = [((box[0] / s - x) + 0.5) / 2, ((box[1] / s - y) + 0.5) / 2, np.sqrt(box[2] / aw) / 2, np.sqrt(box[3] / ah) / 2]
    assert all(0.02 < v < 0.98 for v in sig), sig
    ch = a * geom.no
    for c, v in enumerate(sig):
        heads[level][b, ch + c, y, x] = _logit(v)
    heads[level][b, ch + 5 + k, y, x] = np.float32(_logit(cls_p))
    # the objectness that gives obj * cls = the wanted confidence with the class logit as float32 holds it
    cls_real = sigmoid64(heads[level][b, ch + 5 + k, y, x])
    heads[level][b, ch + 4, y, x] = _logit(obj / cls_real) if cls_p else _logit(obj)


def planted(nc, hw, bs, clusters, seed, strides=(8, 16, 32), conf_thres=0.25, decoys=4):
    """(heads, geometry): background objectness logit -12, other background logits uniform in [-6, -2]; per image
    ``clusters`` clusters of len(strides) overlapping boxes of one class, one per level, their logits the inverted
    decode; the confidences of all planted rows on a shuffled ladder between 0.3 and 0.9; ``decoys`` rows per image
    whose objectness passes and whose best confidence does not.  No margin is asserted here: first_good_seed() does."""
    geom = geometry(nc, strides)
    shapes = level_shapes(hw, strides)
    rng = np.random.RandomState(seed)
    heads = [rng.uniform(-6.0, -2.0, (bs, geom.na * geom.no, ny, nx)).astype(np.float32) for ny, nx in shapes]
    for l in range(geom.nl):
        for a in range(geom.na):
            heads[l][:, a * geom.no + 4] = -12.0
    n = bs * clusters * geom.nl
    ladder = 0.3 + 0.6 * (rng.permutation(n) + 0.5) / n
    used, i = set(), 0
    for b in range(bs):
        for c in range(clusters):
            k = int(rng.randint(0, nc))
            for _ in range(200):
                base = np.array([rng.uniform(4, hw[1] - 4), rng.uniform(4, hw[0] - 4), rng.uniform(28, 64),
                                 rng.uniform(28, 64)])
                members = []
                for l in range(geom.nl):
                    box = base + np.concatenate([rng.uniform(-2.5, 2.5, 2), rng.uniform(-4, 4, 2)])
                    box[0] = min(max(box[0], 0.5), hw[1] - 0.5)
                    box[1] = min(max(box[1], 0.5), hw[0] - 0.5)
                    s = float(geom.stride[l])
                    x, y = int(box[0] // s), int(box[1] // s)
                    fit = [a for a in range(geom.na) if (b, l, a, y, x) not in used and
                           all(0.05 < box[2 + d] / geom.anchor_grid[l, a, d] < 3.5 for d in range(2))]
                    if not fit:
                        break
                    members.append((l, fit[int(rng.randint(0, len(fit)))], y, x, box))
                if len(members) == geom.nl:
                    break
            assert len(members) == geom.nl, "no free cell for cluster %d of image %d" % (c, b)
            for l, a, y, x, box in members:
                used.add((b, l, a, y, x))
                _plant(heads, geom, shapes, b, l, a, y, x, box, k, ladder[i], 0.95)
                i += 1
        for _ in range(decoys):
            while True:
                l = int(rng.randint(0, geom.nl))
                a, y, x = int(rng.randint(0, geom.na)), int(rng.randint(0, shapes[l][0])), int(rng.randint(0, shapes[l][1]))
                if (b, l, a, y, x) not in used:
                    break
            used.add((b, l, a, y, x))
            heads[l][b, a * geom.no + 4, y, x] = _logit(rng.uniform(0.3, 0.6))     # best class below 0.12: conf < 0.08
    return heads, geom


def planted_ok(heads, geom, conf_thres=0.25, iou_thres=0.45):
    """(every margin >= DECISION_MARGIN and every image has a suppression, the margins, suppressions per image)."""
    truth = decode(heads, geom)
    worst, supp = {}, []
    for x in truth:
        for k, v in margins(x, conf_thres, iou_thres).items():
            worst[k] = min(worst.get(k, np.inf), v)
        supp.append(detections_image64(x, conf_thres, iou_thres, max_det=1 << 30)[2])
    return all(v >= DECISION_MARGIN for v in worst.values()) and all(s >= 1 for s in supp), worst, supp


def first_good_seed(nc, hw, bs, clusters, seeds=range(20)):
    for seed in seeds:
        heads, geom = planted(nc, hw, bs, clusters, seed)
        if planted_ok(heads, geom)[0]:
            return seed
    raise AssertionError("no seed of %s keeps every margin" % (list(seeds),))


def one_hot_head(nc, hw, bs, strides, na, where):
    """All logits -8 but +8 in every channel of the rows ``where`` = [(image, level, a, y, x), ...]."""
    geom = geometry(nc, strides, na)
    heads = [np.full((bs, geom.na * geom.no, ny, nx), -8.0, np.float32) for ny, nx in level_shapes(hw, strides)]
    for b, l, a, y, x in where:
        heads[l][b, a * geom.no:(a + 1) * geom.no, y, x] = 8.0
    return heads, geom


BUILDERS = {"dense_heads": dense_heads, "planted": planted}


def build_input(builder, args):
    heads, geom = BUILDERS[builder](**{k: tuple(v) if isinstance(v, list) else v for k, v in args.items()})
    for h in heads:
        assert h.dtype == np.float32 and h.flags["C_CONTIGUOUS"]
    return heads, geom


def input_bytes(heads, geom):
    return b"".join(h.tobytes() for h in heads) + geom.anchor_grid.tobytes() + geom.stride.tobytes()


# ---- the comparator ----

def errors(got, truth):
    """(relative L2, worst absolute element error) of one group against the float64 truth."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    d = np.abs(got - truth)
    return float(np.linalg.norm(d) / max(np.linalg.norm(truth), 1e-300)), float(d.max(initial=0.0))


def group_figures(got, truth, ref_rel_l2, ref_worst):
    """One group of elements against the float64 truth, given the reference's own two figures on the same input: the
    relative L2 may be MARGIN x the reference's or FLOOR_ULPS float32 ulps; every element's absolute error may be
    MARGIN x the reference's worst element or FLOOR_ULPS ulps of that element's own truth."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    rel, worst = errors(got, truth)
    bound_l2 = max(MARGIN * ref_rel_l2, FLOOR_ULPS * EPS32)
    bound_el = np.maximum(MARGIN * ref_worst, FLOOR_ULPS * EPS32 * np.abs(truth))
    excess = float((np.abs(got - truth) - bound_el).max(initial=-1.0))
    return dict(rel_l2=rel, rel_l2_reference=ref_rel_l2, rel_l2_bound=bound_l2, worst=worst, worst_reference=ref_worst,
                worst_excess=excess, ok=bool(np.isfinite(got).all() and rel <= bound_l2 and excess <= 0.0))


def pred_figures(got, truth, ref_figures):
    """{group: group_figures} of a [bs, N, no] prediction; ref_figures: {group: [rel_l2, worst]} of the reference."""
    return {g: group_figures(got[..., s], truth[..., s], *ref_figures[g]) for g, s in GROUPS.items()}
