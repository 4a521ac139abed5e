"""numpy restatement of the detector-output -> detections contract of gaussianrpg_amd.perception.detections
(csrc/nms.hip, include/grpg_rasterizer.h), float32 throughout: every arithmetic step below is one IEEE float32
operation on float32 operands, which is what the kernels do (-ffp-contract=off, correctly rounded divide).

It is written from the text of the reference's non_max_suppression (utils/general.py:1005-1116), its scale_coords /
clip_coords (utils/torch_utils.py:501-547) and the documented rule of torchvision.ops.nms (greedy: walk the boxes in
descending score, drop a box whose IoU with an already kept box exceeds the threshold).  The reference's modules
cannot be imported here -- they need torchvision, cv2 and pandas -- but its FUNCTIONS run: tests/golden/ref_nms.json +
.npz hold what non_max_suppression and scale_coords(...).round() themselves returned on CPU torch for 21 inputs
(tests/golden/make_golden_nms.py cuts them out with ast; only torchvision.ops.nms is a stand-in there), and
tests/test_nms_golden.py holds this restatement to those outputs bit for bit.  tests/test_nms_host.py compares the
greedy step with torchvision.ops.nms wherever torchvision imports.

Where the reference's text leaves a choice open -- and what its recorded output says about it:
  * equal confidences are ordered by ascending row (argsort(descending=True) leaves ties unspecified): this
    project's definition; the golden's inputs have distinct confidences and say nothing about it;
  * equal best class scores give the lowest class: likewise this project's definition;
  * thresholds are compared as float32 values: CONFIRMED by the golden (a row at exactly float32(t) is dropped, its
    successor kept, for t = 0.25 and for t = 0.3 where float32(0.3) > 0.3: CPU torch casts the Python threshold to
    the tensor's type).  The IoU threshold likewise here; torchvision's CPU kernel compares the float IoU with the
    threshold in double, which differs only for an IoU of exactly float32(t) when float32(t) > t -- for the
    reference's 0.45 no float32 value tells the two apart;
  * the frame mapping divides by the gain (a true float32 division) and rounds half to even: CONFIRMED by the
    golden on CPU torch, gain 1 and gain 224/375 alike, with all four clamps binding; it clamps with comparisons,
    NaN stays NaN: confirmed for the NaN box of nan_case(), whose NaN IoU is the stand-in's.
"""
import numpy as np

F = np.float32
MAX_WH = 7680
MAX_NMS = 30000


def candidates(x, conf_thres, classes=None):
    """x float32 [N, 5+nc] -> (rows, conf, cls) of the rows that stay, in ascending row order."""
    ct = F(conf_thres)
    with np.errstate(all="ignore"):
        rows = np.nonzero(x[:, 4] > ct)[0]                      # NaN > ct is false
        cj = x[rows, 5:] * x[rows, 4:5]                         # conf_j = obj * cls_j, float32
        assert cj.dtype == np.float32
        nan = np.isnan(cj).any(axis=1)
        cls = np.argmax(np.where(np.isnan(cj), F(-np.inf), cj), axis=1)     # the first (lowest) maximum
        conf = cj[np.arange(len(rows)), cls]
        stays = ~nan & (conf > ct)                              # torch.max gives NaN for a row with a NaN: dropped
    if classes is not None:
        stays &= np.isin(cls, np.asarray(list(classes), dtype=np.int64))
    return rows[stays], conf[stays], cls[stays].astype(np.int64)


def xywh2xyxy(x):
    two = F(2)
    with np.errstate(all="ignore"):
        hw, hh = x[:, 2] / two, x[:, 3] / two
        return np.stack([x[:, 0] - hw, x[:, 1] - hh, x[:, 0] + hw, x[:, 1] + hh], axis=1).astype(np.float32)


def area_of(b):
    with np.errstate(all="ignore"):
        return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def iou(a, area_a, b, area_b):
    """IoU of the kept boxes a [k,4] with one box b [4], float32 step by step.  min / max are the comparisons the
    kernel makes; with a NaN coordinate the area, and so the IoU, is NaN whichever operand they pick."""
    with np.errstate(all="ignore"):
        lx = np.where(b[0] > a[:, 0], b[0], a[:, 0])
        ly = np.where(b[1] > a[:, 1], b[1], a[:, 1])
        rx = np.where(b[2] < a[:, 2], b[2], a[:, 2])
        ry = np.where(b[3] < a[:, 3], b[3], a[:, 3])
        dw, dh = rx - lx, ry - ly
        iw, ih = np.where(dw > 0, dw, F(0)), np.where(dh > 0, dh, F(0))
        inter = iw * ih
        out = inter / (area_a + area_b - inter)
    assert out.dtype == np.float32
    return out


def greedy_nms(boxes, iou_thres, max_keep=None):
    """boxes float32 [n,4] in descending score -> indices kept, ascending.  A NaN IoU suppresses nothing."""
    thr = F(iou_thres)
    areas = area_of(boxes)
    kept = []
    kb = np.zeros((0, 4), np.float32)
    ka = np.zeros((0,), np.float32)
    for i in range(len(boxes)):
        if max_keep is not None and len(kept) == max_keep:
            break
        if len(kept) and bool((iou(kb, ka, boxes[i], areas[i]) > thr).any()):
            continue
        kept.append(i)
        kb = np.concatenate([kb, boxes[i:i + 1]])
        ka = np.concatenate([ka, areas[i:i + 1]])
    return np.asarray(kept, dtype=np.int64)


def frame_map(h, w, H, W):
    """scale_coords((h, w), ., (H, W)) with ratio_pad=None: (gain, pad_x, pad_y) in double."""
    gain = min(h / H, w / W)
    return gain, (w - W * gain) / 2, (h - H * gain) / 2


def to_frame(boxes, h, w, H, W):
    """float32 xyxy [n,4] in the detector input's pixels -> scale_coords(...).round() in the frame's."""
    gain, pad_x, pad_y = frame_map(h, w, H, W)
    gain, pad = F(gain), np.asarray([pad_x, pad_y, pad_x, pad_y], dtype=np.float32)
    hi = np.asarray([W, H, W, H], dtype=np.float32)
    with np.errstate(all="ignore"):
        t = (boxes.astype(np.float32) - pad) / gain
        t = np.where(t < 0, F(0), np.where(t > hi, hi, t))
        out = np.rint(t)
    assert out.dtype == np.float32
    return out


def detections_image(x, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, max_det=300,
                     max_nms=MAX_NMS, max_wh=MAX_WH, frame=None):
    """One image: x float32 [N, 5+nc] -> float32 [n, 6] rows x1, y1, x2, y2, conf, cls; frame: (h, w, H, W) or None."""
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] >= 6
    rows, conf, cls = candidates(x, conf_thres, classes)
    order = np.argsort(-conf, kind="stable")[:max_nms]           # rows ascend: stable = ties by ascending row
    rows, conf, cls = rows[order], conf[order], cls[order]
    box = xywh2xyxy(x[rows, :4])
    with np.errstate(all="ignore"):
        shift = cls.astype(np.float32) * F(0 if agnostic else max_wh)
        shifted = box + shift[:, None]
    assert shifted.dtype == np.float32
    keep = greedy_nms(shifted, iou_thres, max_keep=max_det)
    out = np.concatenate([box[keep], conf[keep, None], cls[keep, None].astype(np.float32)], axis=1).astype(np.float32)
    if frame is not None:
        out[:, :4] = to_frame(out[:, :4], *frame)
    return out


def detections(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, max_det=300,
               max_nms=MAX_NMS, max_wh=MAX_WH, frame=None):
    """prediction float32 [bs, N, 5+nc] -> (det float32 [bs, max_det, 6] zero below count, count int32 [bs])."""
    bs = prediction.shape[0]
    det = np.zeros((bs, max_det, 6), np.float32)
    count = np.zeros((bs,), np.int32)
    for b in range(bs):
        d = detections_image(prediction[b], conf_thres, iou_thres, classes, agnostic, max_det, max_nms, max_wh, frame)
        det[b, :len(d)] = d
        count[b] = len(d)
    return det, count


def kept_sets_float64(x, conf_thres=0.25, iou_thres=0.45, agnostic=False, max_wh=MAX_WH):
    """The same rule with the boxes and the IoU in float64 (candidates, confidences and order as in float32):
    the rows kept, in order.  For inputs on which every float32 step but the division is exact."""
    rows, conf, cls = candidates(x, conf_thres)
    order = np.argsort(-conf, kind="stable")
    rows, cls = rows[order], cls[order]
    xs = x[rows, :4].astype(np.float64)
    box = np.stack([xs[:, 0] - xs[:, 2] / 2, xs[:, 1] - xs[:, 3] / 2, xs[:, 0] + xs[:, 2] / 2,
                    xs[:, 1] + xs[:, 3] / 2], axis=1)
    box = box + (cls.astype(np.float64) * (0 if agnostic else max_wh))[:, None]
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    kept = []
    for i in range(len(box)):
        ok = True
        for k in kept:
            iw = max(min(box[k, 2], box[i, 2]) - max(box[k, 0], box[i, 0]), 0.0)
            ih = max(min(box[k, 3], box[i, 3]) - max(box[k, 1], box[i, 1]), 0.0)
            inter = iw * ih
            union = area[k] + area[i] - inter
            if union != 0 and inter / union > float(np.float32(iou_thres)):
                ok = False
                break
        if ok:
            kept.append(i)
    return rows[np.asarray(kept, dtype=np.int64)]


# ---- hand-made rows shared by the host and the GPU tests ----

def rows_of(*rows, nc=1):
    """rows (x1, y1, x2, y2, obj, cls_0, ...) given as corners -> float32 [n, 5+nc] in the head's cx, cy, w, h."""
    out = np.zeros((len(rows), 5 + nc), np.float32)
    for i, r in enumerate(rows):
        x1, y1, x2, y2 = r[:4]
        out[i, :4] = [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]
        out[i, 4:4 + len(r) - 4] = r[4:]
    return out


def nan_case():
    nan = float("nan")
    x = rows_of((0, 0, 10, 10, nan, 1.0, 1.0),        # NaN objectness: dropped
                (20, 0, 30, 10, 0.9, nan, 1.0),       # NaN class score: conf is NaN (torch.max), dropped
                (40, 0, 50, 10, 0.8, 1.0, 0.5),       # a NaN box, made below: kept, suppresses nothing
                (40, 0, 50, 10, 0.7, 1.0, 0.5),       # would fall to row 2 if its IoU were a number
                (41, 0, 51, 10, 0.6, 1.0, 0.5), nc=2)  # falls to row 3
    x[2, 0] = nan
    return x


def tie_case():
    """Rows 0 and 2 tie at 0.5 and overlap; row 1 is better and elsewhere.  Row 0 has two equal class scores."""
    return rows_of((0, 0, 10, 10, 0.5, 1.0, 1.0), (100, 100, 110, 110, 0.75, 1.0, 0.0), (1, 0, 11, 10, 0.5, 0.0, 1.0),
                   nc=2)


# ---- seeded inputs whose candidate count is what the caller asks for ----

def make_prediction(N, nc, n_cand, seed, size=(640, 640), clusters=None, jitter=4.0, bs=1, grid=None):
    """float32 [bs, N, 5+nc]: exactly n_cand rows per image with obj > 0.5 and a best class score > 0.6 (so
    conf > 0.3 > 0.25), at seeded rows; every other row has obj < 0.2.  Boxes: centres uniform over `size`, sides
    8..120 -- or, with clusters=k, jittered copies of k boxes (heavy overlap).  grid: round the boxes to multiples of
    it.  Confidences are random: a test that needs them distinct asserts that they are."""
    rng = np.random.RandomState(seed)
    p = np.zeros((bs, N, 5 + nc), np.float32)
    for b in range(bs):
        p[b, :, 0] = rng.uniform(0, size[1], N)
        p[b, :, 1] = rng.uniform(0, size[0], N)
        p[b, :, 2:4] = rng.uniform(8, 120, (N, 2))
        p[b, :, 4] = rng.uniform(0.0, 0.2, N)
        p[b, :, 5:] = rng.uniform(0.0, 0.5, (N, nc))
        n = n_cand[b] if isinstance(n_cand, (list, tuple)) else n_cand
        rows = np.sort(rng.choice(N, n, replace=False))
        if clusters:
            base = np.stack([rng.uniform(100, size[1] - 100, clusters), rng.uniform(100, size[0] - 100, clusters),
                             rng.uniform(40, 120, clusters), rng.uniform(40, 120, clusters)], axis=1)
            which = rng.randint(0, clusters, n)
            p[b, rows, :4] = (base[which] + rng.uniform(-jitter, jitter, (n, 4))).astype(np.float32)
            p[b, rows, 5:] = rng.uniform(0.0, 0.3, (n, nc))
            p[b, rows, 5 + which % nc] = rng.uniform(0.7, 1.0, n)
        else:
            p[b, rows, 5 + rng.randint(0, nc, n)] = rng.uniform(0.6, 1.0, n)
        p[b, rows, 4] = (0.5 + 0.5 * (rng.permutation(n) + 0.5) / max(n, 1)).astype(np.float32)
        if grid:
            p[b, :, :4] = np.round(p[b, :, :4] / grid) * grid
    return p


# ---- the inputs of tests/golden/ref_nms.* (make_golden_nms.py records the reference's own outputs for them) ----

SIM = (1088, 1600, 1066, 1600)        # LetterboxPlan.for_simulator(1066, 1600): gain 1, 11 rows of border above
RESIZE = (224, 640, 375, 1242)        # LetterboxPlan(375, 1242, 640)


def frame_case(h, w, seed):
    """400 candidates on a half-pixel grid over the (h, w) input, 40 each pushed beyond its right, top, left and
    bottom side: all four clamps of the frame mapping bind, and mapped values land on halves."""
    p = make_prediction(3000, 3, 400, seed=seed, size=(h, w), grid=0.5)
    rows = np.nonzero(p[0, :, 4] > F(0.25))[0]
    p[0, rows[:40], 0] += w
    p[0, rows[40:80], 1] -= h
    p[0, rows[80:120], 0] -= w
    p[0, rows[120:160], 1] += h
    return p


def threshold_case(t, product):
    """Rows at the confidence threshold t and one ulp above it, and one plainly above.  product=False: the
    objectness is float32(t) / its successor, the class score 1.  product=True: objectness 0.5 and class score
    2 * float32(t) / 2 * its successor, so obj * cls lands exactly there."""
    ft = F(t)
    up = np.nextafter(ft, F(1))
    if product:
        x = rows_of((0, 0, 10, 10, 0.5, F(2) * ft), (100, 0, 110, 10, 0.5, F(2) * up), (200, 0, 210, 10, 0.9, 1.0))
        assert F(0.5) * x[0, 5] == ft and F(0.5) * x[1, 5] == up
    else:
        x = rows_of((0, 0, 10, 10, ft, 1.0), (100, 0, 110, 10, up, 1.0), (200, 0, 210, 10, 0.9, 1.0))
        assert x[0, 4] == ft and x[1, 4] == up
    return x[None]


MAX_NMS_ISOLATED_Y = 2000.0


def max_nms_case(seed=21):
    """N = 32768, nc = 1, class score exactly 1 (conf = obj): 30 000 candidates in 56 well separated clusters, and
    200 isolated candidates (centre y >= MAX_NMS_ISOLATED_Y) that hold the 200 LOWEST confidences -- beyond the
    reference's max_nms = 30000 cut, so absent from its output although nothing overlaps them.  The confidences are
    (20000 + rank) / 65536, exact in float32 and distinct."""
    rng = np.random.RandomState(seed)
    N, n_cl, n_iso = 32768, 30000, 200
    p = np.zeros((1, N, 6), np.float32)
    p[0, :, 0] = rng.uniform(0, 1200, N)
    p[0, :, 1] = rng.uniform(0, 1000, N)
    p[0, :, 2:4] = rng.uniform(8, 120, (N, 2))
    p[0, :, 4] = rng.uniform(0.0, 0.2, N)
    p[0, :, 5] = 1.0
    rows = rng.permutation(N)[:n_cl + n_iso]
    iso, cl = rows[:n_iso], rows[n_iso:]
    k = np.arange(n_iso)
    p[0, iso, 0] = 50.0 + 40.0 * (k % 25)
    p[0, iso, 1] = MAX_NMS_ISOLATED_Y + 40.0 * (k // 25)
    p[0, iso, 2:4] = 20.0
    p[0, iso, 4] = ((20000 + rng.permutation(n_iso)) / 65536.0).astype(np.float32)
    c = np.arange(56)
    base = np.stack([100.0 + 150.0 * (c % 8), 100.0 + 150.0 * (c // 8), rng.uniform(60, 100, 56),
                     rng.uniform(60, 100, 56)], axis=1)
    which = rng.randint(0, 56, n_cl)
    p[0, cl, :4] = (base[which] + rng.uniform(-3, 3, (n_cl, 4))).astype(np.float32)
    p[0, cl, 4] = ((20000 + n_iso + rng.permutation(n_cl)) / 65536.0).astype(np.float32)
    return p


BUILDERS = {"make_prediction": make_prediction, "frame_case": frame_case, "threshold_case": threshold_case,
            "max_nms_case": max_nms_case, "nan_case": lambda: nan_case()[None]}


def build_input(builder, args):
    """The float32 [bs, N, 5+nc] input a golden case names: BUILDERS[builder](**args)."""
    p = BUILDERS[builder](**args)
    assert p.dtype == np.float32 and p.ndim == 3 and p.flags["C_CONTIGUOUS"]
    return p
