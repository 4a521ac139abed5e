"""GPU tests of the fused detector head -> prediction / detections step (gaussianrpg_amd/perception.py decode_heads /
detections_from_heads, csrc/nms.hip).

1. decode_heads against the float64 truth (tests/detect_truth.py) per column group: at most MARGIN x the reference's
   own distance from that truth on the same input (recorded in tests/golden/ref_detect.json), or FLOOR_ULPS float32
   ulps; shape and row order exact.  Every figure is printed before it is asserted and collected in
   bench_out/detect_parity.json (committed copy: profiles/detect_parity.json).
2. detections_from_heads(h) against detections(decode_heads(h)): det and count bit for bit, whatever the input.
3. detections_from_heads against the reference's recorded detections on the margin-planted inputs: count, order and
   class exact, confidences and boxes by the rule of 1.
4. The C ABI through ctypes, workspace and outputs prefilled with 0xFF.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import detect_truth as dt
from test_detect_host import CASES, PLANTED, case_input, golden_dets, truth_dets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _record(name, figures):
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "detect_parity.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[name] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(name, json.dumps(figures))


def _geom(g):
    from gaussianrpg_amd.perception import DetectGeometry
    return DetectGeometry(g.anchor_grid, g.stride, g.nc)


def _to(heads, dev):
    return [torch.from_numpy(h.copy()).to(dev) for h in heads]


def _bits(t):
    return t.view(torch.int32)


# ---- 1. decode_heads against the float64 truth ----

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_decode_heads_against_the_float64_truth(dev, case):
    from gaussianrpg_amd.perception import decode_heads
    heads, g, truth = case_input(case)
    h = _to(heads, dev)
    pred = decode_heads(h, _geom(g))
    assert pred.dtype == torch.float32 and list(pred.shape) == case["shape"] and pred.is_contiguous()
    out = torch.full(case["shape"], NAN, device=dev)
    assert decode_heads(h, _geom(g), out=out) is out
    assert torch.equal(_bits(out), _bits(pred)), "out= differs, or an element of it was not written"
    for a, b in zip(h, heads):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)), "a head changed"
    figs = dt.pred_figures(pred.cpu().numpy(), truth, case["figures"])
    _record("decode/" + case["name"], figs)
    for k, f in figs.items():
        assert f["ok"], "%s / %s: beyond %gx the reference's own distance from the truth: %r" % (case["name"], k,
                                                                                                dt.MARGIN, f)


def test_decode_heads_row_order(dev):
    """One hot row per (image, level, anchor, y, x) corner, all at once: the hot rows of the prediction are
    row_index()'s, for the shapes whose waves straddle anchors, levels and images, odd nx, one level, and four."""
    from gaussianrpg_amd.perception import decode_heads
    for nc, hw, bs, strides, na in ((80, (64, 96), 2, (8, 16, 32), 3), (3, (96, 160), 1, (8, 16, 32), 3),
                                    (1, (40, 56), 1, (8,), 1), (65, (128, 192), 2, (8, 16, 32, 64), 4)):
        shapes = dt.level_shapes(hw, strides)
        where = sorted(set((b, l, a, y, x) for b in (0, bs - 1) for l in range(len(strides)) for a in (0, na - 1)
                           for y in (0, shapes[l][0] - 1) for x in (0, shapes[l][1] - 1)))
        heads, g = dt.one_hot_head(nc, hw, bs, strides, na, where)
        pred = decode_heads(_to(heads, dev), _geom(g)).cpu().numpy()
        assert pred.shape == (bs, dt.n_rows(g, shapes), nc + 5)
        hot = sorted(map(tuple, np.argwhere(pred[:, :, 4] > 0.5).tolist()))
        assert hot == sorted((b, dt.row_index(g, shapes, l, a, y, x)) for b, l, a, y, x in where), (nc, hw)
        truth = dt.decode(heads, g)
        assert np.allclose(pred, truth, rtol=1e-5, atol=0)


# ---- 2. the two routes give the same bits ----

def _plan(hw, dev):
    """A frame four rows shorter than the input and 1.5 x its size: a gain below 1 and a pad."""
    from gaussianrpg_amd.perception import LetterboxPlan
    H, W = (hw[0] - 4) * 3 // 2, hw[1] * 3 // 2
    p = LetterboxPlan(H, W, hw[1], auto=True, stride=8, device=dev)
    assert p.out_shape == tuple(hw), (p, hw)
    return p


def _both(dev, what, heads, g, **kw):
    """detections_from_heads(h) and detections(decode_heads(h)), asserted identical; returns (det, count) on the host."""
    from gaussianrpg_amd.perception import decode_heads, detections, detections_from_heads
    h, geom = _to(heads, dev), _geom(g)
    fused = detections_from_heads(h, geom, **kw)
    plain = detections(decode_heads(h, geom), **kw)
    bs, max_det = heads[0].shape[0], kw.get("max_det", 300)
    assert tuple(fused[0].shape) == (bs, max_det, 6) and fused[0].dtype == torch.float32 and fused[0].is_contiguous()
    assert tuple(fused[1].shape) == (bs,) and fused[1].dtype == torch.int32
    assert fused[1].tolist() == plain[1].tolist(), (what, fused[1].tolist(), plain[1].tolist())
    bad = (_bits(fused[0]) != _bits(plain[0])).cpu().numpy()
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size,
                                                                      np.argwhere(bad)[0].tolist())
    for a, b in zip(h, heads):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)), "%s: a head changed" % what
    return fused[0].cpu().numpy(), fused[1].cpu().numpy()


def _with_ties(heads, g, n=40, seed=0):
    """Copy the logits of n cells into a later cell of the same level and anchor: the same objectness and class
    scores in a later row, so equal confidences that only the row order resolves."""
    rng = np.random.RandomState(seed)
    heads = [h.copy() for h in heads]
    for _ in range(n):
        l = int(rng.randint(0, len(heads)))
        bs, _, ny, nx = heads[l].shape
        if ny * nx < 2:
            continue
        b, a = int(rng.randint(0, bs)), int(rng.randint(0, g.na))
        src, dst = sorted(rng.choice(ny * nx, 2, replace=False).tolist())
        ch = slice(a * g.no, (a + 1) * g.no)
        heads[l][b, ch, dst // nx, dst % nx] = heads[l][b, ch, src // nx, src % nx]
        heads[l][b, a * g.no + 4, dst // nx, dst % nx] = heads[l][b, a * g.no + 4, src // nx, src % nx] = 3.0
    return heads


DENSE = {"64x96_bs2_nc80": dict(nc=80, hw=(64, 96), bs=2, seed=11),
         "96x160_nc3": dict(nc=3, hw=(96, 160), bs=1, seed=12),
         "96x160_bs2_nc65": dict(nc=65, hw=(96, 160), bs=2, seed=13),
         "5x7_one_level_na1_nc1": dict(nc=1, hw=(40, 56), bs=1, seed=14, strides=(8,), na=1),
         "nl4_nc65": dict(nc=65, hw=(128, 192), bs=1, seed=15, strides=(8, 16, 32, 64))}


@pytest.mark.parametrize("name", list(DENSE))
def test_routes_agree_on_dense_heads_with_ties(dev, name):
    heads, g = dt.dense_heads(**DENSE[name])
    heads = _with_ties(heads, g)
    hw = DENSE[name]["hw"]
    det, count = _both(dev, name, heads, g)
    assert (count > 0).all()
    ties = sum(len(np.unique(det[b, :c, 4])) < c for b, c in enumerate(count))
    for max_det in (1, 10, 1024):
        d, c = _both(dev, "%s max_det=%d" % (name, max_det), heads, g, max_det=max_det, conf_thres=0.1, iou_thres=0.3)
        assert (c <= max_det).all() and (c > 0).all()
    full, cfull = _both(dev, name + " all", heads, g, max_det=1024, conf_thres=0.05, iou_thres=0.9)
    ties += sum(len(np.unique(full[b, :c, 4])) < c for b, c in enumerate(cfull))
    assert ties > 0, "no two detections tie: the tie rule went untested"
    _both(dev, name + " agnostic", heads, g, agnostic=True)
    classes = [0] if g.nc == 1 else [0, 2, g.nc - 1]
    d, c = _both(dev, name + " classes", heads, g, classes=classes, conf_thres=0.1)
    assert all(set(d[b, :n, 5].tolist()) <= set(map(float, classes)) for b, n in enumerate(c))
    _both(dev, name + " classes none of the head's", heads, g, classes=[g.nc + 3])
    d, c = _both(dev, name + " plan", heads, g, plan=_plan(hw, dev), max_det=10)
    assert np.array_equal(d[..., :4], np.rint(d[..., :4]))


def test_routes_agree_beyond_one_staging_round(dev):
    """N = 2520 at conf_thres = 0.001: the walk stages more than 1024 candidates; max_nms below and above their
    number."""
    from gaussianrpg_amd.perception import decode_heads
    heads, g = dt.dense_heads(nc=80, hw=(160, 256), bs=1, seed=16)
    pred = decode_heads(_to(heads, dev), _geom(g)).cpu().numpy()[0]
    n_cand = int(((pred[:, 4] > 0.001) & ((pred[:, 5:] * pred[:, 4:5]).max(1) > 0.001)).sum())
    assert 1024 < n_cand < 2520
    for max_nms in (n_cand - 700, n_cand + 100):
        for max_det in (300, 1024):
            d, c = _both(dev, "max_nms=%d max_det=%d" % (max_nms, max_det), heads, g, conf_thres=0.001, iou_thres=0.6,
                         max_nms=max_nms, max_det=max_det)
            assert c[0] > 100
    a = _both(dev, "cut", heads, g, conf_thres=0.001, iou_thres=0.99, max_nms=1100, max_det=1024)
    b = _both(dev, "uncut", heads, g, conf_thres=0.001, iou_thres=0.99, max_nms=n_cand + 100, max_det=1024)
    assert a[1][0] == 1024 or a[1][0] < b[1][0]


def test_routes_agree_with_inf_and_nan_logits(dev):
    """+-Inf and NaN logits in objectness, class and box planes are ordinary inputs: a NaN objectness or class score
    drops the row, a NaN box stays and suppresses nothing, as in detections."""
    heads, g = dt.dense_heads(nc=3, hw=(64, 96), bs=2, seed=17)
    heads = [h.copy() for h in heads]
    rng = np.random.RandomState(5)
    planted = 0
    for l, h in enumerate(heads):
        bs, _, ny, nx = h.shape
        for v in (INF, -INF, NAN):
            for c in (0, 2, 4, 5, 7):                 # x, w, objectness, first and last class
                for _ in range(2):
                    b, a, y, x = (int(rng.randint(0, k)) for k in (bs, g.na, ny, nx))
                    h[b, a * g.no + c, y, x] = v
                    if c != 4:
                        h[b, a * g.no + 4, y, x] = 4.0   # the row passes the objectness test: its planes are read
                    planted += 1
    assert planted == 90
    for kw in (dict(), dict(conf_thres=0.05, iou_thres=0.2, max_det=1024), dict(agnostic=True, plan=_plan((64, 96), dev))):
        det, count = _both(dev, "inf / nan %s" % sorted(kw), heads, g, **kw)
        assert (count > 0).all() and not np.isnan(det[..., 4]).any()
    assert np.isnan(det).any() or np.isinf(det).any()    # a box with a non-finite side was kept


def test_out_is_reused_and_calls_repeat(dev):
    from gaussianrpg_amd.perception import detections_from_heads
    heads, g = dt.dense_heads(nc=80, hw=(64, 96), bs=2, seed=18)
    other, _ = dt.dense_heads(nc=80, hw=(64, 96), bs=2, seed=19)
    geom = _geom(g)
    det = torch.full((2, 50, 6), NAN, device=dev)
    count = torch.full((2,), -7, dtype=torch.int32, device=dev)
    want = {}
    for key, hs in (("a", heads), ("b", other), ("a2", heads)):
        h = _to(hs, dev)
        r = detections_from_heads(h, geom, max_det=50, out=(det, count))
        assert r[0] is det and r[1] is count
        fresh = detections_from_heads(h, geom, max_det=50)
        assert torch.equal(_bits(det), _bits(fresh[0])) and torch.equal(count, fresh[1]), key
        assert not torch.isnan(det).any()
        want[key] = (det.clone(), count.clone())
    assert torch.equal(_bits(want["a"][0]), _bits(want["a2"][0])) and torch.equal(want["a"][1], want["a2"][1])
    assert not torch.equal(_bits(want["a"][0]), _bits(want["b"][0]))
    with pytest.raises(RuntimeError, match="out det must be a contiguous float32"):
        detections_from_heads(_to(heads, dev), geom, max_det=60, out=(det, count))
    with pytest.raises(RuntimeError, match=r"out must be a contiguous float32 \[2,378,85\]"):
        from gaussianrpg_amd.perception import decode_heads
        decode_heads(_to(heads, dev), geom, out=torch.zeros(2, 378, 84, device=dev))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    h = _to(heads, dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        side = detections_from_heads(h, geom, max_det=50)
    s.synchronize()
    assert torch.equal(_bits(side[0]), _bits(want["a"][0])) and torch.equal(side[1], want["a"][1])


def test_simulator_detections_from_heads_both_ways(dev):
    from gaussianrpg_amd import harness as hz
    case = PLANTED[0]
    heads, g, _ = case_input(case)
    h, geom, plan = _to(heads, dev), _geom(g), _plan((64, 96), dev)
    fused = hz.simulator_detections_from_heads(h, geom, plan, fused=True)
    plain = hz.simulator_detections_from_heads(h, geom, plan, fused=False)
    assert len(fused) == len(plain) == 2
    for b, (f, p) in enumerate(zip(fused, plain)):
        n = min(case["counts"][b], 10)
        assert f.shape == p.shape == (n, 6)
        assert torch.equal(f[:, 5], p[:, 5]) and torch.allclose(f[:, 4], p[:, 4], rtol=1e-5, atol=0)
        assert torch.equal(f[:, :4], f[:, :4].round()) and (f[:, :4] - p[:, :4]).abs().max() <= 1   # whole pixels


# ---- 3. against the reference's recorded detections ----

@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_detections_from_heads_equal_the_references(dev, case):
    from gaussianrpg_amd.perception import detections_from_heads
    heads, g, _ = case_input(case)
    det, count = detections_from_heads(_to(heads, dev), _geom(g))
    det, count = det.cpu().numpy(), count.cpu().numpy()
    ref, truth = golden_dets(case), truth_dets(case)
    assert count.tolist() == case["counts"]
    got = []
    for b, n in enumerate(count):
        d = det[b, :n]
        assert np.array_equal(d[:, 5], ref[b][:, 5]), "%s image %d: class or order differs" % (case["name"], b)
        assert (np.diff(d[:, 4]) < 0).all() and np.abs(d[:, :5] - ref[b][:, :5]).max() < dt.DECISION_MARGIN / 2
        assert not det[b, n:].any()
        got.append(d)
    got, truth = np.concatenate(got), np.concatenate(truth)
    figs = {"box": dt.group_figures(got[:, :4], truth[:, :4], *case["det_figures"]["box"]),
            "conf": dt.group_figures(got[:, 4], truth[:, 4], *case["det_figures"]["conf"])}
    _record("detections/" + case["name"], figs)
    for k, f in figs.items():
        assert f["ok"], "%s / %s: beyond %gx the reference's own distance from the truth: %r" % (case["name"], k,
                                                                                                dt.MARGIN, f)


# ---- 4. the C ABI ----

class _Geometry(ctypes.Structure):
    _fields_ = [("nl", ctypes.c_int), ("na", ctypes.c_int), ("nc", ctypes.c_int), ("ny", ctypes.c_int * 4),
                ("nx", ctypes.c_int * 4), ("stride", ctypes.c_float * 4), ("anchor_grid", (ctypes.c_float * 2) * 16)]


def test_c_abi_directly(dev):
    """ctypes, no _C: torch only allocates.  Workspace, det, count and pred start as 0xFF bytes: a box-array row
    that is not a candidate's holds NaN and is never read."""
    from gaussianrpg_amd.perception import decode_heads, detections_from_heads
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_detect_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_detect_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.grpg_detect_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.grpg_detect_detections.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
    heads, g = dt.dense_heads(nc=4, hw=(96, 160), bs=2, seed=20)
    heads = _with_ties(heads, g)
    h, geom = _to(heads, dev), _geom(g)
    bs, N = 2, 945

    def geometry(**o):
        s = _Geometry(nl=g.nl, na=g.na, nc=g.nc)
        for l, t in enumerate(heads):
            s.ny[l], s.nx[l], s.stride[l] = t.shape[2], t.shape[3], float(g.stride[l])
        for i, (w, hh) in enumerate(g.anchor_grid.reshape(-1, 2)):
            s.anchor_grid[i][0], s.anchor_grid[i][1] = float(w), float(hh)
        for k, v in o.items():
            setattr(s, k, v)
        return s
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in h])
    nbytes = lib.grpg_detect_workspace_bytes(bs, N)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    allow = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=dev)
    det = torch.full((bs * 20 * 6 * 4,), 0xFF, dtype=torch.uint8, device=dev)
    count = torch.full((bs * 4,), 0xFF, dtype=torch.uint8, device=dev)
    pred = torch.full((bs * N * 9 * 4,), 0xFF, dtype=torch.uint8, device=dev)
    plan = _plan((96, 160), dev)
    from gaussianrpg_amd.perception import frame_map
    fmap = (ctypes.c_double * 6)(*frame_map(plan))
    torch.cuda.synchronize()

    def call(**o):
        a = dict(heads=ctypes.addressof(ptrs), geom=geometry(), bs=bs, conf=0.25, iou=0.45, allow=allow.data_ptr(),
                 max_det=20, max_nms=30000, max_wh=7680.0, ws=ws.data_ptr(), nbytes=nbytes, det=det.data_ptr())
        a.update(o)
        return lib.grpg_detect_detections(a["heads"], ctypes.addressof(a["geom"]) if a["geom"] else None, a["bs"],
                                          a["conf"], a["iou"], a["allow"], 0, a["max_det"], a["max_nms"], a["max_wh"],
                                          ctypes.addressof(fmap), a["ws"], a["nbytes"], a["det"], count.data_ptr(), None)
    assert call() == 0, lib.grpg_last_error()
    good, no_level = geometry(), geometry(nl=0)
    assert lib.grpg_detect_decode(ctypes.addressof(ptrs), ctypes.addressof(good), bs, pred.data_ptr(), None) == 0, \
        lib.grpg_last_error()
    torch.cuda.synchronize()
    want = detections_from_heads(h, geom, classes=[0, 2, 3], max_det=20, plan=plan)
    assert torch.equal(det.view(torch.int32).view(bs, 20, 6), _bits(want[0]))
    assert torch.equal(count.view(torch.int32), want[1]) and (want[1] > 0).all()
    assert torch.equal(pred.view(torch.int32).view(bs, N, 9), _bits(decode_heads(h, geom)))
    # the argument errors: all before any launch
    assert call(nbytes=nbytes - 1) == -1 and b"workspace smaller than grpg_detect_workspace_bytes" in lib.grpg_last_error()
    assert call(ws=ws.data_ptr() + 4) == -1 and b"256-byte aligned" in lib.grpg_last_error()
    assert call(max_det=1025) == -1 and b"max_det" in lib.grpg_last_error()
    assert call(max_det=0) == -1 and call(max_nms=0) == -1 and call(max_wh=-1.0) == -1
    assert call(conf=1.5) == -1 and b"[0, 1]" in lib.grpg_last_error()
    assert call(iou=NAN) == -1
    assert call(bs=0) == -1 and call(heads=None) == -1 and call(geom=None) == -1 and call(ws=None) == -1
    assert call(det=None) == -1 and call(det=det.data_ptr() + 2) == -1
    for bad in (dict(nl=0), dict(nl=5), dict(na=0), dict(na=6), dict(nc=0)):
        assert call(geom=geometry(**bad)) == -1, bad
    assert b"positive" in lib.grpg_last_error()
    assert call(geom=geometry(nl=4, na=5)) == -1 and b"nl * na <= 16" in lib.grpg_last_error()
    for nc in (2 ** 31 - 1, 2 ** 31 - 5, (2 ** 31) // 3):            # 5 + nc, or na * (5 + nc), no longer an int
        assert call(geom=geometry(nc=nc)) == -1 and b"na * (5 + nc) must be below 2^31" in lib.grpg_last_error(), nc
    bad = geometry()
    bad.ny[1] = 0
    assert call(geom=bad) == -1 and b"ny and nx" in lib.grpg_last_error()
    bad = geometry()
    bad.stride[2] = 0.0
    assert call(geom=bad) == -1 and b"strides" in lib.grpg_last_error()
    bad = geometry()
    bad.anchor_grid[4][1] = INF
    assert call(geom=bad) == -1 and b"anchor_grid" in lib.grpg_last_error()
    bad = geometry()
    bad.ny[0], bad.nx[0] = 2 ** 15, 2 ** 15
    assert call(geom=bad) == -1 and b"2^31" in lib.grpg_last_error()
    null_head = (ctypes.c_void_p * 3)(h[0].data_ptr(), None, h[2].data_ptr())
    assert call(heads=ctypes.addressof(null_head)) == -1 and b"every head" in lib.grpg_last_error()
    assert lib.grpg_detect_decode(ctypes.addressof(ptrs), ctypes.addressof(good), bs, None, None) == -1
    assert lib.grpg_detect_decode(ctypes.addressof(ptrs), ctypes.addressof(no_level), bs, pred.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(det.view(torch.int32).view(bs, 20, 6), _bits(want[0]))       # a refused call writes nothing
