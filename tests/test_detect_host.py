"""CPU tests (-m "not gpu") of the detector head -> prediction / detections step (gaussianrpg_amd/perception.py
decode_heads / detections_from_heads, csrc/nms.hip): the float64 restatement (tests/detect_truth.py) against what the
reference's OWN ``Detect.forward`` and ``non_max_suppression`` returned (tests/golden/ref_detect.*, recorded by
tests/golden/make_golden_detect.py), the margins of the planted inputs, the row order, and the refusals of the Python
surface, none of which needs a device.  tests/test_gpu_detect.py compares the HIP ops with the same golden."""
import ctypes
import hashlib
import json
import os
import types

import numpy as np
import pytest
import torch

import detect_truth as dt
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
NAN = float("nan")


def load_golden():
    with open(os.path.join(GOLDEN, "ref_detect.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "ref_detect.npz"))
    return meta, {k: z[k] for k in z.files}


META, ARRAYS = load_golden()
CASES = META["cases"]
PLANTED = [c for c in CASES if c["builder"] == "planted"]
_INPUTS = {}


def case_input(case):
    """(heads, geometry, float64 truth) of a case, rebuilt from its builder and checked against the recorded hash;
    built once and read-only."""
    if case["name"] not in _INPUTS:
        heads, geom = dt.build_input(case["builder"], case["args"])
        assert hashlib.sha256(dt.input_bytes(heads, geom)).hexdigest() == case["sha256"], \
            "%s: the rebuilt input is not the recorded one" % case["name"]
        truth = dt.decode(heads, geom)
        assert list(truth.shape) == case["shape"]
        for a in heads + [truth]:
            a.setflags(write=False)
        _INPUTS[case["name"]] = (heads, geom, truth)
    return _INPUTS[case["name"]]


def golden_dets(case):
    return [ARRAYS["%s/%d/det" % (case["name"], b)] for b in range(case["shape"][0])]


def truth_dets(case):
    return [dt.detections_image64(x)[1] for x in case_input(case)[2]]


def test_golden_layout():
    assert "Detect" in META["source"] and "non_max_suppression" in META["source"]
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) == 9 and len(PLANTED) == 4
    assert [(c["args"]["nc"], tuple(c["args"]["hw"]), c["args"]["bs"], c["args"]["clusters"]) for c in PLANTED] == \
        [(80, (64, 96), 2, 6), (3, (96, 160), 1, 16), (1, (64, 96), 1, 6), (80, (160, 256), 1, 40)]
    assert set(k.split("/")[0] for k in ARRAYS) <= set(names)
    for c in CASES:
        assert (c["name"] + "/pred" in ARRAYS) == c["pred_stored"]
        assert set(c["figures"]) == set(dt.GROUPS)
    size = sum(os.path.getsize(os.path.join(GOLDEN, "ref_detect." + e)) for e in ("json", "npz"))
    assert size < 512 * 1024


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_inputs_keep_every_margin(case):
    heads, geom, truth = case_input(case)
    assert case["args"]["seed"] == dt.first_good_seed(*(case["args"][k] for k in ("nc", "hw", "bs", "clusters")))
    ok, worst, supp = dt.planted_ok(heads, geom)
    assert set(worst) == {"objectness", "confidence", "class_gap", "confidence_gap", "iou"}
    for k, v in worst.items():
        assert v >= dt.DECISION_MARGIN == 1e-3, (k, v)
    assert ok and all(s >= 1 for s in supp) and supp == case["suppressed"]
    for l in range(geom.nl):          # the background objectness logit
        obj = heads[l].reshape(heads[l].shape[0], geom.na, geom.no, -1)[:, :, 4]
        assert (obj == np.float32(-12.0)).mean() > 0.5
    # objectness passes and the best confidence does not, somewhere: the second test of the candidate pass decides
    assert any(((x[:, 4] > 0.25) & ((x[:, 5:] * x[:, 4:5]).max(1) < 0.25)).any() for x in truth)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_references_prediction_against_the_truth(case):
    """The recorded figures are the recorded prediction's; the reference lies as close to the float64 truth as a
    numpy float32 restatement of the same steps does, by the rule decode_heads is held to."""
    heads, geom, truth = case_input(case)
    f32 = dt.decode(heads, geom, np.float32)
    assert f32.dtype == np.float32 and f32.shape == truth.shape
    own = {g: dt.errors(f32[..., s], truth[..., s]) for g, s in dt.GROUPS.items()}
    for g, (rel, worst) in case["figures"].items():
        assert 0 < rel < 4 * dt.EPS32 and rel <= max(dt.MARGIN * own[g][0], dt.FLOOR_ULPS * dt.EPS32), (g, rel, own[g])
    if case["pred_stored"]:
        pred = ARRAYS[case["name"] + "/pred"]
        assert pred.dtype == np.float32 and pred.shape == truth.shape
        for g, s in dt.GROUPS.items():
            assert list(dt.errors(pred[..., s], truth[..., s])) == case["figures"][g]
        figs = dt.pred_figures(pred, truth, own)
        assert all(f["ok"] for f in figs.values()), figs


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_references_detections_equal_the_truths(case):
    got, want = golden_dets(case), truth_dets(case)
    assert [len(d) for d in got] == case["counts"] == [len(d) for d in want]
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g[:, 5], w[:, 5])                                    # class, and with it the order:
        assert (np.diff(g[:, 4]) < 0).all() and np.abs(g[:, 4] - w[:, 4]).max() < dt.DECISION_MARGIN / 2
    g, w = np.concatenate(got), np.concatenate(want)
    assert list(dt.errors(g[:, :4], w[:, :4])) == case["det_figures"]["box"]
    assert list(dt.errors(g[:, 4], w[:, 4])) == case["det_figures"]["conf"]
    # a float32 evaluation of the same steps is the yardstick: the reference within MARGIN of it or FLOOR_ULPS
    heads, geom, truth = case_input(case)
    f32 = dt.decode(heads, geom, np.float32)
    own = np.concatenate([dt.detections_image64(x.astype(np.float64))[1] for x in f32])
    assert own.shape == w.shape
    for name, s in (("box", slice(0, 4)), ("conf", slice(4, 5))):
        f = dt.group_figures(g[:, s], w[:, s], *dt.errors(own[:, s], w[:, s]))
        assert f["ok"], (name, f)


def test_row_order_by_planted_one_hot_rows():
    """One row per (level, anchor, y, x, image) corner: where it lands in the float64 prediction is what
    Detect.forward's view / permute / cat says, and row_index() says the same."""
    strides, hw, na, nc, bs = (8, 16, 32), (64, 96), 3, 2, 2
    shapes = dt.level_shapes(hw, strides)
    assert shapes == [(8, 12), (4, 6), (2, 3)]
    corners = [(b, l, a, y, x) for b in (0, bs - 1) for l in range(3) for a in (0, na - 1)
               for y in (0, shapes[l][0] - 1) for x in (0, shapes[l][1] - 1)]
    for where in corners:
        heads, geom = dt.one_hot_head(nc, hw, bs, strides, na, [where])
        t = dt.decode(heads, geom)
        hot = np.argwhere(t[:, :, 4] > 0.5)
        b, l, a, y, x = where
        assert hot.tolist() == [[b, dt.row_index(geom, shapes, l, a, y, x)]], where
        # reference's own arithmetic of the row: sigma(8) in every column
        s = dt.sigmoid64(8.0)
        row = t[b, hot[0, 1]]
        assert np.allclose(row[:2], [(s * 2 - 0.5 + x) * strides[l], (s * 2 - 0.5 + y) * strides[l]], rtol=1e-14)
        assert np.allclose(row[2:4], (s * 2) ** 2 * geom.anchor_grid[l, a], rtol=1e-14)
    assert dt.n_rows(geom, shapes) == 378 == t.shape[1]


# ---- the Python surface ----

def _module(nl=3, na=3, nc=80):
    g = dt.geometry(nc, (8, 16, 32, 64)[:nl], na)
    return types.SimpleNamespace(anchor_grid=torch.from_numpy(g.anchor_grid.copy()).view(nl, 1, na, 1, 1, 2),
                                 anchors=torch.from_numpy(g.anchor_grid / g.stride[:, None, None]),
                                 stride=torch.from_numpy(g.stride.copy()), nc=nc, na=na, nl=nl), g


def test_geometry_from_a_stand_in_module():
    from gaussianrpg_amd.perception import DetectGeometry
    m, g = _module()
    geom = DetectGeometry.from_module(m)
    assert (geom.nl, geom.na, geom.nc, geom.no) == (3, 3, 80, 85)
    assert np.array_equal(geom.anchor_grid, g.anchor_grid) and geom.anchor_grid.max() == 373     # pixels, not / stride
    assert np.array_equal(geom.stride, [8, 16, 32])
    direct = DetectGeometry(g.anchor_grid, [8, 16, 32], 80)
    assert np.array_equal(direct.anchor_grid, geom.anchor_grid)
    assert geom.rows([torch.zeros(2, 255, 8, 12), torch.zeros(2, 255, 4, 6), torch.zeros(2, 255, 2, 3)]) == 378
    assert DetectGeometry.from_module(_module(4, 4, 1)[0]).na == 4          # nl * na = 16: the limit
    assert DetectGeometry.from_module(_module(1, 16, 1)[0]).nl == 1
    for nl, na in ((4, 5), (1, 17)):
        with pytest.raises(ValueError, match="nl \\* na <= 16"):
            DetectGeometry.from_module(_module(nl, na, 1)[0])
    with pytest.raises(ValueError, match="nl \\* na <= 16"):
        DetectGeometry(np.ones((5, 1, 2)), np.ones(5), 1)
    with pytest.raises(ValueError, match="use DetectGeometry.from_module"):
        DetectGeometry(m.anchor_grid, m.stride, 80)
    with pytest.raises(ValueError, match="nc must be a positive integer"):
        DetectGeometry(g.anchor_grid, [8, 16, 32], 0)
    with pytest.raises(ValueError, match=r"na \* \(5 \+ nc\) must be below 2\^31"):
        DetectGeometry(g.anchor_grid, [8, 16, 32], 2 ** 31 // 3)
    with pytest.raises(ValueError, match="stride positive"):
        DetectGeometry(g.anchor_grid, [8, 0, 32], 80)


def test_refusals_need_no_device():
    from gaussianrpg_amd.perception import DetectGeometry, decode_heads, detections_from_heads
    geom = DetectGeometry.from_module(_module(3, 3, 2)[0])
    good = [torch.zeros(2, 21, 8, 12), torch.zeros(2, 21, 4, 6), torch.zeros(2, 21, 2, 3)]

    def swap(i, t):
        return [t if k == i else h for k, h in enumerate(good)]
    for fn in (decode_heads, detections_from_heads):
        with pytest.raises(TypeError, match=r"head 1 must be float32 \(got torch.float16\).*pass head.float\(\)"):
            fn(swap(1, good[1].half()), geom)
        with pytest.raises(TypeError, match="head 0 must be a tensor"):
            fn(swap(0, good[0].numpy()), geom)
        with pytest.raises(TypeError, match="geom must be a DetectGeometry"):
            fn(good, None)
        with pytest.raises(ValueError, match="list of the 3 conv outputs"):
            fn(good[:2], geom)
        with pytest.raises(ValueError, match="list of the 3 conv outputs"):
            fn(good[0], geom)
        with pytest.raises(ValueError, match=r"head 2 has 24 channels, na \* \(5 \+ nc\) = 3 \* 7 = 21 expected"):
            fn(swap(2, torch.zeros(2, 24, 2, 3)), geom)
        with pytest.raises(ValueError, match=r"head 0 must be \[bs, na\*\(5\+nc\), ny, nx\]"):
            fn(swap(0, torch.zeros(2, 21, 96)), geom)
        with pytest.raises(ValueError, match="same bs .head 0 has 2, head 1 has 1"):
            fn(swap(1, torch.zeros(1, 21, 4, 6)), geom)
        with pytest.raises(ValueError, match="head 0 must be contiguous NCHW"):
            fn(swap(0, torch.zeros(2, 8, 12, 21).permute(0, 3, 1, 2)), geom)
        with pytest.raises(ValueError, match="head 1 must be contiguous NCHW"):
            fn(swap(1, torch.zeros(2, 21, 4, 6).contiguous(memory_format=torch.channels_last)), geom)
        # bs * N = 2^16 * 3 * (2^8 * 2^6) * ... >= 2^31: no memory behind it, the sizes alone are refused
        big = [torch.zeros(1, 21, 1, 1).expand(2 ** 16, 21, 2 ** 8, 2 ** 6) for _ in range(3)]
        with pytest.raises(ValueError, match=r"bs \* N must be below 2\^31"):
            fn(big, geom)
        # everything about the call is right but the device: no CPU path, no fall-back
        with pytest.raises(ValueError, match="no CPU path"):
            fn(good, geom)
    for bad in (-0.1, 1.5, NAN):
        with pytest.raises(ValueError, match="invalid confidence threshold"):
            detections_from_heads(good, geom, conf_thres=bad)
        with pytest.raises(ValueError, match="invalid IoU threshold"):
            detections_from_heads(good, geom, iou_thres=bad)
    for bad in (0, 1025, -3, 2.5):
        with pytest.raises(ValueError, match="max_det must be an integer in"):
            detections_from_heads(good, geom, max_det=bad)
    with pytest.raises(ValueError, match="max_nms must be a positive integer"):
        detections_from_heads(good, geom, max_nms=0)


def test_binding_refusals():
    from gaussianrpg_amd.rasterizer import _C
    good = [torch.zeros(1, 14, 4, 6), torch.zeros(1, 14, 2, 3)]
    ag, st = [10.0, 13, 16, 30, 30, 61, 62, 45], [8.0, 16.0]
    with pytest.raises(RuntimeError, match="head 1 must be float32"):
        _C.detect_decode([good[0], good[1].half()], ag, st, 2, 2)
    with pytest.raises(RuntimeError, match=r"head 0 must be \[bs, na\*\(5\+nc\) = 21"):
        _C.detect_decode(good, ag + [1.0, 1.0] * 2, st, 3, 2)
    with pytest.raises(RuntimeError, match="anchor_grid must hold nl \\* na \\* 2 values"):
        _C.detect_decode(good, ag[:6], st, 2, 2)
    with pytest.raises(RuntimeError, match="nl \\* na <= 16"):
        _C.detect_decode(good, ag, st, 9, 2)
    with pytest.raises(RuntimeError, match=r"na \* \(5 \+ nc\) must be below 2\^31"):
        _C.detect_decode(good, ag, st, 2, 2 ** 31 - 1)
    with pytest.raises(RuntimeError, match="2 heads expected"):
        _C.detect_detections(good[:1], ag, st, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.detect_decode(good, ag, st, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.detect_detections(good, ag, st, 2, 2)


def test_workspace_size_needs_no_device():
    lib = ctypes.CDLL(LIB)
    for f in (lib.grpg_detect_workspace_bytes, lib.grpg_nms_workspace_bytes):
        f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    sim = lib.grpg_detect_workspace_bytes(1, 107100)
    # the NMS workspace and one [N, 4] float32 box array
    assert sim % 256 == 0 and 0 <= sim - lib.grpg_nms_workspace_bytes(1, 107100) - 16 * 107100 < 256
    assert lib.grpg_detect_workspace_bytes(2, 378) >= lib.grpg_nms_workspace_bytes(2, 378) + 2 * 378 * 16
    assert lib.grpg_detect_workspace_bytes(0, 10) == 0 and lib.grpg_detect_workspace_bytes(1, 0) == 0
    assert lib.grpg_detect_workspace_bytes(2, 2 ** 30) == 0
    from gaussianrpg_amd.rasterizer import _C
    assert _C.detect_workspace_bytes(1, 107100) == sim
