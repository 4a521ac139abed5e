"""GPU tests of the fused detector-output -> detections step (gaussianrpg_amd/perception.py, csrc/nms.hip): the whole
``det`` array, zero rows included, and ``count`` bit for bit against the numpy restatement (tests/nms_truth.py), and
against what the reference's own functions returned (tests/golden/ref_nms.*, see tests/test_nms_golden.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nms_truth as nt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM, RESIZE = nt.SIM, nt.RESIZE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _plan(frame, device):
    from gaussianrpg_amd.perception import LetterboxPlan
    p = LetterboxPlan.for_simulator(frame[2], frame[3], device=device) if frame == SIM else \
        LetterboxPlan(frame[2], frame[3], 640, device=device)
    assert p.out_shape == frame[:2]
    return p


def _same(what, det, count, ref_det, ref_count):
    det, count = det.cpu().numpy(), count.cpu().numpy()
    assert det.shape == ref_det.shape and det.dtype == np.float32, (what, det.shape, ref_det.shape, det.dtype)
    assert count.dtype == np.int32 and count.tolist() == ref_count.tolist(), (what, count.tolist(), ref_count.tolist())
    bad = det.view(np.uint32) != ref_det.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %r != %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), det[bad][0], ref_det[bad][0])


def _check(dev, what, p, frame=None, **kw):
    """detections(p, **kw) on the device against the restatement; the prediction must come back unchanged."""
    from gaussianrpg_amd.perception import detections
    t = torch.from_numpy(p).to(dev)
    det, count = detections(t, plan=None if frame is None else _plan(frame, dev), **kw)
    ref = nt.detections(p, frame=frame, **kw)
    assert tuple(det.shape) == (p.shape[0], kw.get("max_det", 300), 6) and det.is_contiguous()
    _same(what, det, count, *ref)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), p.view(np.uint32)), "%s: the prediction changed" % what
    return ref


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 1000])
def test_candidate_counts_at_1000_rows(dev, n):
    p = nt.make_prediction(1000, 3, n, seed=10 + n)
    assert len(nt.candidates(p[0], 0.25)[0]) == n
    _, count = _check(dev, "%d candidates" % n, p)
    assert (count[0] > 0) == (n > 0)


def test_one_row_one_class(dev):
    p = nt.make_prediction(1, 1, 1, seed=1)
    assert _check(dev, "N=1 candidate", p)[1].tolist() == [1]
    assert _check(dev, "N=1 empty", nt.make_prediction(1, 1, 0, seed=1))[1].tolist() == [0]


@pytest.mark.parametrize("N,nc,n", [(777, 5, 200), (2049, 65, 130), (300, 130, 300)])
def test_sizes_off_every_tile(dev, N, nc, n):
    """N no multiple of the workgroup (256), the wave (64) or the sort's chunk (2048); nc above one and two waves."""
    p = nt.make_prediction(N, nc, n, seed=N)
    assert len(nt.candidates(p[0], 0.25)[0]) == n
    _check(dev, "N=%d nc=%d" % (N, nc), p)


def test_yolov5_640_head(dev):
    p = nt.make_prediction(25200, 80, 300, seed=2)
    assert len(nt.candidates(p[0], 0.25)[0]) == 300
    _check(dev, "N=25200", p)


def test_simulator_head_with_its_plan(dev):
    """The simulator's own size: 1600 x 1088 input, N = 107 100, about 3000 candidates, max_det = 10, mapped back to
    the 1066 x 1600 frame; and the same prediction unmapped at the default max_det."""
    p = nt.make_prediction(107100, 80, 3000, seed=3, size=(1088, 1600), grid=0.5)
    assert len(nt.candidates(p[0], 0.25)[0]) == 3000
    _check(dev, "N=107100 simulator", p, frame=SIM, max_det=10)
    _, count = _check(dev, "N=107100", p)
    assert count.tolist() == [300]


def test_more_keeps_than_max_det(dev):
    p = nt.make_prediction(1000, 3, 400, seed=4)
    full = nt.detections(p, max_det=1024)
    assert 10 < full[1][0] < 1024
    det, count = _check(dev, "max_det=10", p, max_det=10)
    assert count.tolist() == [10] and np.array_equal(det[0], full[0][0, :10])
    _check(dev, "max_det=1", p, max_det=1)
    _check(dev, "max_det=1024 not reached", p, max_det=1024)


def test_max_det_1024_reached(dev):
    p = nt.make_prediction(4000, 3, 3000, seed=5, size=(6000, 6000))
    _, count = _check(dev, "max_det=1024", p, max_det=1024)
    assert count.tolist() == [1024]


def test_more_candidates_than_max_nms(dev):
    p = nt.make_prediction(1000, 3, 300, seed=6)
    det, count = _check(dev, "max_nms=100", p, max_nms=100, max_det=1024)
    assert 0 < count[0] <= 100
    assert count[0] < nt.detections(p, max_det=1024)[1][0]
    _check(dev, "max_nms=1", p, max_nms=1)


def test_two_images_one_empty(dev):
    for n_cand in ([200, 0], [0, 200], [150, 70]):
        p = nt.make_prediction(1000, 3, n_cand, seed=7, bs=2)
        _, count = _check(dev, "bs=2 %s" % n_cand, p)
        assert [c > 0 for c in count.tolist()] == [n > 0 for n in n_cand]
    _check(dev, "bs=3 odd N", nt.make_prediction(333, 2, [5, 100, 64], seed=8, bs=3))


@pytest.mark.parametrize("agnostic", [False, True])
def test_agnostic_and_class_filter(dev, agnostic):
    p = nt.make_prediction(1000, 4, 500, seed=9, clusters=12, jitter=10.0)
    a = _check(dev, "agnostic=%d" % agnostic, p, agnostic=agnostic)
    b = _check(dev, "classes", p, agnostic=agnostic, classes=[0, 2])
    assert set(b[0][0, :b[1][0], 5].tolist()) == {0.0, 2.0} and b[1][0] < a[1][0]
    _check(dev, "classes none of the head's", p, agnostic=agnostic, classes=[7])
    if agnostic:
        assert a[1][0] < nt.detections(p, agnostic=False)[1][0]      # the same boxes in several classes


def test_nan_rows_and_ties(dev):
    x = nt.nan_case()
    det, count = _check(dev, "NaN rows", x[None])
    assert count.tolist() == [2] and np.isnan(det[0, 0, 0])
    _check(dev, "NaN rows mapped", x[None], frame=SIM)
    t = nt.tie_case()
    det, _ = _check(dev, "ties", t[None], agnostic=True)
    assert det[0, :2, :4].tolist() == [[100, 100, 110, 110], [0, 0, 10, 10]] and det[0, 1, 5] == 0
    det, _ = _check(dev, "ties swapped", t[::-1].copy()[None], agnostic=True)
    assert det[0, 1, :4].tolist() == [1, 0, 11, 10]
    # many equal confidences across several 64-candidate blocks and sort chunks: the order is the rows'
    p = nt.make_prediction(5000, 3, 700, seed=11)
    rows = nt.candidates(p[0], 0.25)[0]
    p[0, rows, 4] = np.float32(0.75)
    p[0, rows, 5:] = np.float32(0.5)
    p[0, rows[::3], 4] = np.float32(0.875)
    det, count = _check(dev, "700 candidates, two confidences", p, max_det=1024)
    assert set(det[0, :count[0], 5].tolist()) == {0.0} and len(set(det[0, :count[0], 4].tolist())) == 2
    # the threshold itself: IoU exactly 0.5
    e = nt.rows_of((0, 0, 2, 2, 0.9, 1.0), (0, 0, 2, 1, 0.8, 1.0))
    assert _check(dev, "iou == thres", e[None], iou_thres=0.5)[1].tolist() == [2]
    assert _check(dev, "iou > thres", e[None], iou_thres=0.49)[1].tolist() == [1]
    c = nt.rows_of((0, 0, 10, 10, 0.9, 1.0), (0, 0, 10, 6, 0.8, 1.0), (0, 0, 10, 3.5, 0.7, 1.0))
    assert _check(dev, "chain", c[None])[1].tolist() == [2]


def test_heavy_overlap(dev):
    p = nt.make_prediction(2000, 3, 500, seed=12, clusters=5, jitter=4.0)
    _, count = _check(dev, "500 around 5", p)
    assert 5 <= count[0] < 60
    _check(dev, "500 around 5, agnostic, strict", p, agnostic=True, iou_thres=0.9, max_det=1024)
    _check(dev, "500 around 5, loose", p, iou_thres=0.0, conf_thres=0.0)


@pytest.mark.parametrize("frame", [SIM, RESIZE], ids=["simulator-plan", "resizing-plan"])
def test_mapped_to_the_frame(dev, frame):
    h, w = frame[:2]
    p = nt.make_prediction(3000, 3, 400, seed=13, size=(h, w), grid=0.5)       # halves: values that land on .5
    rows = nt.candidates(p[0], 0.25)[0]
    p[0, rows[:40], 0] += w                                                     # boxes beyond the frame: clamped
    p[0, rows[40:80], 1] -= h
    det, count = _check(dev, "mapped", p, frame=frame, max_det=1024)
    d = det[0, :count[0], :4]
    assert np.array_equal(d, np.rint(d)) and d.min() == 0 and d[:, [0, 2]].max() == frame[3]
    unmapped = nt.detections(p, max_det=1024)
    assert np.array_equal(det[0, :, 4:], unmapped[0][0, :, 4:]) and not np.array_equal(det[0], unmapped[0][0])


def test_out_given_and_side_stream(dev):
    from gaussianrpg_amd.perception import detections
    p = nt.make_prediction(1000, 3, 200, seed=14, bs=2)
    ref = nt.detections(p, max_det=50)
    t = torch.from_numpy(p).to(dev)
    det = torch.full((2, 50, 6), float("nan"), device=dev)
    count = torch.full((2,), -7, dtype=torch.int32, device=dev)
    r = detections(t, max_det=50, out=(det, count))
    assert r[0] is det and r[1] is count
    _same("out=", det, count, *ref)
    with pytest.raises(RuntimeError, match="out det must be a contiguous float32"):
        detections(t, max_det=60, out=(det, count))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        det2, count2 = detections(t, max_det=50)
    s.synchronize()
    _same("side stream", det2, count2, *ref)


def test_two_calls_give_identical_bytes(dev):
    from gaussianrpg_amd.perception import detections
    p = nt.make_prediction(25200, 80, 600, seed=15, clusters=20, jitter=12.0)
    t = torch.from_numpy(p).to(dev)
    a = detections(t, classes=[0, 1, 2, 3, 4, 5, 6, 7])
    b = detections(t, classes=[0, 1, 2, 3, 4, 5, 6, 7])
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert int(a[1][0]) > 0


def test_non_max_suppression_lists(dev):
    from gaussianrpg_amd.perception import non_max_suppression
    p = nt.make_prediction(1000, 3, [200, 0, 30], seed=16, bs=3)
    t = torch.from_numpy(p).to(dev)
    for kw in (dict(), dict(conf_thres=0.4, iou_thres=0.6, classes=[1], agnostic=True, max_det=7)):
        out = non_max_suppression((t, None) if kw else t, **kw)
        assert isinstance(out, list) and len(out) == 3
        for b in range(3):
            ref = nt.detections_image(p[b], **kw)
            got = out[b].cpu().numpy()
            assert got.shape == ref.shape and got.shape[1] == 6
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert out[1].shape == (0, 6)


@pytest.mark.parametrize("frame", [SIM, RESIZE], ids=["simulator-plan", "resizing-plan"])
def test_simulator_detections_fused_equals_the_torch_route(dev, frame):
    from gaussianrpg_amd import harness as hz
    h, w = frame[:2]
    p = nt.make_prediction(3000, 80, [300, 0], seed=17, size=(h, w), clusters=15, jitter=10.0, bs=2)
    for b in range(2):
        rows, conf, _ = nt.candidates(p[b], 0.25)
        assert len(np.unique(conf)) == len(conf)                    # no two candidates tie
        cj = np.sort(p[b, rows, 5:] * p[b, rows, 4:5], axis=1)
        assert (cj[:, -1] > cj[:, -2]).all()                        # and no row has two best classes
    t = torch.from_numpy(p).to(dev)
    plan = _plan(frame, dev)
    for kw in (dict(), dict(max_det=300, agnostic=True), dict(classes=[0, 1, 2])):
        fused = hz.simulator_detections(t, plan, fused=True, **kw)
        plain = hz.simulator_detections(t, plan, fused=False, **kw)
        assert len(fused) == len(plain) == 2 and fused[1].shape == plain[1].shape == (0, 6)
        assert fused[0].shape == plain[0].shape and fused[0].shape[0] > 0
        assert torch.equal(fused[0].view(torch.int32), plain[0].view(torch.int32))
        ref = nt.detections_image(p[0], frame=frame, **dict(dict(max_det=10), **kw))
        assert np.array_equal(fused[0].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(t.cpu().numpy(), p)


def test_c_abi_directly(dev):
    """ctypes and grpg_nms_detections, no _C: torch only allocates."""
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_nms_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_nms_detections.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                        ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    p = nt.make_prediction(700, 4, 150, seed=18, bs=2)
    t = torch.from_numpy(p).to(dev)
    nbytes = lib.grpg_nms_workspace_bytes(2, 700)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    allow = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=dev)
    det, count = torch.empty(2, 20, 6, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    fmap = (ctypes.c_double * 6)(*([float(v) for v in RESIZE] + list(nt.frame_map(*RESIZE)[1:])))
    torch.cuda.synchronize()

    def call(**o):
        a = dict(pred=t.data_ptr(), bs=2, N=700, nc=4, conf=0.25, iou=0.45, allow=allow.data_ptr(), agnostic=0,
                 max_det=20, max_nms=30000, ws=ws.data_ptr(), nbytes=nbytes)
        a.update(o)
        return lib.grpg_nms_detections(a["pred"], a["bs"], a["N"], a["nc"], a["conf"], a["iou"], a["allow"],
                                       a["agnostic"], a["max_det"], a["max_nms"], 7680.0, ctypes.addressof(fmap),
                                       a["ws"], a["nbytes"], det.data_ptr(), count.data_ptr(), None)
    assert call() == 0, lib.grpg_last_error()
    torch.cuda.synchronize()
    _same("C ABI", det, count, *nt.detections(p, classes=[0, 2, 3], max_det=20, frame=RESIZE))
    # the argument errors: all before any launch
    assert call(nbytes=nbytes - 1) == -1 and b"workspace smaller" in lib.grpg_last_error()
    assert call(ws=ws.data_ptr() + 4) == -1 and b"256-byte aligned" in lib.grpg_last_error()
    assert call(max_det=1025) == -1 and b"max_det" in lib.grpg_last_error()
    assert call(max_det=0) == -1
    assert call(conf=1.5) == -1 and b"[0, 1]" in lib.grpg_last_error()
    assert call(iou=float("nan")) == -1
    assert call(nc=0) == -1 and call(N=0) == -1 and call(bs=0) == -1
    assert call(bs=2, N=2 ** 30) == -1 and b"2^31" in lib.grpg_last_error()
    assert call(pred=None) == -1 and call(max_nms=0) == -1


# ---- against the reference's own output (tests/golden/ref_nms.*), not through the restatement ----

def _golden_cases():
    from test_nms_golden import CASES
    return CASES


@pytest.mark.parametrize("case", _golden_cases(), ids=[c["name"] for c in _golden_cases()])
def test_detections_equal_the_references_own_output(dev, case):
    """perception.detections against what the reference's non_max_suppression (and, with a frame, its
    scale_coords(...).round()) returned for the same input: the whole det array -- the golden's rows, then zeros --
    and count, bit for bit; the prediction comes back unchanged.  Batches also through non_max_suppression's lists."""
    from gaussianrpg_amd.perception import detections, non_max_suppression
    from test_nms_golden import case_frame, case_input, golden_rows
    p, frame, kw = case_input(case), case_frame(case), case["settings"]
    bs, max_det = p.shape[0], kw.get("max_det", 300)
    want = np.zeros((bs, max_det, 6), np.float32)
    for b in range(bs):
        rows = golden_rows(case, b, mapped=frame is not None)
        assert len(rows) == case["counts"][b] <= max_det
        want[b, :len(rows)] = rows
    t = torch.from_numpy(p.copy()).to(dev)
    det, count = detections(t, plan=None if frame is None else _plan(frame, dev), **kw)
    assert tuple(det.shape) == (bs, max_det, 6) and det.is_contiguous()
    _same(case["name"], det, count, want, np.asarray(case["counts"], np.int32))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), p.view(np.uint32)), "%s: the prediction changed" % case["name"]
    if bs > 1:
        out = non_max_suppression(t, **kw)
        assert isinstance(out, list) and len(out) == bs
        for b in range(bs):
            got, ref = out[b].cpu().numpy(), golden_rows(case, b, mapped=False)
            assert got.shape == ref.shape and got.dtype == np.float32, (b, got.shape, ref.shape)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "%s: list %d differs" % (case["name"], b)
