"""CPU tests (-m "not gpu") of the detector-output -> detections step (gaussianrpg_amd/perception.py, csrc/nms.hip):
hand-worked cases through the numpy restatement (tests/nms_truth.py), the restatement's float32 arithmetic against a
float64 evaluation of the same rule where float32 is exact, its frame mapping against the reference's scale_coords
arithmetic, its greedy step against torchvision.ops.nms where torchvision is installed, the refusals of the Python
surface, and the C entries without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nms_truth as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
NAN = float("nan")


rows_of = nt.rows_of


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the libamdhip64 the library links)
    lib = ctypes.CDLL(LIB)
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_nms_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_nms_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


# ---- hand-worked cases ----

def test_chain_b_is_suppressed_so_c_lives():
    """A = [0,0,10,10], B = [0,0,10,6] (IoU with A 0.6), C = [0,0,10,3.5] (IoU with A 0.35, with B 0.583): B falls to
    A, and C -- which only B would have suppressed -- is kept."""
    x = rows_of((0, 0, 10, 10, 0.9, 1.0), (0, 0, 10, 6, 0.8, 1.0), (0, 0, 10, 3.5, 0.7, 1.0))
    d = nt.detections_image(x, 0.25, 0.45)
    assert d[:, :4].tolist() == [[0, 0, 10, 10], [0, 0, 10, 3.5]]
    assert d[:, 4].tolist() == [np.float32(0.9), np.float32(0.7)] and d[:, 5].tolist() == [0, 0]
    # without A, B is kept and suppresses C
    assert nt.detections_image(x[1:], 0.25, 0.45)[:, :4].tolist() == [[0, 0, 10, 6]]


def test_iou_exactly_at_the_threshold_is_not_suppressed():
    x = rows_of((0, 0, 2, 2, 0.9, 1.0), (0, 0, 2, 1, 0.8, 1.0))
    a = nt.xywh2xyxy(x[:, :4])
    assert nt.iou(a[:1], nt.area_of(a[:1]), a[1], nt.area_of(a[1]))[0] == np.float32(0.5)
    assert len(nt.detections_image(x, 0.25, 0.5)) == 2
    assert len(nt.detections_image(x, 0.25, 0.49)) == 1


def test_same_box_in_two_classes():
    x = rows_of((10, 10, 50, 50, 0.9, 1.0, 0.1), (10, 10, 50, 50, 0.8, 0.1, 1.0), nc=2)
    d = nt.detections_image(x, 0.25, 0.45)
    assert len(d) == 2 and d[:, 5].tolist() == [0, 1]
    assert np.array_equal(d[0, :4], d[1, :4])                      # the output boxes are not shifted
    d = nt.detections_image(x, 0.25, 0.45, agnostic=True)
    assert len(d) == 1 and d[0, 5] == 0
    d = nt.detections_image(x, 0.25, 0.45, classes=[1])
    assert len(d) == 1 and d[0, 5] == 1 and d[0, 4] == np.float32(0.8)


def test_equal_confidences_resolve_by_row_and_equal_scores_by_class():
    x = nt.tie_case()     # rows 0 and 2 tie at 0.5 and overlap: the lower row wins; row 1 is better
    d = nt.detections_image(x, 0.25, 0.45, agnostic=True)
    assert d[:, :4].tolist() == [[100, 100, 110, 110], [0, 0, 10, 10]]
    assert d[1, 5] == 0                                            # both class scores 1.0: the lowest class
    rows, conf, cls = nt.candidates(x, 0.25)
    assert rows.tolist() == [0, 1, 2] and cls.tolist() == [0, 0, 1]
    # swapped rows: now the other box is first
    d = nt.detections_image(x[::-1].copy(), 0.25, 0.45, agnostic=True)
    assert d[:, :4].tolist() == [[100, 100, 110, 110], [1, 0, 11, 10]]


def test_nan_rows():
    x = nt.nan_case()
    d = nt.detections_image(x, 0.25, 0.45)
    assert d[:, 4].tolist() == [np.float32(0.8), np.float32(0.7)]
    assert np.isnan(d[0, 0]) and np.isnan(d[0, 2]) and d[0, 1] == 0 and d[0, 3] == 10
    assert d[1, :4].tolist() == [40, 0, 50, 10]
    # 0 / 0: two empty boxes at one point have IoU NaN -- nothing is suppressed
    z = rows_of((5, 5, 5, 5, 0.9, 1.0), (5, 5, 5, 5, 0.8, 1.0))
    assert len(nt.detections_image(z, 0.25, 0.45)) == 2


def test_limits_max_det_and_max_nms():
    x = nt.make_prediction(400, 3, 200, seed=3)[0]
    full = nt.detections_image(x, max_det=1024)
    assert 20 < len(full) <= 200
    assert np.array_equal(nt.detections_image(x, max_det=10), full[:10])      # stopping early changes nothing
    few = nt.detections_image(x, max_det=1024, max_nms=50)
    rows, conf, _ = nt.candidates(x, 0.25)
    assert len(few) <= 50 and few[:, 4].min() >= np.sort(conf)[-50]
    det, count = nt.detections(x[None], max_det=10)
    assert det.shape == (1, 10, 6) and count.tolist() == [10] and det.dtype == np.float32


# ---- float32 against float64 where float32 is exact ----

@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("agnostic", [False, True])
def test_float32_kept_sets_equal_float64_on_exact_inputs(seed, agnostic):
    """Coordinates on multiples of 1/4 with sides <= 512 and nc <= 80: corners, shifted corners (below 2^20, a
    multiple of 1/4), differences, areas and intersections (multiples of 1/16 below 2^19) are exact in float32; only
    the final division rounds, and a correctly rounded quotient compares with the float32 threshold like the exact
    one unless the exact one lies within an ulp of it -- none of these seeds does."""
    rng = np.random.RandomState(seed)
    n, nc = 300, 80
    x = np.zeros((n, 5 + nc), np.float32)
    base = rng.randint(0, 8, n)
    x[:, 0] = (base % 4) * 300 + 256 + rng.randint(-40, 41, n) / 4.0
    x[:, 1] = (base // 4) * 300 + 256 + rng.randint(-40, 41, n) / 4.0
    x[:, 2:4] = rng.randint(8, 1025, (n, 2)) / 2.0          # sides: multiples of 1/2, so half sides of 1/4; <= 512
    x[:, 4] = rng.uniform(0.5, 1.0, n)
    x[np.arange(n), 5 + rng.choice([0, 7, 79], n)] = rng.uniform(0.6, 1.0, n)
    rows32 = nt.candidates(x, 0.25)[0]
    d = nt.detections_image(x, 0.25, 0.45, agnostic=agnostic, max_det=1024)
    rows64 = nt.kept_sets_float64(x, 0.25, 0.45, agnostic=agnostic)
    assert len(rows32) == n and 8 <= len(d) < n
    box = nt.xywh2xyxy(x[rows64, :4])
    assert np.array_equal(d[:, :4], box)
    assert np.array_equal(d[:, 4], (x[rows64, 5:] * x[rows64, 4:5]).max(1))


# ---- the frame mapping ----

def _scale_coords_float32(boxes, h, w, H, W):
    """scale_coords(...).round() of utils/torch_utils.py:501-547 line by line, on a float32 array."""
    gain = min(h / H, w / W)
    pad = (w - W * gain) / 2, (h - H * gain) / 2
    c = boxes.astype(np.float32).copy()
    c[:, [0, 2]] -= np.float32(pad[0])
    c[:, [1, 3]] -= np.float32(pad[1])
    c[:, :4] /= np.float32(gain)
    c[:, 0].clip(0, W, out=c[:, 0])
    c[:, 1].clip(0, H, out=c[:, 1])
    c[:, 2].clip(0, W, out=c[:, 2])
    c[:, 3].clip(0, H, out=c[:, 3])
    return np.round(c)                                  # half to even, like torch.round


@pytest.mark.parametrize("h,w,H,W", [(1088, 1600, 1066, 1600), (224, 640, 375, 1242)],
                         ids=["simulator", "resizing"])
def test_frame_mapping_equals_scale_coords(h, w, H, W):
    rng = np.random.RandomState(5)
    b = rng.uniform(-50, max(h, w) + 50, (400, 4)).astype(np.float32)
    gain, pad_x, pad_y = nt.frame_map(h, w, H, W)
    # values that land on .5 after the mapping: (k + .5) * gain + pad, both parities of k, where float32 holds them
    k = np.arange(0, 40, dtype=np.float64)
    b[:40, 0] = ((k + 0.5) * gain + pad_x).astype(np.float32)
    b[:40, 1] = ((k + 0.5) * gain + pad_y).astype(np.float32)
    got = nt.to_frame(b, h, w, H, W)
    assert np.array_equal(got, _scale_coords_float32(b, h, w, H, W))
    assert got.min() == 0 and got[:, [0, 2]].max() == W and got[:, [1, 3]].max() == H
    if gain == 1.0:
        assert pad_x == 0 and pad_y == 11
        assert got[:40, 1].tolist() == [float(np.round(v + 0.5)) for v in k]      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    det = nt.detections_image(rows_of((10, 20.5, 50, 61.5, 0.9, 1.0)), frame=(h, w, H, W))
    assert np.array_equal(det[:, :4], _scale_coords_float32(np.float32([[10, 20.5, 50, 61.5]]), h, w, H, W))


def test_plan_frame_map_is_scale_coords_own():
    from gaussianrpg_amd.perception import LetterboxPlan, frame_map
    p = LetterboxPlan.for_simulator(1066, 1600)
    assert frame_map(p) == (1088.0, 1600.0, 1066.0, 1600.0, 0.0, 11.0)
    p = LetterboxPlan(375, 1242, 640)
    h, w, H, W, px, py = frame_map(p)
    assert (h, w, H, W) == (224.0, 640.0, 375.0, 1242.0)
    assert (min(h / H, w / W), px, py) == nt.frame_map(224, 640, 375, 1242)


# ---- torchvision, where it is installed ----

def test_greedy_step_equals_torchvision_nms():
    tv = pytest.importorskip("torchvision")
    x = nt.make_prediction(600, 1, 300, seed=7, clusters=6, jitter=20.0)[0]
    rows, conf, cls = nt.candidates(x, 0.25)
    order = np.argsort(-conf, kind="stable")
    boxes = nt.xywh2xyxy(x[rows[order], :4])
    assert len(np.unique(conf)) == len(conf)
    ref = tv.ops.nms(torch.from_numpy(boxes), torch.from_numpy(conf[order].copy()), 0.45).numpy()
    assert np.array_equal(nt.greedy_nms(boxes, 0.45), ref)


# ---- the Python surface refuses before any device use ----

def test_refusals():
    from gaussianrpg_amd.perception import detections, non_max_suppression
    good = torch.zeros(1, 8, 7)
    for fn in (detections, non_max_suppression):
        with pytest.raises(TypeError, match="prediction must be float32"):
            fn(good.half())
        with pytest.raises(TypeError, match="prediction must be float32"):
            fn(good.double())
        with pytest.raises(TypeError, match="prediction must be a tensor"):
            fn(good.numpy())
        with pytest.raises(ValueError, match=r"prediction must be \[bs, N, 5 \+ nc\]"):
            fn(good[0])
        with pytest.raises(ValueError, match=r"prediction must be \[bs, N, 5 \+ nc\]"):
            fn(torch.zeros(1, 8, 5))
        with pytest.raises(ValueError, match="prediction must be contiguous"):
            fn(torch.zeros(1, 7, 8).transpose(1, 2))
        for bad in (-0.1, 1.5, NAN):
            with pytest.raises(ValueError, match="invalid confidence threshold"):
                fn(good, conf_thres=bad)
            with pytest.raises(ValueError, match="invalid IoU threshold"):
                fn(good, iou_thres=bad)
        for bad in (0, 1025, -3, 2.5):
            with pytest.raises(ValueError, match="max_det must be an integer in"):
                fn(good, max_det=bad)
    with pytest.raises(ValueError, match="max_nms must be a positive integer"):
        detections(good, max_nms=0)
    with pytest.raises(ValueError, match="multi_label=True is not supported"):
        non_max_suppression(good, multi_label=True)
    with pytest.raises(ValueError, match="labels .* are not supported"):
        non_max_suppression(good, labels=[torch.zeros(1, 5)])
    with pytest.raises(ValueError, match="nm > 0"):
        non_max_suppression(good, nm=32)
    with pytest.raises(TypeError, match="prediction must be float32"):
        non_max_suppression((good.half(), None))                # the tuple form is unpacked first
    # everything about the call is right but the device: no CPU path, no fall-back
    with pytest.raises(RuntimeError, match="no CPU path"):
        detections(good)
    with pytest.raises(RuntimeError, match="no CPU path"):
        non_max_suppression((good, None))


def test_binding_refusals():
    from gaussianrpg_amd.rasterizer import _C
    good = torch.zeros(1, 8, 7)
    with pytest.raises(RuntimeError, match="prediction must be float32"):
        _C.nms_detections(good.half())
    with pytest.raises(RuntimeError, match="must be contiguous"):
        _C.nms_detections(torch.zeros(1, 7, 8).transpose(1, 2))
    with pytest.raises(RuntimeError, match=r"max_det must lie in \[1, 1024\]"):
        _C.nms_detections(good, max_det=2000)
    with pytest.raises(RuntimeError, match=r"must lie in \[0, 1\]"):
        _C.nms_detections(good, conf_thres=1.5)
    with pytest.raises(RuntimeError, match="frame_map must be empty or"):
        _C.nms_detections(good, frame_map=[1.0, 2.0])
    with pytest.raises(RuntimeError, match="out det must be a contiguous float32"):
        _C.nms_detections(good, det_out=torch.zeros(1, 300, 5))
    with pytest.raises(RuntimeError, match="out count must be a contiguous int32"):
        _C.nms_detections(good, count_out=torch.zeros(1))


# ---- the C entries ----

def test_workspace_size_needs_no_device_and_grows_with_the_rows_only(lib):
    small, sim = lib.grpg_nms_workspace_bytes(1, 1000), lib.grpg_nms_workspace_bytes(1, 107100)
    assert 0 < small < sim < 64 * 107100                  # a few words per row, no N x N mask
    assert lib.grpg_nms_workspace_bytes(2, 107100) < 2 * sim + 4096
    assert sim % 256 == 0
    assert lib.grpg_nms_workspace_bytes(0, 10) == 0 and lib.grpg_nms_workspace_bytes(1, 0) == 0
    assert lib.grpg_nms_workspace_bytes(2, 2 ** 30) == 0   # bs * N >= 2^31 is refused
    from gaussianrpg_amd.rasterizer import _C
    assert _C.nms_workspace_bytes(1, 107100) == sim


def test_device_entry_fails_loudly_without_a_device(lib):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib.grpg_nms_detections.restype = ctypes.c_int
    lib.grpg_nms_detections.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                        ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.grpg_nms_detections(None, 1, 8, 2, 0.25, 0.45, None, 0, 300, 30000, 7680.0, None, None, 0, None, None,
                                   None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
