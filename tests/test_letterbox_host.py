"""CPU tests (-m "not gpu") of the frame -> detector-input hand-off (gaussianrpg_amd/perception.py,
csrc/letterbox.hip): the geometry against what the reference's letterbox() gives (tests/golden/ref_letterbox.json,
written by tests/golden/make_golden_letterbox.py), the host-built resize tables against the numpy restatement, the
restatement against the float64 bilinear (what stands in for cv2, which is not part of this stack) and against cv2
itself where it is installed, the box mapping, and the argument errors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import letterbox_truth as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
with open(os.path.join(ROOT, "tests", "golden", "ref_letterbox.json")) as _f:
    CASES = json.load(_f)["cases"]

# (H, W, new_h, new_w): downscale, upscale, non-uniform, and the sizes of the issue's own check
RESIZES = [(1280, 1920, 427, 640), (375, 1242, 193, 640), (37, 53, 45, 64), (5, 7, 13, 20), (96, 160, 38, 64),
           (37, 53, 40, 72), (64, 48, 31, 100)]


def _case_id(r):
    return "%dx%d-%s-a%d-f%d-u%d-s%d" % (r["height"], r["width"], r["new_shape"], r["auto"], r["scaleFill"],
                                         r["scaleup"], r["stride"])


def _new_shape(r):
    return r["new_shape"] if isinstance(r["new_shape"], int) else tuple(r["new_shape"])


def _expected_geometry(r):
    rw = r["resized_wh"]
    new_h, new_w = (rw[1], rw[0]) if rw else (r["height"], r["width"])   # cv2.resize is skipped when nothing changes
    return [new_h, new_w] + r["border"] + r["out_shape"]


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the libamdhip64 the library links)
    lib = ctypes.CDLL(LIB)
    lib.grpg_last_error.restype = ctypes.c_char_p
    return lib


def test_the_golden_file_covers_the_ground():
    assert len(CASES) >= 30
    assert {(r["auto"], r["scaleFill"], r["scaleup"]) for r in CASES} >= {
        (a, f, u) for a in (False, True) for f in (False, True) for u in (False, True)}
    assert {r["stride"] for r in CASES} >= {32, 64}
    assert any(isinstance(r["new_shape"], list) for r in CASES) and any(isinstance(r["new_shape"], int) for r in CASES)
    sim = {(r["height"], r["width"]): r for r in CASES if r["new_shape"] == r["width"] and r["stride"] == 32}
    assert sim[(1066, 1600)]["border"] == [11, 11, 0, 0] and sim[(1066, 1600)]["out_shape"] == [1088, 1600]
    assert sim[(1280, 1920)]["border"] == [0, 0, 0, 0] and sim[(1280, 1920)]["resized_wh"] is None


@pytest.mark.parametrize("r", CASES, ids=_case_id)
def test_c_geometry_equals_the_reference(lib, r):
    ns = _new_shape(r)
    nh, nw = (ns, ns) if isinstance(ns, int) else ns
    out = (ctypes.c_int * 8)()
    rc = lib.grpg_letterbox_geometry(r["height"], r["width"], nh, nw, int(r["auto"]), int(r["scaleFill"]),
                                     int(r["scaleup"]), r["stride"], out)
    assert rc == 0, lib.grpg_last_error()
    assert list(out) == _expected_geometry(r)


@pytest.mark.parametrize("r", CASES, ids=_case_id)
def test_plan_equals_the_reference(r):
    from gaussianrpg_amd.perception import LetterboxPlan
    p = LetterboxPlan(r["height"], r["width"], _new_shape(r), auto=r["auto"], scale_fill=r["scaleFill"],
                      scaleup=r["scaleup"], stride=r["stride"])
    g = _expected_geometry(r)
    assert list(p.resized) == g[0:2] and list(p.pad) == g[2:6] and list(p.out_shape) == g[6:8]
    assert p.geometry == g
    assert p.needs_resize == (r["resized_wh"] is not None)
    # float64, bit for bit
    assert [float(v) for v in p.ratio] == r["ratio"]
    assert [float(v) for v in p.dwdh] == r["dwdh"]


def test_for_simulator_is_the_imgsz_equals_width_case():
    from gaussianrpg_amd.perception import LetterboxPlan
    p = LetterboxPlan.for_simulator(1066, 1600)
    assert p.resized == (1066, 1600) and p.pad == (11, 11, 0, 0) and p.out_shape == (1088, 1600)
    assert not p.needs_resize and p.tables("cpu") == (None, None)
    q = LetterboxPlan.for_simulator(1280, 1920, stride=64)
    assert q.pad == (0, 0, 0, 0) and q.out_shape == (1280, 1920)


def test_geometry_rejects_bad_arguments(lib):
    out = (ctypes.c_int * 8)()
    assert lib.grpg_letterbox_geometry(0, 64, 64, 64, 1, 0, 1, 32, out) == -1
    assert b"positive" in lib.grpg_last_error()
    assert lib.grpg_letterbox_geometry(48, 64, 64, 64, 1, 0, 1, 0, out) == -1
    assert b"stride" in lib.grpg_last_error()
    assert lib.grpg_letterbox_geometry(48, 64, 64, 64, 1, 0, 1, 32, None) == -1
    assert lib.grpg_letterbox_tables(48, 64, 24, 32, None, None) == -1
    assert lib.grpg_letterbox_tables(48, 64, 0, 32, out, out) == -1


@pytest.mark.parametrize("H,W,nh,nw", RESIZES + [(5, 7, 1, 1), (1, 1, 3, 5), (2, 9, 2, 31)])
def test_c_tables_equal_the_restatement(lib, H, W, nh, nw):
    """Host only, no device: entry for entry, the clamped first and last columns and rows included."""
    xt, yt = (ctypes.c_int * (2 * nw))(), (ctypes.c_int * (2 * nh))()
    assert lib.grpg_letterbox_tables(H, W, nh, nw, xt, yt) == 0, lib.grpg_last_error()
    assert np.array_equal(np.array(xt, np.int32).reshape(nw, 2), lt.packed_table(W, nw))
    assert np.array_equal(np.array(yt, np.int32).reshape(nh, 2), lt.packed_table(H, nh))
    from gaussianrpg_amd.rasterizer import _C
    bx, by = _C.letterbox_tables(H, W, nh, nw)
    assert bx.dtype == torch.int32 and not bx.is_cuda and tuple(bx.shape) == (nw, 2) and tuple(by.shape) == (nh, 2)
    assert np.array_equal(bx.numpy(), lt.packed_table(W, nw)) and np.array_equal(by.numpy(), lt.packed_table(H, nh))
    s, a0, a1 = lt.axis_table(W, nw)
    assert s.min() >= 0 and s.max() <= W - 1 and (np.abs(a0 + a1 - 2048) <= 1).all()
    if nw > W:   # upscale: the first and the last column are clamped onto a sample
        assert (s[0], a0[0], a1[0]) == (0, 2048, 0) and (s[-1], a0[-1], a1[-1]) == (W - 1, 2048, 0)


@pytest.mark.parametrize("H,W,nh,nw", RESIZES)
def test_restatement_stays_below_one_grey_level_of_the_float64_bilinear(H, W, nh, nw):
    """What stands in for cv2: the float64 bilinear of the same bytes with half-pixel centres."""
    for name, im in lt.images(H, W, seed=H + W).items():
        got = lt.resize(im, nh, nw).astype(np.float64)
        ref = F.interpolate(torch.from_numpy(im).permute(2, 0, 1)[None].double(), size=(nh, nw), mode="bilinear",
                            align_corners=False)[0].permute(1, 2, 0).numpy()
        err = np.abs(got - ref).max()
        print("%dx%d -> %dx%d %s: max |restatement - float64 bilinear| = %.4f grey levels" % (H, W, nh, nw, name, err))
        assert err < 1.0, (name, err)


@pytest.mark.parametrize("H,W,nh,nw", RESIZES)
def test_restatement_equals_cv2(H, W, nh, nw):
    """Settles the open question wherever cv2 is installed (the exact-1/2 area case is not among RESIZES)."""
    cv2 = pytest.importorskip("cv2")
    for name, im in lt.images(H, W, seed=H + W).items():
        ref = cv2.resize(im, (nw, nh), interpolation=cv2.INTER_LINEAR)
        assert np.array_equal(lt.resize(im, nh, nw), ref), name


def test_host_route_of_the_package_equals_the_restatement():
    """perception.letterbox_host (the cv2 stand-in of harness.simulator_perception_frame(fused=False)) from the
    library's tables == the restatement from its own."""
    from gaussianrpg_amd import perception as pc
    for H, W, ns, kw in [(37, 53, 64, {}), (96, 160, 64, {}), (48, 64, 640, dict(auto=False, scaleup=False)),
                         (37, 53, (40, 72), dict(auto=False, scale_fill=True)), (40, 64, 64, {})]:
        p = pc.LetterboxPlan(H, W, ns, **kw)
        for name, im in lt.images(H, W, seed=5).items():
            got = pc.letterbox_host(im, p)
            assert got.shape == p.out_shape + (3,) and got.dtype == np.uint8
            assert np.array_equal(got, lt.letterbox(im, p.resized, p.pad)), (H, W, ns, name)


def test_to_frame_against_float64_scale_and_clip():
    from gaussianrpg_amd.perception import LetterboxPlan
    for p in (LetterboxPlan(1280, 1920, 640), LetterboxPlan.for_simulator(1066, 1600),
              LetterboxPlan(48, 64, 640, auto=False, scaleup=False),
              LetterboxPlan(1280, 1920, (384, 640), auto=False, scale_fill=True)):
        h, w = p.out_shape
        top, _, left, _ = p.pad
        boxes = torch.tensor([[left + 10.25, top + 7.5, left + 100.0, top + 50.75, 0.9, 2.0],     # inside the image
                              [0.0, 0.0, float(w), float(h), 0.5, 0.0],                        # the whole input
                              [left - 3.0, top - 2.0, left + 5.0, top + 4.0, 0.4, 1.0],        # reaches into the border
                              [0.0, 0.0, left * 0.5, top * 0.5, 0.3, 1.0],                     # inside the border
                              [w - 1.5, h - 0.5, w + 4.0, h + 9.0, 0.2, 3.0]], dtype=torch.float32)
        keep = boxes.clone()
        got = p.to_frame(boxes)
        assert torch.equal(boxes, keep) and got.dtype == torch.float32
        ref = boxes.double().numpy().copy()
        ref[:, [0, 2]] -= p.dwdh[0]
        ref[:, [1, 3]] -= p.dwdh[1]
        ref[:, :4] /= p.ratio[0]
        ref[:, [0, 2]] = ref[:, [0, 2]].clip(0, p.width)
        ref[:, [1, 3]] = ref[:, [1, 3]].clip(0, p.height)
        # float32, every value below 2^11 (ulp 2^-12): the subtraction's half ulp grows by 1 / ratio <= 3, the ratio's
        # own float32 rounding moves the quotient by 2^-25 of it, the division adds half an ulp -- under 2 ulp in all
        assert np.abs(got.double().numpy() - ref).max() <= 4 * 2048 * 2.0 ** -24
        assert torch.equal(got[:, 4:], boxes[:, 4:])
        assert torch.equal(p.to_frame(boxes.double()), torch.from_numpy(ref))


def test_detector_input_argument_errors():
    from gaussianrpg_amd.perception import LetterboxPlan, detector_input
    p = LetterboxPlan(40, 64, 64)
    frame = torch.zeros(40, 64, 3, dtype=torch.uint8)
    planes = torch.zeros(3, 40, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        detector_input(frame, p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        detector_input(planes, p, truncate=False)
    with pytest.raises(RuntimeError, match="no CPU path"):      # a plan that resizes: still the device comes first
        detector_input(torch.zeros(37, 53, 3, dtype=torch.uint8), LetterboxPlan(37, 53, 64))
    with pytest.raises(TypeError, match="frame must be a uint8 .* or float32"):
        detector_input(frame.to(torch.int32), p)
    with pytest.raises(TypeError, match="dtype must be torch.float32 or torch.float16"):
        detector_input(frame, p, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"frame must be uint8 \[40, 64, 3\]"):
        detector_input(torch.zeros(64, 40, 3, dtype=torch.uint8), p)
    with pytest.raises(ValueError, match=r"frame must be float32 \[3, 40, 64\]"):
        detector_input(torch.zeros(40, 64, 3), p)
    with pytest.raises(RuntimeError, match="out must be float32"):
        detector_input(frame, p, out=torch.zeros(3, 64, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="out must be float16"):
        detector_input(frame, p, dtype=torch.float16, out=torch.zeros(3, 64, 64))
    with pytest.raises(RuntimeError, match=r"out must be \[3,64,64\] or \[1,3,64,64\]"):
        detector_input(frame, p, out=torch.zeros(3, 40, 64))
    with pytest.raises(RuntimeError, match="out must be contiguous"):
        detector_input(frame, p, out=torch.zeros(3, 64, 128)[:, :, ::2])
    with pytest.raises(RuntimeError, match="frame must be contiguous"):
        detector_input(torch.zeros(40, 64, 6, dtype=torch.uint8)[:, :, ::2], p)
    # the bindings name their argument too
    from gaussianrpg_amd.rasterizer import _C
    with pytest.raises(RuntimeError, match="letterbox_rgb8: frame must be uint8"):
        _C.letterbox_rgb8(planes, p.geometry)
    with pytest.raises(RuntimeError, match=r"letterbox_planes: frame must be \[3,H,W\]"):
        _C.letterbox_planes(torch.zeros(40, 64, 3), p.geometry)
    with pytest.raises(RuntimeError, match="geometry must hold 8 ints"):
        _C.letterbox_rgb8(frame, [1, 2, 3])


def test_device_entry_points_fail_loudly_without_a_device(lib):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    g = (ctypes.c_int * 8)(40, 64, 12, 12, 0, 0, 64, 64)
    assert lib.grpg_letterbox_rgb8(None, 40, 64, g, None, None, 1, None, 0, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_letterbox_planes(None, 40, 64, g, None, None, 1, 1, None, 0, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
