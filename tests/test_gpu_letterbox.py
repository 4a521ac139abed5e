"""GPU tests of the fused frame -> detector-input op (gaussianrpg_amd/perception.py, csrc/letterbox.hip): the whole
output, borders included, bit for bit against the numpy restatement of the reference's four lines
(tests/letterbox_truth.py), for both sources, both channel orders and both output types."""
import ctypes
import os

import numpy as np
import pytest
import torch

import letterbox_truth as lt
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id -> (H, W, plan arguments); None: LetterboxPlan.for_simulator
PLANS = {
    "pad-40x64": (40, 64, dict(new_shape=64)),                                       # 12 / 12 rows
    "pad-four-sides": (48, 64, dict(new_shape=640, auto=False, scaleup=False)),      # 296/296/288/288
    "pad-simulator": (1066, 1600, None),                                             # -> 1088 x 1600
    "pad-none": (64, 64, dict(new_shape=64)),
    "down-96x160": (96, 160, dict(new_shape=64)),
    "up-37x53": (37, 53, dict(new_shape=64)),
    "up-5x7": (5, 7, dict(new_shape=20)),
    "odd-width-50": (37, 53, dict(new_shape=50, auto=False)),                        # w no multiple of the vector
    "scale-fill": (37, 53, dict(new_shape=(40, 72), auto=False, scale_fill=True)),   # x and y ratios differ
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _plan(name, device=None):
    from gaussianrpg_amd.perception import LetterboxPlan
    H, W, kw = PLANS[name]
    return LetterboxPlan.for_simulator(H, W, device=device) if kw is None else LetterboxPlan(H, W, device=device, **kw)


def _same(what, got, ref):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bits = np.uint16 if ref.dtype == np.float16 else np.uint32
    bad = got.view(bits) != ref.view(bits)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size,
                                                                        np.argwhere(bad)[0].tolist())


def test_plans_are_the_cases_they_claim():
    assert _plan("pad-40x64").pad == (12, 12, 0, 0) and not _plan("pad-40x64").needs_resize
    assert _plan("pad-four-sides").pad == (296, 296, 288, 288) and _plan("pad-four-sides").out_shape == (640, 640)
    assert _plan("pad-simulator").out_shape == (1088, 1600) and not _plan("pad-simulator").needs_resize
    assert _plan("pad-none").pad == (0, 0, 0, 0) and not _plan("pad-none").needs_resize
    assert _plan("down-96x160").resized == (38, 64) and _plan("up-37x53").resized == (45, 64)
    assert _plan("up-5x7").resized == (14, 20) and _plan("odd-width-50").out_shape == (50, 50)
    assert _plan("scale-fill").resized == (40, 72) and _plan("scale-fill").ratio[0] != _plan("scale-fill").ratio[1]


@pytest.mark.parametrize("name", list(PLANS))
def test_rgb8_equals_the_restatement(dev, name):
    from gaussianrpg_amd.perception import detector_input
    p = _plan(name, device=dev)
    H, W, _ = PLANS[name]
    imgs = lt.images(H, W, seed=len(name))
    if H * W > 100000:      # the large case: its rows run through all 256 values; the checker adds nothing to a copy
        del imgs["checker"]
    for img_name, im in imgs.items():
        frame = torch.from_numpy(im).to(dev)
        for rev in (True, False):
            ref = lt.detector_input(im, p.resized, p.pad, reverse_channels=rev)
            got = detector_input(frame, p, reverse_channels=rev)
            assert tuple(got.shape) == (1, 3) + p.out_shape and got.dtype == torch.float32 and got.is_contiguous()
            _same("%s %s rev=%d float32" % (name, img_name, rev), got, ref)
            got16 = detector_input(frame, p, reverse_channels=rev, dtype=torch.float16)
            assert got16.dtype == torch.float16
            _same("%s %s rev=%d float16" % (name, img_name, rev), got16, ref.astype(np.float16))


def test_all_256_values_are_the_correctly_rounded_quotient(dev):
    from gaussianrpg_amd.perception import LetterboxPlan, detector_input
    p = LetterboxPlan(3, 256, 256, auto=False, scaleup=False)      # 256 x 256, borders above and below
    im = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=0).repeat(3, axis=2)
    got = detector_input(torch.from_numpy(im).to(dev), p)
    top = p.pad[0]
    q32 = np.arange(256, dtype=np.float32) / np.float32(255.0)
    for c in range(3):
        assert np.array_equal(got[0, c, top].cpu().numpy().view(np.uint32), q32.view(np.uint32))
    got16 = detector_input(torch.from_numpy(im).to(dev), p, dtype=torch.float16)
    assert np.array_equal(got16[0, 1, top + 2].cpu().numpy().view(np.uint16), q32.astype(np.float16).view(np.uint16))
    assert float(got[0, 0, 0, 0]) == float(np.float32(114) / np.float32(255.0))


@pytest.mark.parametrize("name", ["pad-40x64", "up-37x53", "odd-width-50"])
@pytest.mark.parametrize("truncate", [True, False])
def test_planes_equal_pack_hwc_then_rgb8(dev, name, truncate):
    from gaussianrpg_amd import trajectory as tj
    from gaussianrpg_amd.perception import detector_input
    p = _plan(name, device=dev)
    H, W, _ = PLANS[name]
    rng = np.random.RandomState(11)
    v = rng.uniform(-0.2, 1.2, size=(3, H, W)).astype(np.float32)
    k = (np.arange(H * W * 3) % 256).reshape(3, H, W).astype(np.float32) / np.float32(255.0)   # exactly k / 255
    v[:, ::3] = k[:, ::3]
    v[:, 1::6] = np.nextafter(k[:, 1::6], np.float32(2))                                     # just above
    v[:, 4::6] = np.nextafter(k[:, 4::6], np.float32(-1))                                    # just below
    v[0, 0, :4] = [-1.0, 0.0, 1.0, 7.5]
    planes = torch.from_numpy(v).to(dev)
    packed = tj.pack_hwc(planes, truncate=truncate)
    assert np.array_equal(packed.cpu().numpy(), lt.quantise(v, truncate))
    for half in (False, True):
        dt = torch.float16 if half else torch.float32
        via_bytes = detector_input(packed, p, dtype=dt)
        direct = detector_input(planes, p, truncate=truncate, dtype=dt)
        assert torch.equal(direct, via_bytes)
        _same("planes %s" % name, direct, lt.detector_input(lt.quantise(v, truncate), p.resized, p.pad, half=half))
    assert torch.equal(detector_input(planes, p, truncate=truncate, reverse_channels=False),
                       detector_input(packed, p, reverse_channels=False))


@pytest.mark.parametrize("name", ["pad-40x64", "odd-width-50"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_out_as_one_slice_of_a_batch(dev, name, dtype):
    """Only that slice changes.  At 50 x 50 every other row starts off the store vector's alignment."""
    from gaussianrpg_amd.perception import detector_input
    p = _plan(name, device=dev)
    H, W, _ = PLANS[name]
    im = lt.images(H, W, seed=2)["random"]
    ref = lt.detector_input(im, p.resized, p.pad, half=dtype == torch.float16)
    frame = torch.from_numpy(im).to(dev)
    for slot in (1, 2):
        batch = torch.full((4, 3) + p.out_shape, float("nan"), dtype=dtype, device=dev)
        ret = detector_input(frame, p, dtype=dtype, out=batch[slot])
        assert ret.data_ptr() == batch[slot].data_ptr() and tuple(ret.shape) == (3,) + p.out_shape
        _same("slot %d" % slot, batch[slot:slot + 1], ref)
        others = [i for i in range(4) if i != slot]
        assert bool(torch.isnan(batch[others]).all())
    out4 = torch.empty((1, 3) + p.out_shape, dtype=dtype, device=dev)
    assert detector_input(frame, p, dtype=dtype, out=out4) is out4
    _same("[1,3,h,w] out", out4, ref)


def test_runs_on_the_current_stream(dev):
    from gaussianrpg_amd.perception import detector_input
    p = _plan("down-96x160", device=dev)
    im = lt.images(96, 160, seed=4)["random"]
    frame = torch.from_numpy(im).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        got = detector_input(frame, p)
    s.synchronize()
    _same("side stream", got, lt.detector_input(im, p.resized, p.pad))


def test_c_abi_directly_gives_the_same_bytes(dev):
    """ctypes and grpg_letterbox_rgb8, no _C: geometry and tables from the two host entries, uploaded by torch."""
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_letterbox_rgb8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    H, W = 37, 53
    g = (ctypes.c_int * 8)()
    assert lib.grpg_letterbox_geometry(H, W, 64, 64, 1, 0, 1, 32, g) == 0
    xt, yt = np.zeros((g[1], 2), np.int32), np.zeros((g[0], 2), np.int32)
    assert lib.grpg_letterbox_tables(H, W, g[0], g[1], xt.ctypes.data_as(ctypes.c_void_p),
                                     yt.ctypes.data_as(ctypes.c_void_p)) == 0
    im = lt.images(H, W, seed=9)["random"]
    frame, dxt, dyt = torch.from_numpy(im).to(dev), torch.from_numpy(xt).to(dev), torch.from_numpy(yt).to(dev)
    out = torch.empty(3, g[6], g[7], device=dev)
    torch.cuda.synchronize()
    rc = lib.grpg_letterbox_rgb8(frame.data_ptr(), H, W, ctypes.addressof(g), dxt.data_ptr(), dyt.data_ptr(), 1,
                                 out.data_ptr(), 0, None)
    assert rc == 0, lib.grpg_last_error()
    torch.cuda.synchronize()
    _same("C ABI", out[None], lt.detector_input(im, (g[0], g[1]), (g[2], g[3], g[4], g[5])))
    # the argument errors of the device entries
    bad = (ctypes.c_int * 8)(*list(g))
    bad[6] += 1
    assert lib.grpg_letterbox_rgb8(frame.data_ptr(), H, W, ctypes.addressof(bad), dxt.data_ptr(), dyt.data_ptr(), 1,
                                   out.data_ptr(), 0, None) == -1
    assert b"does not add up" in lib.grpg_last_error()
    assert lib.grpg_letterbox_rgb8(frame.data_ptr(), H, W, ctypes.addressof(g), None, None, 1, out.data_ptr(), 0,
                                   None) == -1
    assert b"x_table and y_table needed" in lib.grpg_last_error()
    assert lib.grpg_letterbox_rgb8(frame.data_ptr(), H, W, ctypes.addressof(g), dxt.data_ptr(), dyt.data_ptr(), 1,
                                   out.data_ptr() + 2, 0, None) == -1
    assert b"aligned" in lib.grpg_last_error()
    assert lib.grpg_letterbox_rgb8(None, H, W, ctypes.addressof(g), dxt.data_ptr(), dyt.data_ptr(), 1, out.data_ptr(),
                                   0, None) == -1
    assert lib.grpg_letterbox_rgb8(frame.data_ptr(), 0, W, ctypes.addressof(g), dxt.data_ptr(), dyt.data_ptr(), 1,
                                   out.data_ptr(), 0, None) == -1


@pytest.mark.parametrize("which", ["toy-48x64", "smoke-375x1242"])
def test_simulator_perception_frame_fused_equals_the_host_route(dev, which):
    from gaussianrpg_amd.perception import LetterboxPlan
    if which == "toy-48x64":
        sc, cam = hz.toy_scene(3000, seed=8, sh_degree=1).to(dev), hz.trajectory_camera(2, W=64, H=48, device=dev)
        H, W = 48, 64
    else:
        sc, cam = hz.smoke_scene(4000, seed=1).to(dev), hz.smoke_camera(1242, 375, device=dev)
        H, W = 375, 1242
    p = LetterboxPlan(H, W, 640, device=dev)
    fused = hz.simulator_perception_frame(sc, cam, p, fused=True)
    host = hz.simulator_perception_frame(sc, cam, p, fused=False)
    torch.cuda.synchronize()
    assert tuple(fused.shape) == (1, 3) + p.out_shape and fused.dtype == torch.float32
    assert torch.equal(fused, host)
    inside = fused[0, :, p.pad[0]:p.pad[0] + p.resized[0]]
    assert float(inside.max()) > float(inside.min())       # a picture, not a constant
