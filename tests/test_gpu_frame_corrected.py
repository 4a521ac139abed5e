"""-m gpu: the colour correction inside the one-call frame's epilogue (``forward_frame(..., affine=A)``; C ABI
``grpg_bind_frame_correction``; csrc/render_fwd.hip ``frame_finish``) against the chain it replaces for a scene trained
with ``use_color_correction`` (lib/models/street_gaussian_renderer.py:103-116):

    o     = forward_frame(planes=True, rgb8=False, sky_cube=None, clamp=True)     the op's evaluation planes
    x     = o.rgb + clamp(sky) * (1 - o.alpha)                                    unclamped
    y     = clamp(A[:, :3] x + A[:, 3])
    frame = uint8(y * 255), [H,W,3]

here: ``appearance.corrected_frame`` / ``sky_corrected`` / ``color_correct`` (csrc/color_correction.hip, one launch behind
the render).  The epilogue runs the same statements from the same bodies (csrc/sky_math.h, csrc/color_math.h) on the
pixel's final state: every byte and every plane must be IDENTICAL, on every store path of the epilogue (dword stores,
byte stores, system-scope stores into pinned host memory, the drained staging frame).  The cube map holds values
outside [0,1] and one matrix has gains above 1, so that every clamp binds; test_order_is_visible shows that a clamp in
the wrong place would be seen.  The float64 truth of tests/color_correction_truth.py bounds the bytes from outside.
"""
import numpy as np
import pytest
import torch

import color_correction_truth as T
import helpers
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

# (W, H, destination): the smallest shapes at which each store path and tile edge of the epilogue occurs
SHAPES = [(200, 136, "device"),     # dword path (W % 4 == 0), no drain
          (203, 121, "device"),     # byte path, partial tiles both ways
          (256, 100, "host"),       # W % 64 == 0: drained whole lines, partial last tile row
          (400, 300, "host"),       # W % 16 == 0: drained, narrower last unit
          (203, 121, "host")]       # direct system-scope stores
WIDE, NEAR = ("wide", 1), ("near", 9)      # build_affine(kind, seed): gains up to 2 / within 0.1 of the identity


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _K_w2c(cam):
    W, H = int(cam.image_width), int(cam.image_height)
    K = torch.tensor([[W / (2.0 * cam.tanfovx), 0.0, W / 2.0], [0.0, H / (2.0 * cam.tanfovy), H / 2.0],
                      [0.0, 0.0, 1.0]], dtype=torch.float32)
    return K, cam.viewmatrix.detach().cpu().t().contiguous()


def _cube(res=32, seed=3):
    """values outside [0,1] too: the lookup clamps the sample, the composite is NOT clamped in front of the map"""
    return torch.rand(6, res, res, 3, generator=torch.Generator().manual_seed(seed)) * 1.3 - 0.15


def _sky(dev, res=32, seed=3, white=False, cube=None):
    from gaussianrpg_amd.sky import SkyCubeMap
    sky = SkyCubeMap(resolution=res, white_background=white).to(dev)
    with torch.no_grad():
        sky.sky_cube_map.copy_((_cube(res, seed) if cube is None else cube).to(dev))
    return sky


def _rast(cam, sh_degree, dev, bg=(0.05, 0.1, 0.0)):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(
        cam, sh_degree, bg=torch.tensor(bg, dtype=torch.float32, device=dev))))


def _affine(spec, dev):
    return torch.from_numpy(T.build_affine(spec[0], seed=spec[1])).to(dev)


def _same(name, a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: %d of %d values differ" % (
        name, int((a != b).sum()), a.size)


def _dest(kind, H, W, dev):
    d = torch.full((H, W, 3), 7, dtype=torch.uint8)
    return d.pin_memory() if kind == "host" else d.to(dev)


_SETUPS = {}


def _setup(dev, W, H, dense=False):
    """scene, layer mask, camera, rasterizer and the UNCORRECTED evaluation planes of a shape; computed once, read-only.
    The scene is a thin cloud: a third of the pixels is mostly sky, most of the rest partly; dense: the 6000 + 900
    Gaussians of tests/test_gpu_frame.py, which cover the frame (a tenth to a fifth of the pixels still fetch the sky)."""
    if (W, H, dense) not in _SETUPS:
        from test_gpu_layers import _objects_scene
        sc, obj = _objects_scene(6000, 900, seed=3) if dense else _objects_scene(600, 300, seed=3)
        d, m = sc.to(dev), obj.to(dev)
        cam = hz.trajectory_camera(1, W=W, H=H, device=dev)
        K, w2c = _K_w2c(cam)
        rast = _rast(cam, 1, dev)
        kw = dict(shs=d.shs, scales=d.scales, rotations=d.rotations)
        with torch.no_grad():
            o = rast.forward_frame(d.means3D, d.opacity, planes=True, rgb8=False, sky_cube=None, clamp=True, **kw)
        _SETUPS[(W, H, dense)] = dict(d=d, m=m, cam=cam, K=K.to(dev), w2c=w2c.to(dev), rast=rast, kw=kw, o=o)
    return _SETUPS[(W, H, dense)]


def _chain(o, A, sky, K, w2c, truncate=True):
    """(clamped planes, bytes) of the stand-alone launch on the uncorrected planes"""
    from gaussianrpg_amd import appearance
    if sky is None:
        planes = appearance.color_correct(o["rgb"], A, clamp=True)
    else:
        planes = appearance.sky_corrected(sky, o["rgb"], o["alpha"], A, K=K, w2c=w2c, train=False)
    return planes, appearance.corrected_frame(o["rgb"], o["alpha"], A, sky=sky, K=K, w2c=w2c, truncate=truncate)


def _sky_args(sky, K, w2c):
    from gaussianrpg_amd.sky import ray_matrix
    if sky is None:
        return {}
    return dict(sky_cube=sky.sky_cube_map, ray_matrix=ray_matrix(K, w2c), sky_fill=sky.fill)


# ---------------------------------------------------------------------------------------------------------------
# 1. one call == the chain, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,where", SHAPES, ids=["%dx%d-%s" % s for s in SHAPES])
def test_one_call_equals_the_chain(dev, W, H, where):
    from gaussianrpg_amd import appearance
    s = _setup(dev, W, H)
    d, o, rast, K, w2c = s["d"], s["o"], s["rast"], s["K"], s["w2c"]
    skies = {None: None, 0: _sky(dev), 1: _sky(dev, white=True)}
    assert skies[0].fill == 0.0 and skies[1].fill == 1.0
    # the final clamp binds for the wide matrix, on both sides
    with torch.no_grad():
        y = appearance.sky_corrected(skies[0], o["rgb"], o["alpha"], _affine(WIDE, dev), K=K, w2c=w2c, train=True)
    assert float(y.max()) > 1.05 and float(y.min()) < -0.05
    assert float((o["alpha"] < 0.5).float().mean()) > 0.05, "the composite reaches too little of the frame"
    n = 0
    for fill in (None, 0, 1):
        for truncate in (True, False):
            spec = (WIDE, NEAR, NEAR, WIDE, WIDE, NEAR)[n]         # both matrices meet both conversions
            n += 1
            A, sky = _affine(spec, dev), skies[fill]
            what = "sky_fill=%s truncate=%s %s" % (fill, truncate, spec[0])
            with torch.no_grad():
                planes_ref, bytes_ref = _chain(o, A, sky, K, w2c, truncate)
                dst, dst2 = _dest(where, H, W, dev), _dest(where, H, W, dev)
                res = rast.forward_frame(d.means3D, d.opacity, planes=True, truncate=truncate, affine=A, out=dst,
                                         **s["kw"], **_sky_args(sky, K, w2c))
                only = rast.forward_frame(d.means3D, d.opacity, planes=False, truncate=truncate, affine=A, out=dst2,
                                          **s["kw"], **_sky_args(sky, K, w2c))
            torch.cuda.synchronize()
            assert res["rgb8"].data_ptr() == dst.data_ptr() and "rgb" not in only
            _same("rgb8 " + what, dst, bytes_ref)
            _same("rgb8 (bytes only) " + what, dst2, bytes_ref)
            _same("rgb " + what, res["rgb"], planes_ref)
            _same("depth " + what, res["depth"], o["depth"])
            _same("alpha " + what, res["alpha"], o["alpha"])
            assert len(np.unique(bytes_ref.cpu().numpy())) > 50, "the frame is not a picture"


# ---------------------------------------------------------------------------------------------------------------
# 2. the identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
def test_identity_is_the_uncorrected_frame(dev, where):
    W, H = 200, 136
    s = _setup(dev, W, H)
    d, rast = s["d"], s["rast"]
    e = _sky_args(_sky(dev), s["K"], s["w2c"])
    eye = torch.eye(4, device=dev)[:3].contiguous()
    with torch.no_grad():
        want = rast.forward_frame(d.means3D, d.opacity, planes=True, clamp=True, **s["kw"], **e)
        got = rast.forward_frame(d.means3D, d.opacity, planes=True, clamp=True, affine=eye, out=_dest(where, H, W, dev),
                                 **s["kw"], **e)
    torch.cuda.synchronize()
    _same("rgb8", got["rgb8"], want["rgb8"])
    for k in ("rgb", "depth", "alpha"):       # by value: 1 * (-0) + 0 is +0
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------
# 3. the order of composite, map and clamp is visible on this input
# ---------------------------------------------------------------------------------------------------------------
# Share of the bytes at which the wrong order (composite CLAMPED in front of the map) differs from the one-call frame.
# It takes a pixel whose colour plus sky exceeds 1 in a channel the map does not saturate anyway.  First run on an
# MI355X (200x136, the thin scene, wide matrix): 0.0064 of the bytes, 522 of 81 600; the floor is half of that.
ORDER_SHARE_MEASURED = 0.0064
ORDER_SHARE_FLOOR = 0.003


def test_order_is_visible(dev):
    from gaussianrpg_amd import appearance
    W, H = 200, 136
    s = _setup(dev, W, H)
    d, rast = s["d"], s["rast"]
    sky = _sky(dev)
    e = _sky_args(sky, s["K"], s["w2c"])
    A = _affine(WIDE, dev)
    with torch.no_grad():
        got = rast.forward_frame(d.means3D, d.opacity, affine=A, **s["kw"], **e)["rgb8"]
        clamped = rast.forward_frame(d.means3D, d.opacity, planes=True, rgb8=False, clamp=True, **s["kw"], **e)
        wrong = appearance.corrected_frame(clamped["rgb"], clamped["alpha"], A)
    share = float((got != wrong).float().mean())
    print("order_is_visible: the wrong order differs at %.4f of the bytes" % share)
    helpers.PARITY_STATS.append(dict(test="test_order_is_visible", plane="rgb8", differing_share=share))
    assert share > ORDER_SHARE_FLOOR


# ---------------------------------------------------------------------------------------------------------------
# 4. layered frame: the composition is corrected, the layers are not
# ---------------------------------------------------------------------------------------------------------------
def test_layered_frame_corrects_the_composition_only(dev):
    W, H = 200, 136
    s = _setup(dev, W, H)
    d, m, rast, K, w2c = s["d"], s["m"], s["rast"], s["K"], s["w2c"]
    sky = _sky(dev, res=16, seed=5)
    A = _affine(WIDE, dev)
    with torch.no_grad():
        plain = rast.forward_frame(d.means3D, d.opacity, layer_class=m, planes=True, rgb8=False, sky_cube=None,
                                   clamp=True, **s["kw"])
        planes_ref, bytes_ref = _chain(plain, A, sky, K, w2c)
        got = rast.forward_frame(d.means3D, d.opacity, layer_class=m, planes=True, affine=A, **s["kw"],
                                 **_sky_args(sky, K, w2c))
        host = _dest("host", H, W, dev)
        rast.forward_frame(d.means3D, d.opacity, layer_class=m, affine=A, out=host, **s["kw"], **_sky_args(sky, K, w2c))
    torch.cuda.synchronize()
    _same("rgb8", got["rgb8"], bytes_ref)
    _same("rgb8 (pinned host)", host, bytes_ref)
    _same("rgb", got["rgb"], planes_ref)
    for k in ("depth", "alpha", "color_background", "alpha_background", "color_object", "alpha_object"):
        _same(k, got[k], plain[k])
    assert float((plain["color_object"] - plain["color_background"]).abs().max()) > 0.1     # two different layers


# ---------------------------------------------------------------------------------------------------------------
# 5. composed frame; both bindings on one call
# ---------------------------------------------------------------------------------------------------------------
def test_composed_frame_equals_the_flat_one_call_frame(dev):
    import frame_truth
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussianrpg_amd.composed import ComposedRasterizer, compose
    from gaussianrpg_amd.sky import ray_matrix
    from gaussianrpg_amd.tracks import PoseBatch
    from test_compose import _to
    c = frame_truth.composed_case(320, 200)
    models, poses = c["models"], c["poses"]
    md = [_to(mm, dev) for mm in models]
    cam = hz.trajectory_camera(4, W=320, H=200, device=dev)
    K, w2c = _K_w2c(cam)
    settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1))
    cr, flat = ComposedRasterizer(settings), GaussianRasterizer(settings)
    sky = _sky(dev, res=24, cube=torch.from_numpy(np.asarray(c["cube"])))
    e = dict(sky_cube=sky.sky_cube_map, ray_matrix=ray_matrix(K.to(dev), w2c.to(dev)))
    A = _affine(WIDE, dev)
    actors = [p for p in poses if p is not None]
    static = len(poses) - len(actors)
    assert static >= 1 and all(p is None for p in poses[:static]) and len(actors) >= 2
    batch = PoseBatch(torch.tensor([[list(map(float, p.obj_rot)) for p in actors]], device=dev),
                      torch.tensor([[list(map(float, p.obj_trans)) for p in actors]], device=dev),
                      torch.ones(1, len(actors), dtype=torch.uint8, device=dev))
    table = batch.rows(0, list(range(len(actors))), [p.fourier_time for p in actors], static=static)
    with torch.no_grad():
        means3D, scales, rotations, opacity, shs = compose(md, poses)
        want = flat.forward_frame(means3D, opacity, shs=shs, scales=scales, rotations=rotations, planes=True, affine=A, **e)
        plain = flat.forward_frame(means3D, opacity, shs=shs, scales=scales, rotations=rotations, planes=True, **e)
        got = cr.forward_frame(md, poses, planes=True, affine=A, **e)
        rows = cr.forward_frame(md, table, planes=True, affine=A, **e)
        after = cr.forward_frame(md, table, planes=True, **e)          # neither binding outlives its call
    torch.cuda.synchronize()
    for name, r in (("host poses", got), ("device poses", rows)):
        for k in ("rgb8", "rgb", "depth", "alpha"):
            _same("%s: %s" % (name, k), r[k], want[k])
    _same("uncorrected behind a corrected call", after["rgb8"], plain["rgb8"])
    assert float((want["rgb8"] != plain["rgb8"]).float().mean()) > 0.3


# ---------------------------------------------------------------------------------------------------------------
# 6. a frame without Gaussians
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(70, 50), (256, 100)])
def test_frame_without_gaussians_is_corrected(dev, W, H):
    cam = hz.trajectory_camera(0, W=W, H=H, device=dev)
    K, w2c = _K_w2c(cam)
    K, w2c = K.to(dev), w2c.to(dev)
    sky = _sky(dev, res=8, seed=1)
    rast = _rast(cam, 0, dev, bg=(0.5, 0.25, 0.125))
    A = _affine(WIDE, dev)
    z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
    empty = dict(shs=z(0, 1, 3), scales=z(0, 3), rotations=z(0, 4))
    host = _dest("host", H, W, dev)
    with torch.no_grad():
        # P == 0: the op's colour is ZERO (not the background), alpha zero -> the corrected sky everywhere
        planes_ref, bytes_ref = _chain(dict(rgb=z(3, H, W), alpha=z(1, H, W)), A, sky, K, w2c)
        res = rast.forward_frame(z(0, 3), z(0, 1), planes=True, affine=A, **empty, **_sky_args(sky, K, w2c))
        rast.forward_frame(z(0, 3), z(0, 1), affine=A, out=host, **empty, **_sky_args(sky, K, w2c))
    torch.cuda.synchronize()
    _same("rgb8", res["rgb8"], bytes_ref)
    _same("rgb8 (pinned host)", host, bytes_ref)
    _same("rgb", res["rgb"], planes_ref)
    assert len(np.unique(bytes_ref.cpu().numpy())) > 20


# ---------------------------------------------------------------------------------------------------------------
# 7. against the float64 truth
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,where", [(203, 121, "device"), (256, 100, "host")])
def test_bytes_against_the_float64_truth(dev, W, H, where):
    from gaussianrpg_amd.sky import ray_matrix
    # The share of bytes the truth cannot determine grows with the composite's own tolerance: the sample's (16 res u
    # per weight, tests/sky_truth.py) times (1 - acc), carried through |A| and times 255 against a byte's unit width;
    # the map alone (4u) leaves 6e-4.  The thin scene with a 32^2 cube puts 3 % of the pixels there (first run:
    # 0.0356 / 0.0300), so this test takes the covering scene and an 8^2 cube: 6.5e-4 / 8.6e-4 on the CPU oracle's
    # planes of the same scene, from the truth alone (on an MI355X: 6.5e-4 / 8.2e-4; the bytes differ from the
    # truth's at 2 and 1 places, all fragile).
    s = _setup(dev, W, H, dense=True)
    d, o, rast = s["d"], s["o"], s["rast"]
    cube = _cube(8, 3)
    sky = _sky(dev, res=8, cube=cube)
    M = ray_matrix(s["K"].cpu(), s["w2c"].cpu())             # the float32 matrix the kernel is handed
    spec = NEAR
    A = T.build_affine(spec[0], seed=spec[1])
    dst = _dest(where, H, W, dev)
    with torch.no_grad():
        rast.forward_frame(d.means3D, d.opacity, affine=torch.from_numpy(A).to(dev), out=dst, sky_cube=sky.sky_cube_map,
                           ray_matrix=M.to(dev), **s["kw"])
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    i = dict(cube=cube.numpy(), M=M.numpy(), acc=o["alpha"].cpu().numpy(), mask=None, jitter=None, fill=0.0,
             rgb=o["rgb"].cpu().numpy())
    x64, tol_x = T.composite64(i, H, W)
    y64, tol = T.forward64(A, x64, tol_x)
    fragile = T.fragile_bytes(y64, tol).transpose(1, 2, 0)
    share = float(fragile.any(axis=2).mean())
    want = T.bytes64(y64)
    print("frame_corrected/%dx%d-%s: fragile share %.3g, one call != truth at %d bytes" % (
        W, H, where, share, int((got != want).sum())))
    helpers.PARITY_STATS.append(dict(test="test_bytes_against_the_float64_truth", plane="%dx%d-%s" % (W, H, where),
                                     fragile_share=share, differing_bytes=int((got != want).sum()),
                                     matrix="%s seed %d" % spec, cube="8^2 seed 3"))
    assert float((o["alpha"] < 0.999).float().mean()) > 0.05, "the composite reaches too little of the frame"
    assert share < 1e-3
    assert not ((got != want) & ~fragile).any(), "the one-call frame differs from the truth at a byte it determines"
    assert len(np.unique(got)) > 50, "the frame is not a picture"


# ---------------------------------------------------------------------------------------------------------------
# 8. the binding does not outlive its call
# ---------------------------------------------------------------------------------------------------------------
def test_binding_hygiene_through_the_torch_module(dev):
    W, H = 200, 136
    s = _setup(dev, W, H)
    d, rast = s["d"], s["rast"]
    e = _sky_args(_sky(dev), s["K"], s["w2c"])
    params = torch.stack([_affine(NEAR, dev), _affine(WIDE, dev), _affine(NEAR, dev)])     # affine_trans [N,3,4]
    call = lambda **k: rast.forward_frame(d.means3D, d.opacity, **s["kw"], **e, **k)["rgb8"]   # noqa: E731
    with torch.no_grad():
        plain = call()
        first = call(affine=params[1])                       # a view of the parameter, used as it is
        again = call()
        second = call(affine=params[1])
        spread = torch.zeros(3, 8, device=dev)
        spread[:, ::2] = params[1]
        assert not spread[:, ::2].is_contiguous()
        strided = call(affine=spread[:, ::2])                # not contiguous: made contiguous
    _same("uncorrected behind a corrected frame", again, plain)
    _same("two identical corrected calls", second, first)
    _same("a strided view", strided, first)
    assert float((first != plain).float().mean()) > 0.3
    for bad in (torch.zeros(3, 3, device=dev), torch.zeros(3, 4), torch.zeros(3, 4, device=dev, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=r"affine must be a float32 tensor \[3,4\] on the image's device"):
            call(affine=bad)
    _same("uncorrected behind refused calls", call(), plain)
    from gaussianrpg_amd.rasterizer import _C                      # noqa: F401  (the library is loaded)
    import ctypes
    import os
    lib = ctypes.CDLL(os.path.join(os.path.dirname(hz.__file__), "libgrpg_rasterizer.so"))
    assert lib.grpg_frame_correction_bound() == 0


# ---------------------------------------------------------------------------------------------------------------
# 9. harness.simulator_frame_corrected(one_call=True)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sky", [False, True])
def test_harness_one_call_equals_the_fused_route(dev, with_sky):
    W, H = 320, 200
    sc = hz.toy_scene(5000, seed=9, sh_degree=1).to(dev)
    cam = hz.trajectory_camera(3, W=W, H=H, device=dev)
    K, w2c = _K_w2c(cam)
    sky = _sky(dev, seed=4) if with_sky else None
    A = _affine(WIDE, dev)
    fused = hz.simulator_frame_corrected(sc, cam, A, sky, K, w2c, fused=True)
    out = torch.full((H, W, 3), 3, dtype=torch.uint8).pin_memory()
    one = hz.simulator_frame_corrected(sc, cam, A, sky, K, w2c, one_call=True, out=out)
    assert one.shape == (H, W, 3) and one.dtype == np.uint8
    np.testing.assert_array_equal(one, fused)
    np.testing.assert_array_equal(out.numpy(), fused)
    np.testing.assert_array_equal(hz.simulator_frame_corrected(sc, cam, A, sky, K, w2c, one_call=True), fused)
    assert len(np.unique(fused)) > 50, "the frame is not a picture"
