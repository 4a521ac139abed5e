"""The simulator's published frame from the CPU oracle alone -- plain numpy, no GPU: what the reference's callers make of
the op's planes per frame (lib/models/street_gaussian_renderer.py:106-116,236-237; simulator.py:313-314),

    rgb   = clip(op colour, 0, 1)
    rgb   = clip(rgb + clip(sky_cubemap(rays)) * (1 - acc), 0, 1)
    frame = floor(255 rgb [+ 0.5]) as uint8 [H, W, 3]

from oracle.forward's planes and oracle/sky_torch.py, and the bars a device frame is held to against it.  The bars come
from the project's existing ones (tests/helpers.py, tests/test_sky.py), not from the code under test.
"""
import os

import numpy as np
import torch

import helpers
from gaussianrpg_amd import harness as hz
from helpers import ATOL, FRAGILE_ATOL, RTOL
from oracle import sky_torch as st

SKY_BAR = 3e-5            # tests/test_sky.py's bar on the composite
# caps on what a comparison may hide or never look at, asserted on the oracle alone
MAX_NEAR, MAX_FRAGILE, MIN_SKY_VISIBLE, MAX_SATURATED = 0.25, 0.10, 0.2, 0.05


def K_w2c(cam):
    """Intrinsics and world-to-camera matrix of a harness camera (viewmatrix is the TRANSPOSED w2c; principal point
    at the image centre)."""
    W, H = int(cam.image_width), int(cam.image_height)
    K = torch.tensor([[W / (2.0 * cam.tanfovx), 0.0, W / 2.0], [0.0, H / (2.0 * cam.tanfovy), H / 2.0],
                      [0.0, 0.0, 1.0]], dtype=torch.float32)
    return K, cam.viewmatrix.detach().cpu().t().contiguous()


def sky_cube(res=32, seed=3):
    """The cube map tests/test_gpu_frame.py's _sky() loads: values beyond [0, 1] too, the lookup clamps."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(6, res, res, 3, generator=g) * 1.4 - 0.2


def turned_camera(W, H, yaw=0.22, pitch=-0.12, device="cpu"):
    """A camera whose rotation is NOT symmetric (the trajectory cameras have the identity): yaw about y, then pitch
    about x, at the origin.  With it a transposed rotation in the sky's rays shows."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    s = W / hz.WAYMO_W
    return hz.make_camera(R, np.zeros(3), W=W, H=H, fx=hz.WAYMO_FX * s, fy=hz.WAYMO_FY * s, cx=W / 2.0, cy=H / 2.0,
                          device=device)


def to_bytes(v, truncate):
    """float64 [3,H,W] in [0,1] -> uint8 [H,W,3]: floor(255 v) or floor(255 v + 0.5)."""
    x = 255.0 * np.asarray(v, np.float64) + (0.0 if truncate else 0.5)
    return np.floor(x).clip(0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def oracle_frame(o, cube, K, w2c, truncate, fill=0.0):
    """oracle.forward's result o, cube [6,res,res,3] -> (uint8 [H,W,3], the float64 composite v [3,H,W])."""
    color = np.clip(np.asarray(o["color"], np.float64), 0.0, 1.0)
    H, W = color.shape[1:]
    sky = st.sky_color(np.asarray(cube), K, w2c, H, W, acc=o["alpha"], fill=fill)
    v = st.composite(color, o["alpha"], sky, clamp=True)
    return to_bytes(v, truncate), v


def byte_tolerance(v):
    """The float error a device composite may have against v: 2 (ATOL + RTOL |v|) + 3e-5.  The 2: the error of the
    colour (ATOL + RTOL |c|, the image bar) plus the error of acc (the same bar) times a sky value in [0, 1]; 3e-5 is
    the sky composite's own bar.  Not covered: a pixel whose 1 - acc rounds to the other side of the sky mask's 1e-3
    threshold on the device takes the fill where the oracle takes the lookup, worth up to 1e-3; such a pixel would
    fail the bars below and would have to be looked at, not exempted."""
    return 2.0 * (ATOL + RTOL * np.abs(v)) + SKY_BAR


def near_boundary(v, truncate):
    """bool [H,W,3]: 255 v + bias lies within 255 tol of an integer -- an error within the float bar may move the byte."""
    x = (255.0 * v + (0.0 if truncate else 0.5)).transpose(1, 2, 0)
    return np.abs(x - np.rint(x)) <= 255.0 * byte_tolerance(v).transpose(1, 2, 0)


def conditions(o, v, truncate):
    """What the comparison could hide, from the oracle alone: shares of near bytes, fragile pixels, pixels where the
    sky contributes (acc < 0.999) and saturated values."""
    return dict(near=float(near_boundary(v, truncate).mean()), fragile=float((np.asarray(o["fragile"]) != 0).mean()),
                sky_visible=float((np.asarray(o["alpha"]) < 0.999).mean()), saturated=float(((v <= 0.0) | (v >= 1.0)).mean()))


def assert_conditions(name, c):
    assert c["near"] <= MAX_NEAR, "%s: %.3f of the bytes lie near a quantisation boundary" % (name, c["near"])
    assert c["fragile"] <= MAX_FRAGILE, "%s: fragile share %.3f" % (name, c["fragile"])
    assert c["sky_visible"] >= MIN_SKY_VISIBLE, "%s: the sky shows in only %.3f of the pixels" % (name, c["sky_visible"])
    assert c["saturated"] <= MAX_SATURATED, "%s: %.3f of the values are saturated" % (name, c["saturated"])


def compare_bytes(got, v, fragile, truncate, name="rgb8"):
    """got uint8 [H,W,3] against the oracle's composite v [3,H,W]: a byte of a non-fragile pixel that is not near a
    quantisation boundary must be EQUAL, a near one may differ by 1, a byte of a fragile pixel by
    ceil(255 FRAGILE_ATOL (1 + |v|)).  Returns (and records in helpers.PARITY_STATS) the shares of bytes that differ
    at all and by more than 1."""
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == (v.shape[1], v.shape[2], 3), (name, got.dtype, got.shape)
    ref = to_bytes(v, truncate)
    diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    near = near_boundary(v, truncate)
    frag = np.broadcast_to((np.asarray(fragile) != 0)[:, :, None], diff.shape)
    vh = np.abs(v).transpose(1, 2, 0)
    limit = np.where(frag, np.ceil(255.0 * FRAGILE_ATOL * (1.0 + vh)), np.where(near, 1, 0)).astype(np.int64)
    stats = dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], plane=name, pixels=int(diff.size),
                 frac_diff_gt0=float((diff > 0).mean()), frac_diff_gt1=float((diff > 1).mean()),
                 near_frac=float(near.mean()), fragile_frac=float(frag.mean()), max_diff=int(diff.max()))
    helpers.PARITY_STATS.append(stats)
    bad = diff > limit
    if bad.any():
        y, x, c = np.argwhere(bad)[0]
        raise AssertionError(
            "%s: %d of %d bytes beyond their bar (%d of them neither near a boundary nor fragile); first at y=%d x=%d "
            "c=%d: %d against %d, 255 v = %.4f; differ at all %.4f, by more than 1 %.5f" % (
                name, int(bad.sum()), bad.size, int((bad & ~near & ~frag).sum()), y, x, c, got[y, x, c], ref[y, x, c],
                255.0 * v[c, y, x], stats["frac_diff_gt0"], stats["frac_diff_gt1"]))
    return stats


# ---- the frames the host and the GPU tests share: computed once per process, never modified ----

BG = (0.05, 0.1, 0.0)
_CACHE = {}


def _finish(key, o, cube, K, w2c, truncate, fill, **more):
    ref8, v = oracle_frame(o, cube, K, w2c, truncate, fill)
    for a in (ref8, v):
        a.setflags(write=False)
    _CACHE[key] = dict(o=o, cube=cube, K=K, w2c=w2c, truncate=truncate, fill=fill, ref8=ref8, v=v,
                       fragile=np.asarray(o["fragile"]) != 0, **more)
    return _CACHE[key]


def plain_case(W, H, truncate, fill=0.0, turned=False):
    """toy_scene(5000, seed=8, sh_degree=1) from trajectory_camera(2) (or the turned camera), bg BG, sky res 32 seed 3:
    the scene, camera and sky of test_gpu_frame.test_frame_epilogue_equals_the_three_launch_chain."""
    import oracle
    key = ("plain", W, H, truncate, fill, turned)
    if key in _CACHE:
        return _CACHE[key]
    sc = hz.toy_scene(5000, seed=8, sh_degree=1)
    cam = turned_camera(W, H) if turned else hz.trajectory_camera(2, W=W, H=H)
    K, w2c = K_w2c(cam)
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                       **helpers.oracle_kwargs(cam, 1, bg=torch.tensor(BG)))
    return _finish(key, o, sky_cube(32, 3).numpy(), K, w2c, truncate, fill, scene=sc, cam=cam)


def composed_case(W=320, H=200, seed=5):
    """test_compose._scene_graph(sh_degree=1, nb=30_000, actors=((3000, 5), (2000, 3))) from trajectory_camera(4), black
    background, sky res 24 seed 9 (test_gpu_frame.test_composed_frame_is_the_simulators_frame): composition by
    oracle/compose_torch, then oracle.forward, then oracle_frame."""
    import oracle
    from oracle import compose_torch as ct
    from test_compose import _scene_graph
    key = ("composed", W, H, seed)
    if key in _CACHE:
        return _CACHE[key]
    models, poses = _scene_graph(sh_degree=1, nb=30_000, actors=((3000, 5), (2000, 3)), seed=seed)
    cam = hz.trajectory_camera(4, W=W, H=H)
    K, w2c = K_w2c(cam)
    means, scales, rots, opac, shs = ct.compose(
        models, [None if p is None else (p.obj_rot, p.obj_trans, p.fourier_time) for p in poses])
    o = oracle.forward(means, opac, shs=shs, scales=scales, rotations=rots, **helpers.oracle_kwargs(cam, 1))
    return _finish(key, o, sky_cube(24, 9).numpy(), K, w2c, True, 0.0, models=models, poses=poses, cam=cam)
