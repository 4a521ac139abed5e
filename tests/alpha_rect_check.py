"""Test infrastructure (CPU): the rectangle an evaluation frame bins (csrc/preprocess.hip binned_rect over
csrc/blend_math.h alpha_box) restated in numpy float32, the render's accept arithmetic (blend_math.h: pre-scaled
conic, exp2, min(0.99, .), the two rejects) likewise, and the scenes tests/test_gpu_alpha_rect.py renders -- shared
with tests/test_alpha_rect_host.py, which states what the restatement predicts for them.

The restatement follows the device step by step (preprocess.hip is compiled without contraction: every multiply and
add below is one of its roundings; the fused steps go through float64, which holds a product of two floats exactly).
Only the hardware's approximate log / reciprocal / square root / exp2 are numpy's correctly rounded ones here: one
ulp on a bound whose inflation is 1e-3 pixels.   usage: python tests/alpha_rect_check.py  (prints the scene table)
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianrpg_amd import harness as hz          # noqa: E402
from helpers import device_power2                   # noqa: E402

f32 = np.float32
TILE = 16


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def reference_rect(px, py, radius, gx, gy):
    """common.h get_rect: the reference's 3-sigma rectangle, half-open tile ranges (minx, miny, maxx, maxy)."""
    px, py = px.astype(f32), py.astype(f32)
    r = radius.astype(f32)
    with np.errstate(invalid="ignore"):
        t = lambda v, g: np.clip(np.nan_to_num(np.trunc(v / f32(16.0)), nan=0.0, posinf=1e9, neginf=-1e9), 0, g).astype(np.int64)  # noqa: E731
        return t(px - r, gx), t(py - r, gy), t(px + r + f32(15.0), gx), t(py + r + f32(15.0), gy)


def alpha_box_f32(px, py, a, b, c, op):
    """blend_math.h alpha_box -> (x0, x1, y0, y1, keep_all, transparent); tile ranges half-open, unclamped."""
    px, py, a, b, c, op = (np.asarray(v).astype(f32) for v in (px, py, a, b, c, op))
    with np.errstate(all="ignore"):
        t = f32(2.0) * np.log(f32(255.0) * op)
        t = t + f32(1e-4) * np.abs(t) + f32(2e-3)
        p = b * b
        det = _fma(a, c, -p) - _fma(b, b, -p)
        sane = (a > 0) & (c > 0) & (det > 0) & (np.abs(t) < f32(3e38)) & (np.abs(det) < f32(3e38))
        transparent = op < f32((1.0 / 255.0) * 0.999)
        s = t * (f32(1.0) / det)
        hx = np.sqrt(np.fmax(s * c, f32(0.0)))   # (fmaxf: a NaN operand gives the other one)
        hy = np.sqrt(np.fmax(s * a, f32(0.0)))
        hx = hx + (f32(1e-3) + f32(1e-5) * np.abs(hx))
        hy = hy + (f32(1e-3) + f32(1e-5) * np.abs(hy))
        fx0 = np.ceil((px - hx - f32(15.0)) * f32(0.0625)); fx1 = np.floor((px + hx) * f32(0.0625))
        fy0 = np.ceil((py - hy - f32(15.0)) * f32(0.0625)); fy1 = np.floor((py + hy) * f32(0.0625))
        lim = f32(1048576.0)
        finite = (np.abs(fx0) < lim) & (np.abs(fx1) < lim) & (np.abs(fy0) < lim) & (np.abs(fy1) < lim)
    keep_all = ~sane | ~finite
    i = lambda v: np.where(finite, v, 0).astype(np.int64)   # noqa: E731
    return i(fx0), i(fx1) + 1, i(fy0), i(fy1) + 1, keep_all, transparent


def binned_rect(px, py, a, b, c, op, rect):
    """preprocess.hip binned_rect: the 3-sigma rectangle `rect` cut to the alpha box -> (minx, miny, maxx, maxy,
    kept); kept False = no tile left (the Gaussian leaves the binning)."""
    minx, miny, maxx, maxy = (np.asarray(v).astype(np.int64).copy() for v in rect)
    x0, x1, y0, y1, keep_all, transparent = alpha_box_f32(px, py, a, b, c, op)
    cut = ~keep_all
    minx[cut] = np.maximum(minx, x0)[cut]; maxx[cut] = np.minimum(maxx, x1)[cut]
    miny[cut] = np.maximum(miny, y0)[cut]; maxy[cut] = np.minimum(maxy, y1)[cut]
    kept = ~transparent & (maxx > minx) & (maxy > miny)
    return minx, miny, maxx, maxy, kept


def accept_f32(px, py, a, b, c, op, X, Y):
    """The render's accept decision of splat i at pixel centres (X[i, :], Y[i, :]) -- blend_math.h pair_power /
    pair_alpha."""
    conic = np.stack([a, b, c], 1).astype(f32)[:, :, None]
    px, py, op = px[:, None], py[:, None], op[:, None]
    dx = px.astype(f32) - X.astype(f32)
    dy = py.astype(f32) - Y.astype(f32)
    with np.errstate(all="ignore"):
        p2 = device_power2(conic, dx, dy)
        G = np.exp2(p2)
        alpha = np.minimum(f32(0.99), op.astype(f32) * G)
        return ~(p2 > 0) & ~(alpha < f32(1.0 / 255.0))


def instance_counts(rect):
    minx, miny, maxx, maxy = rect
    return np.maximum(maxx - minx, 0) * np.maximum(maxy - miny, 0)


def accepted_outside(px, py, a, b, c, op, rect, chunk=40_000):
    """Brute force over the pixel centres of every tile the reference lists for a splat and the binned rectangle
    drops: how many of those pixels the render would accept (must be 0), and how many tiles were looked at."""
    minx, miny, maxx, maxy = (np.asarray(v).astype(np.int64) for v in rect)
    bx0, by0, bx1, by1, kept = binned_rect(px, py, a, b, c, op, rect)
    bx1 = np.where(kept, bx1, bx0); by1 = np.where(kept, by1, by0)        # nothing kept: every tile is dropped
    n = instance_counts((minx, miny, maxx, maxy))
    gid = np.repeat(np.arange(len(n)), n)
    local = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    w = np.maximum(maxx - minx, 1)[gid]
    tx = minx[gid] + local % w
    ty = miny[gid] + local // w
    dropped = ~((tx >= bx0[gid]) & (tx < bx1[gid]) & (ty >= by0[gid]) & (ty < by1[gid]))
    gid, tx, ty = gid[dropped], tx[dropped], ty[dropped]
    xs = np.tile(np.arange(TILE), TILE)[None, :]
    ys = np.repeat(np.arange(TILE), TILE)[None, :]
    bad = 0
    for s in range(0, len(gid), chunk):
        g = gid[s:s + chunk]
        X = tx[s:s + chunk, None] * TILE + xs
        Y = ty[s:s + chunk, None] * TILE + ys
        bad += int(accept_f32(px[g], py[g], a[g], b[g], c[g], op[g], X, Y).sum())
    return bad, len(gid)


# ---- splats by construction (2-D: centre, covariance after the +0.3 low-pass, opacity) -------------------------------
def splats_from_cov(px, py, s1, s2, theta, op, gx, gy):
    """sigma_1 >= sigma_2 (pixels, low-pass included) at angle theta -> the arrays the kernel derives from the 2-D
    covariance, in its float32 order (preprocess.hip project_and_bound): conic, radius, 3-sigma rectangle."""
    ct, st = np.cos(theta), np.sin(theta)
    cxx = (ct * ct * s1 * s1 + st * st * s2 * s2).astype(f32)
    cxy = (ct * st * (s1 * s1 - s2 * s2)).astype(f32)
    cyy = (st * st * s1 * s1 + ct * ct * s2 * s2).astype(f32)
    det = cxx * cyy - cxy * cxy
    det_inv = f32(1.0) / det
    a, b, c = cyy * det_inv, -cxy * det_inv, cxx * det_inv
    mid = f32(0.5) * (cxx + cyy)
    lam = mid + np.sqrt(np.maximum(f32(0.1), mid * mid - det))
    radius = np.ceil(f32(3.0) * np.sqrt(lam))
    px, py, op = px.astype(f32), py.astype(f32), op.astype(f32)
    ok = det != 0
    out = tuple(v[ok] for v in (px, py, a, b, c, op, radius))
    return out[:6] + (reference_rect(out[0], out[1], out[6], gx, gy),)


def constructed_splats(n, seed, W=96, H=64):
    """>= n splats on a W x H image: generic ones, and by construction opacities within +-5 % of 1/255 and of
    0.999/255, axis ratios up to 1000:1 at every orientation (det = a c - b^2 near cancellation around 45 degrees),
    centres on tile and image borders and off-screen."""
    rng = np.random.default_rng(seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    logu = lambda lo, hi, k: np.exp(rng.uniform(math.log(lo), math.log(hi), k))   # noqa: E731
    parts = []

    def add(k, s2, ratio, theta=None, op=None, px=None, py=None):
        theta = rng.uniform(0, math.pi, k) if theta is None else theta
        op = rng.uniform(0.0, 1.0, k) if op is None else op
        px = rng.uniform(-24, W + 24, k) if px is None else px
        py = rng.uniform(-24, H + 24, k) if py is None else py
        parts.append((px, py, ratio * s2, s2, theta, op))

    lp = math.sqrt(0.3)   # the low-pass floor of a projected sigma
    k = int(0.55 * n)
    add(k, logu(lp, 4.0, k), logu(1.0, 5.0, k))
    k = int(0.15 * n)     # opacities around the two thresholds
    thr = np.where(rng.random(k) < 0.5, 1.0 / 255.0, 0.999 / 255.0)
    add(k, logu(lp, 5.0, k), logu(1.0, 4.0, k), op=thr * (1.0 + rng.uniform(-0.05, 0.05, k)))
    k = int(0.10 * n)     # low opacities: the box is far inside the 3-sigma square
    add(k, logu(lp, 6.0, k), logu(1.0, 4.0, k), op=logu(1.0 / 255.0, 0.1, k))
    k = int(0.08 * n)     # centres on tile borders, image borders, and off-screen
    edge = lambda size, k: (rng.integers(-1, size // 16 + 2, k) * 16 + rng.choice([-0.5, 0.0, 15.0, 15.5], k)   # noqa: E731
                            + rng.choice([0.0, 1e-3, -1e-3, 1e-5], k))
    add(k, logu(lp, 4.0, k), logu(1.0, 6.0, k), px=edge(W, k), py=edge(H, k))
    k = int(0.09 * n)
    side = rng.random(k) < 0.5
    add(k, logu(lp, 8.0, k), logu(1.0, 6.0, k), px=np.where(side, rng.uniform(-150, -1, k), rng.uniform(W, W + 150, k)),
        py=rng.uniform(-100, H + 100, k))
    k = n - sum(len(p[0]) for p in parts) + 64   # axis ratios up to 1000:1 at every orientation
    grid = np.arange(k) * (math.pi / 64.0) + np.where(rng.random(k) < 0.5, 0.0, rng.uniform(-0.01, 0.01, k))
    add(k, logu(lp, 1.0, k), logu(10.0, 1000.0, k), theta=grid, op=logu(1.0 / 255.0, 1.0, k),
        px=rng.uniform(-200, W + 200, k), py=rng.uniform(-200, H + 200, k))
    cat = [np.concatenate([p[i] for p in parts]) for i in range(6)]
    return splats_from_cov(*cat, gx, gy)


# ---- the scenes of the GPU test ----------------------------------------------------------------------------------------
def scenes():
    """name -> (Scene, W, H).  P <= 3000, images from 48 x 32 to 200 x 120 (12.5 x 7.5 tiles: a partial tile column
    and row, two super-tiles)."""
    def toy(P, seed, scale, opacity=None, scales=None, **kw):
        sc = hz.toy_scene(P, seed=seed, sh_degree=1, scale=scale, **kw)
        g = torch.Generator().manual_seed(seed + 100)
        if scales is not None:
            sc = sc._replace(scales=scales(sc, g))
        if opacity is not None:
            sc = sc._replace(opacity=opacity(sc, g))
        return sc
    P = 3000
    sweep = lambda sc, g: (torch.linspace(0.90, 1.10, sc.opacity.shape[0]).reshape(-1, 1) / 255.0)[torch.randperm(sc.opacity.shape[0], generator=g)]   # noqa: E731
    thin = lambda sc, g: torch.cat([sc.scales[:, :1] * 12.0, sc.scales[:, 1:] * 0.05], 1)   # noqa: E731
    faint = lambda sc, g: torch.exp(torch.empty_like(sc.opacity).uniform_(math.log(1.2 / 255.0), math.log(0.08), generator=g))  # noqa: E731
    out = {
        "opacity_sweep": (toy(P, 11, 0.25, opacity=sweep), 200, 120),
        "elongated": (toy(P, 12, 0.08, scales=thin), 200, 120),
        "all_empty": (toy(400, 13, 0.2, opacity=lambda sc, g: torch.full_like(sc.opacity, 0.7 / 255.0)), 48, 32),
        "single": (toy(1, 14, 0.3, spread=0.05), 72, 40),
        "faint": (toy(P, 15, 0.35, opacity=faint), 200, 120),
    }
    big = toy(40, 16, 0.1)   # one splat over every tile, in front of a few small ones
    big = big._replace(means3D=torch.cat([torch.tensor([[0.0, 0.0, 3.0]]), big.means3D[1:]]),
                       scales=torch.cat([torch.tensor([[4.0, 4.0, 0.5]]), big.scales[1:]]),
                       rotations=torch.cat([torch.tensor([[1.0, 0.0, 0.0, 0.0]]), big.rotations[1:]]),
                       opacity=torch.cat([torch.tensor([[0.6]]), big.opacity[1:]]))
    out["one_covers_all"] = (big, 104, 72)
    return out


def camera(W, H, device="cpu"):
    return hz.trajectory_camera(0, W=W, H=H, device=device)


def predicted_counts(px, py, conic, op, radii, W, H):
    """(reference instances, binned instances, Gaussians kept, visible Gaussians) from per-Gaussian arrays as the
    preprocess leaves them (radii 0 = culled)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    vis = np.asarray(radii) > 0
    px, py, op = (np.asarray(v, dtype=f32).reshape(-1)[vis] for v in (px, py, op))
    conic = np.asarray(conic, dtype=f32)[vis]
    rect = reference_rect(px, py, np.asarray(radii)[vis], gx, gy)
    bx0, by0, bx1, by1, kept = binned_rect(px, py, conic[:, 0], conic[:, 1], conic[:, 2], op, rect)
    binned = int((instance_counts((bx0, by0, bx1, by1)) * kept).sum())
    return int(instance_counts(rect).sum()), binned, int(kept.sum()), int(vis.sum())


def oracle_counts(sc, W, H):
    """predicted_counts from the CPU oracle's preprocess of a scene."""
    from oracle import torch_splat as ts
    kw = hz.settings_kwargs(camera(W, H), sc.sh_degree)
    pre = ts.preprocess(sc.means3D, sc.opacity, image_height=H, image_width=W, tanfovx=kw["tanfovx"],
                        tanfovy=kw["tanfovy"], viewmatrix=kw["viewmatrix"], projmatrix=kw["projmatrix"],
                        campos=kw["campos"], sh_degree=sc.sh_degree, shs=sc.shs, scales=sc.scales,
                        rotations=sc.rotations)
    m2 = pre["means2D"].numpy()
    return predicted_counts(m2[:, 0], m2[:, 1], pre["conic"].numpy(), pre["opacity"].numpy(), pre["radii"].numpy(), W, H)


if __name__ == "__main__":
    for name, (sc, W, H) in scenes().items():
        R, B, kept, vis = oracle_counts(sc, W, H)
        print("%-16s P %5d  %3d x %3d  visible %5d kept %5d  instances %7d binned %7d  ratio %.3f" % (
            name, sc.means3D.shape[0], W, H, vis, kept, R, B, B / max(R, 1)))
