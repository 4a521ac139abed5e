"""Float64 truth of the sky cube map's composite and of its backward (csrc/sky.hip sky_backward_kernel), for
tests/test_sky_truth_host.py and tests/test_gpu_sky_backward.py, plus the case table both share.

  out_c  = rgb_c + clamp(sky_c, 0, 1) * (1 - acc),   sky_c = fetch ? sum_k w_k cube[idx_k, c] : fill

The taps (idx, w) are oracle/sky_torch.py cube_taps: face adjacency from the brute-force neighbour table, not from the
kernel's unfold-about-the-edge construction.  The directions are the float64 evaluation of the float32 ray matrix the
kernel is handed, at the sample positions the kernel forms ((float)px + ox in float32): the truth carries neither the
float32 error of the oracle's get_rays nor any rounding of the lookup.

  rays64            directions
  backward64        grad_cube, grad_acc and, per texel-channel / pixel-channel, what the tolerances are built from
  composite_torch64 the same composite with torch gathers, differentiable: only there to check backward64 by autograd
  rays32 / taps32 / backward32   the kernel's arithmetic in float32 numpy, one rounding per operation: shows on the
                    CPU that float32 alone stays inside the bars

Tolerances (eps = 2^-24, the unit roundoff of float32):
  weight allowance  dw = 16 res eps.  A ray component is three products and two sums, the face coordinate one product
                    and one sum more: a few eps absolute; u res - 0.5 scales that by res; a weight is a product of two
                    such fractions: roughly 10..20 res eps.
  sample            phi = dw S + 8 eps |s|,  S = sum_k |cube[idx_k]|
  grad_acc          |got - truth| <= sum_c |g_c| phi_c, every pixel
  fragile           a pixel-channel with |s| < phi or |s - 1| < phi: the clamp gate may legitimately fall either way
  grad_cube         |got - truth| <= dw B + (n + 8) eps A + F per texel-channel, none exempt, where n counts the
                    contributing terms, A = sum |tr w g|, B = sum |tr g| and F = sum |tr w g| over the fragile
                    contributors; (n + 8) eps A bounds n float32 atomic adds in any order.  Unhit texels: exactly 0.
"""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from oracle import sky_torch as st

EPS = 2.0 ** -24


def dw_of(res):
    return 16.0 * res * EPS


# ---------------------------------------------------------------------------------------------------------------
# float64 truth
# ---------------------------------------------------------------------------------------------------------------
def sample_positions32(H, W, jitter32=None):
    """(fx, fy) [H*W] float32, as pixel_ray forms them: (float)px + ox with ox = 0.5 or the jitter plane."""
    px = np.tile(np.arange(W, dtype=np.float32), H)
    py = np.repeat(np.arange(H, dtype=np.float32), W)
    if jitter32 is None:
        ox = oy = np.float32(0.5)
    else:
        j = np.asarray(jitter32, np.float32).reshape(2, H * W)
        ox, oy = j[0], j[1]
    return (px + ox).astype(np.float32), (py + oy).astype(np.float32)


def rays64(M32, H, W, jitter32=None):
    """[H*W,3] float64: normalize(M32 (x + ox, y + oy, 1)) with the float32 matrix and sample positions widened."""
    M = np.asarray(M32, np.float32).reshape(3, 3).astype(np.float64)
    fx, fy = sample_positions32(H, W, jitter32)
    p = np.stack([fx.astype(np.float64), fy.astype(np.float64), np.ones(H * W)], axis=1)
    d = p @ M.T
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def fetch_mask(H, W, acc=None, mask=None):
    """bool [H*W]: the kernel's rule (sky_math.h sky_fetches), in float32."""
    if mask is not None:
        return np.asarray(mask).reshape(-1) != 0
    if acc is None:
        return np.ones(H * W, bool)
    a32 = np.asarray(acc, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (np.float32(1) - a32) > np.float32(1e-3)       # NaN compares false


def backward64(cube, M32, H, W, grad, acc=None, mask=None, jitter=None, fill=0.0):
    cube = np.asarray(cube, np.float64)
    res = cube.shape[1]
    T = 6 * res * res
    texels = cube.reshape(T, 3)
    g = np.asarray(grad, np.float64).reshape(3, H * W).T                     # [N,3]
    N = H * W
    fetch = fetch_mask(H, W, acc, mask)
    tr = np.ones(N) if acc is None else 1.0 - np.asarray(acc, np.float32).reshape(-1).astype(np.float64)
    idx, w = st.cube_taps(res, rays64(M32, H, W, jitter))
    valid = idx >= 0
    tex = np.where(valid[:, :, None], texels[np.maximum(idx, 0)], 0.0)       # [N,4,3]
    s_fetch = (w[:, :, None] * tex).sum(axis=1)
    S_fetch = np.abs(tex).sum(axis=1)
    s = np.where(fetch[:, None], s_fetch, float(fill))
    S = np.where(fetch[:, None], S_fetch, 0.0)
    dw = dw_of(res)
    phi = dw * S + 8.0 * EPS * np.abs(s)
    gate = fetch[:, None] & (s >= 0.0) & (s <= 1.0)
    fragile = fetch[:, None] & ((np.abs(s) < phi) | (np.abs(s - 1.0) < phi))
    clamped = fetch[:, None] & ~gate
    grad_acc = -(np.clip(s, 0.0, 1.0) * g).sum(axis=1)

    grad_cube = np.zeros((T, 3))
    n = np.zeros((T, 3), np.int64)
    A, B, F = np.zeros((T, 3)), np.zeros((T, 3)), np.zeros((T, 3))
    for c in range(3):
        for k in range(4):
            on = valid[:, k] & gate[:, c]
            t, term = idx[on, k], tr[on] * w[on, k] * g[on, c]
            grad_cube[:, c] += np.bincount(t, weights=term, minlength=T)
            n[:, c] += np.bincount(t, minlength=T)
            A[:, c] += np.bincount(t, weights=np.abs(term), minlength=T)
            B[:, c] += np.bincount(t, weights=np.abs(tr[on] * g[on, c]), minlength=T)
            fr = valid[:, k] & fragile[:, c]
            F[:, c] += np.bincount(idx[fr, k], weights=np.abs(tr[fr] * w[fr, k] * g[fr, c]), minlength=T)
    shp = (6, res, res, 3)
    corner = fetch & (~valid).any(axis=1)
    face = idx // (res * res)
    own = st.dir_to_face_uv(rays64(M32, H, W, jitter))[0]
    leaves = fetch & (valid & (face != own[:, None])).any(axis=1)
    return dict(grad_cube=grad_cube.reshape(shp), grad_acc=grad_acc.reshape(H, W), n=n.reshape(shp), A=A.reshape(shp),
                B=B.reshape(shp), F=F.reshape(shp), s=s.T.reshape(3, H, W), S=S.T.reshape(3, H, W),
                phi=phi.T.reshape(3, H, W), fetch=fetch.reshape(H, W), gate=gate.T.reshape(3, H, W),
                fragile=fragile.T.reshape(3, H, W), clamped=clamped.T.reshape(3, H, W), idx=idx, w=w,
                corner=corner.reshape(H, W), leaves=leaves.reshape(H, W), faces=np.unique(own[fetch]), dw=dw,
                tol_cube=dw * B.reshape(shp) + (n.reshape(shp) + 8) * EPS * A.reshape(shp) + F.reshape(shp),
                tol_acc=(np.abs(g) * phi).sum(axis=1).reshape(H, W))


def composite_torch64(cube, rgb, acc, M32, H, W, mask=None, jitter=None, fill=0.0):
    """[3,H,W] float64 torch, differentiable w.r.t. cube, rgb and acc (float64 tensors; acc may be None: a lookup).
    The fetch rule reads the float32 rounding of acc, as the kernel does."""
    res = cube.shape[1]
    acc_np = None if acc is None else acc.detach().numpy().astype(np.float32)
    fetch = torch.from_numpy(np.nonzero(fetch_mask(H, W, acc_np, None if mask is None else np.asarray(mask)))[0])
    idx, w = st.cube_taps(res, rays64(M32, H, W, jitter)[fetch.numpy()])
    idx_t, w_t = torch.from_numpy(np.maximum(idx, 0)), torch.from_numpy(np.where(idx >= 0, w, 0.0))
    samp = (cube.reshape(-1, 3)[idx_t] * w_t[:, :, None]).sum(dim=1).clamp(0.0, 1.0)           # [n,3]
    sky = torch.full((H * W, 3), min(max(float(fill), 0.0), 1.0), dtype=torch.float64).index_copy(0, fetch, samp)
    sky = sky.t().reshape(3, H, W)
    if acc is None:
        return sky if rgb is None else rgb + sky
    return rgb + sky * (1.0 - acc.reshape(1, H, W))


# ---------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy (sky_math.h, statement by statement, one rounding per operation)
# ---------------------------------------------------------------------------------------------------------------
f32 = np.float32


def rays32(M32, H, W, jitter32=None):
    m = np.asarray(M32, f32).reshape(9)
    fx, fy = sample_positions32(H, W, jitter32)
    x = m[0] * fx + m[1] * fy + m[2]
    y = m[3] * fx + m[4] * fy + m[5]
    z = m[6] * fx + m[7] * fy + m[8]
    n = np.sqrt(x * x + y * y + z * z)
    return np.stack([x / n, y / n, z / n], axis=1)


def _face_uv32(x, y, z):
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    zf = az > np.maximum(ax, ay)
    yf = ~zf & (ay > ax)
    f = np.where(zf, np.where(z < 0, 5, 4), np.where(yf, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))
    mj = np.where(zf, az, np.where(yf, ay, ax))
    a = np.where(zf, np.where(z < 0, -x, x), np.where(yf, x, np.where(x < 0, z, -z)))
    b = np.where(zf, -y, np.where(yf, np.where(y < 0, -z, z), -y))
    h = f32(0.5) / mj
    u = np.clip(a * h + f32(0.5), f32(0), f32(1))
    v = np.clip(b * h + f32(0.5), f32(0), f32(1))
    return f, u.astype(f32), v.astype(f32)


def _cube_point32(f, a, b):
    d = np.zeros_like(a)
    d = np.where(a > 1, a - f32(1), np.where(a < -1, f32(-1) - a, d))
    a = np.clip(a, f32(-1), f32(1))
    d = np.where(b > 1, b - f32(1), np.where(b < -1, f32(-1) - b, d))
    b = np.clip(b, f32(-1), f32(1))
    n = f32(1) - d
    x = np.select([f == 0, f == 1, f == 5], [n, -n, -a], a)
    y = np.select([f == 2, f == 3], [n, -n], -b)
    z = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [-a, a, b, -b, n], -n)
    return x.astype(f32), y.astype(f32), z.astype(f32)


def taps32(d32, res):
    """(idx [N,4] int64, w [N,4] float32): sky_math.h cube_taps on float32 directions [N,3]."""
    d32 = np.asarray(d32, f32)
    r = f32(res)
    f, u, v = _face_uv32(d32[:, 0], d32[:, 1], d32[:, 2])
    fu, fv = u * r - f32(0.5), v * r - f32(0.5)
    flu, flv = np.floor(fu), np.floor(fv)
    iu0, iv0 = flu.astype(np.int64), flv.astype(np.int64)
    wu, wv = fu - flu, fv - flv
    N = d32.shape[0]
    idx, wgt, wsum = np.full((N, 4), -1, np.int64), np.zeros((N, 4), f32), np.zeros(N, f32)
    for k in range(4):
        iu, iv = iu0 + (k & 1), iv0 + (k >> 1)
        w = (wu if k & 1 else f32(1) - wu) * (wv if k >> 1 else f32(1) - wv)
        ou, ov = (iu < 0) | (iu >= res), (iv < 0) | (iv >= res)
        a = (iu.astype(f32) + f32(0.5)) * (f32(2) / r) - f32(1)
        b = (iv.astype(f32) + f32(0.5)) * (f32(2) / r) - f32(1)
        nf, nu, nv = _face_uv32(*_cube_point32(f, a, b))
        cu = np.clip(np.floor(nu * r).astype(np.int64), 0, res - 1)
        cv = np.clip(np.floor(nv * r).astype(np.int64), 0, res - 1)
        edge = ou ^ ov
        ok = ~(ou & ov)
        face, tu, tv = np.where(edge, nf, f), np.where(edge, cu, iu), np.where(edge, cv, iv)
        idx[:, k] = np.where(ok, (face * res + tv) * res + tu, -1)
        wgt[:, k] = np.where(ok, w, f32(0))
        wsum = wsum + wgt[:, k]
    inv = f32(1) / np.where(wsum > 0, wsum, f32(1))
    return idx, (wgt * inv[:, None]).astype(f32)


def backward32(cube, M32, H, W, grad, acc=None, mask=None, jitter=None, fill=0.0):
    """sky_backward_kernel in float32 numpy; the scattered float32 terms are summed in float64 (the order of the
    kernel's atomic adds is not defined; its bound is the (n + 8) eps A term).  -> grad_cube, grad_acc, idx, w."""
    cube = np.asarray(cube, f32)
    res = cube.shape[1]
    T, N = 6 * res * res, H * W
    g = np.asarray(grad, f32).reshape(3, N).T
    fetch = fetch_mask(H, W, acc, mask)
    tr = np.ones(N, f32) if acc is None else f32(1) - np.asarray(acc, f32).reshape(-1)
    idx, w = taps32(rays32(M32, H, W, jitter), res)
    texels = cube.reshape(T, 3)
    s = np.zeros((N, 3), f32)
    for k in range(4):
        ok = idx[:, k] >= 0
        s = s + np.where(ok[:, None], w[:, k, None] * texels[np.maximum(idx[:, k], 0)], f32(0))
    s = np.where(fetch[:, None], s, f32(fill)).astype(f32)
    gate = fetch[:, None] & ~((s < 0) | (s > 1))
    grad_cube = np.zeros((T, 3))
    for c in range(3):
        for k in range(4):
            on = (idx[:, k] >= 0) & gate[:, c]
            term = (tr[on] * w[on, k]) * g[on, c]
            grad_cube[:, c] += np.bincount(idx[on, k], weights=term.astype(np.float64), minlength=T)
    ga = np.zeros(N, f32)
    for c in range(3):
        ga = ga - np.clip(s[:, c], f32(0), f32(1)) * g[:, c]
    return dict(grad_cube=grad_cube.reshape(6, res, res, 3), grad_acc=ga.reshape(H, W), idx=idx, w=w)


def max_weight_error(idx_a, w_a, idx_b, w_b, rows):
    """max over the rows and over texel ids of |w_a - w_b|, the taps matched by texel id: a texel only one side
    reads compares its weight with 0."""
    worst = 0.0
    ia, wa, ib, wb = idx_a[rows], np.asarray(w_a, np.float64)[rows], idx_b[rows], np.asarray(w_b, np.float64)[rows]
    for (i1, w1, i2, w2) in ((ia, wa, ib, wb), (ib, wb, ia, wa)):
        for k in range(4):
            has = i1[:, k] >= 0
            same = (i2 == i1[:, k, None]) & has[:, None]
            other = np.where(same, w2, 0.0).sum(axis=1)
            mine = np.where((i1 == i1[:, k, None]) & has[:, None], w1, 0.0).sum(axis=1)   # res 1, 2: a texel twice
            worst = max(worst, float(np.abs(mine - other)[has].max(initial=0.0)))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
FACE = (0.3, -0.25)
CORNER = (math.atan2(1.0, 1.0), -math.atan2(1.0, math.sqrt(2.0)))

# mode: composite (acc given), lookup (acc None), mask_jitter (explicit mask + jitter, acc given), acc_jitter (the acc
# rule, jittered), acc_edge (the acc rule with rows at 1.0, float32(0.999), 1.0005, 0.0 and some NaN)
Case = namedtuple("Case", "name res H W view yaw pitch focal mode fill mdev seed")


def _c(res, hw, view, yp, focal, mode, fill=0, mdev=False, seed=0):
    name = "r%d_%dx%d_%s_f%g_%s_fill%d_%s" % (res, hw[0], hw[1], view, focal, mode, fill, "dev" if mdev else "host")
    return Case(name, res, hw[0], hw[1], view, yp[0], yp[1], focal, mode, float(fill), mdev, seed)


CASES = [
    # every resolution at the three large sizes: a corner view, a wide view and the face view
    _c(1, (61, 67), "corner", CORNER, 0.55, "composite", 0, False),
    _c(1, (72, 120), "wide", (2.2, 0.5), 0.25, "lookup", 0, True),
    _c(1, (130, 257), "face", FACE, 0.55, "mask_jitter", 1, False),
    _c(2, (61, 67), "corner", CORNER, 0.55, "mask_jitter", 0, True),
    _c(2, (72, 120), "wide", (-1.0, 0.3), 0.2, "composite", 1, False),
    _c(2, (130, 257), "face", FACE, 0.55, "acc_jitter", 0, False, seed=1),
    _c(3, (61, 67), "corner", CORNER, 0.55, "lookup", 1, False),
    _c(3, (72, 120), "wide", (0.8, -0.6), 0.3, "acc_jitter", 1, True),
    _c(3, (130, 257), "face", FACE, 0.55, "composite", 0, True),
    _c(16, (61, 67), "corner", CORNER, 1.5, "acc_jitter", 0, False),
    _c(16, (72, 120), "wide", (2.2, 0.5), 0.2, "mask_jitter", 0, False),
    _c(16, (130, 257), "face", FACE, 0.55, "lookup", 0, False),
    _c(16, (130, 257), "corner", CORNER, 0.55, "composite", 1, True),
    _c(64, (61, 67), "corner", CORNER, 8.0, "composite", 0, False),
    _c(64, (72, 120), "wide", (0.8, -0.6), 0.25, "lookup", 0, False),
    _c(64, (130, 257), "face", FACE, 0.55, "mask_jitter", 1, True),
    _c(64, (130, 257), "corner", CORNER, 8.0, "acc_jitter", 0, False),
    # the acc rule at its threshold, NaN included
    _c(16, (61, 67), "face", FACE, 0.55, "acc_edge", 1, False),
    _c(3, (61, 67), "wide", (-1.0, 0.3), 0.3, "acc_edge", 0, True),
    # images smaller than, and exactly, one workgroup
    _c(1, (1, 1), "face", FACE, 0.55, "composite", 1, False),
    _c(16, (1, 1), "face", (1.9, 0.45), 0.55, "lookup", 0, True),
    _c(2, (5, 7), "wide", (2.2, 0.5), 0.2, "composite", 0, False),
    _c(3, (5, 7), "face", FACE, 0.55, "mask_jitter", 1, False),
    _c(64, (5, 7), "wide", (0.8, -0.6), 0.3, "acc_jitter", 0, True),
    _c(1, (4, 64), "wide", (0.0, 0.1), 0.2, "acc_jitter", 1, False),
    _c(3, (4, 64), "face", FACE, 0.55, "lookup", 0, False),
    _c(16, (4, 64), "wide", (0.0, 0.1), 0.3, "composite", 0, True),
    _c(64, (4, 64), "face", FACE, 0.55, "composite", 1, False),
    _c(2, (4, 64), "corner", CORNER, 0.55, "mask_jitter", 0, False),
    _c(64, (61, 67), "wide", (2.2, 0.5), 0.2, "mask_jitter", 0, False),
]
CASE_NAMES = [c.name for c in CASES]
LARGE = (61, 67)       # "at least 61 x 67": both extents


def is_large(case):
    return case.H >= LARGE[0] and case.W >= LARGE[1]


ACC_EDGE_VALUES = (1.0, float(np.float32(0.999)), 1.0005, 0.0)


def case_inputs(case):
    """The float32 inputs of a case, as CPU torch tensors: cube, M (ray matrix), g, acc / mask / jitter or None."""
    from gaussianrpg_amd.sky import ray_matrix
    from test_sky import _camera
    K, w2c = _camera(case.W, case.H, case.yaw, case.pitch, case.focal)
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) + case.seed)
    H, W, res = case.H, case.W, case.res
    cube = torch.rand(6, res, res, 3, generator=gen) * 1.6 - 0.3
    g = torch.randn(3, H, W, generator=gen)
    acc = torch.rand(1, H, W, generator=gen) * 0.95
    mask = torch.rand(H, W, generator=gen) > 0.4
    jitter = torch.rand(2, H, W, generator=gen)
    if case.mode == "lookup":
        acc = None
    if case.mode == "acc_edge":
        for i, v in enumerate(ACC_EDGE_VALUES):
            acc[0, 3 + 2 * i] = v
        acc[0, 20, ::5] = float("nan")
        acc[0, 40:43, 11] = float("nan")
    if case.mode != "mask_jitter":
        mask = None
    if case.mode not in ("mask_jitter", "acc_jitter"):
        jitter = None
    return dict(cube=cube, M=ray_matrix(K, w2c), g=g, acc=acc, mask=mask, jitter=jitter, fill=case.fill)


def _np(t):
    return None if t is None else t.numpy()


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """(inputs, backward64 of them); computed once per session and shared -- treat as read-only."""
    case = CASES[CASE_NAMES.index(name)]
    i = case_inputs(case)
    t = backward64(_np(i["cube"]), _np(i["M"]), case.H, case.W, _np(i["g"]), acc=_np(i["acc"]), mask=_np(i["mask"]),
                   jitter=_np(i["jitter"]), fill=case.fill)
    return i, t


def case_shares(case, t):
    """The measured conditions of section "Conditions on the table"."""
    fetched = int(t["fetch"].sum()) * 3
    hit = t["n"] > 0
    return dict(corner_pixels=int(t["corner"].sum()), faces=int(len(t["faces"])), leaving_pixels=int(t["leaves"].sum()),
                fetched_channels=fetched, clamped_channels=int(t["clamped"].sum()),
                clamped_share=float(t["clamped"].sum() / max(fetched, 1)),
                fragile_share=float(t["fragile"].sum() / max(fetched, 1)),
                texels_F_share=float(((t["F"] > 0.01 * t["A"]) & hit).sum() / max(int(hit.sum()), 1)))


def check_case_conditions(case, t):
    """Asserted on the truth alone, on the CPU and again in the GPU test."""
    sh = case_shares(case, t)
    if case.view == "corner":
        assert sh["corner_pixels"] >= 10, (case.name, sh)
    if case.view == "wide":
        assert sh["faces"] >= 3, (case.name, sh)
    if is_large(case):
        assert sh["leaving_pixels"] > 0, (case.name, sh)
        assert sh["clamped_share"] >= 0.01 and sh["clamped_channels"] >= 50, (case.name, sh)
    assert sh["fragile_share"] <= 0.002, (case.name, sh)
    assert sh["texels_F_share"] <= 0.01, (case.name, sh)
    return sh


def cube_ratio(got, t):
    """worst |got - truth| / tol over the hit texel-channels, and whether every unhit one is exactly 0.0."""
    err = np.abs(np.asarray(got, np.float64).reshape(t["grad_cube"].shape) - t["grad_cube"])
    hit = t["n"] > 0
    frag_only = ~hit & (t["F"] > 0)            # hit by nothing the truth's gate lets through, but by a fragile pixel
    unhit = ~hit & ~frag_only
    ratio = float((err[hit] / t["tol_cube"][hit]).max(initial=0.0))
    if frag_only.any():
        ratio = max(ratio, float((err[frag_only] / t["tol_cube"][frag_only]).max()))
    zeros_ok = bool((np.asarray(got).reshape(err.shape)[unhit] == 0.0).all())
    return ratio, zeros_ok


def acc_ratio(got, t):
    """worst |got - truth| / tol over the pixels; a zero tolerance asks for equality."""
    got = np.asarray(got, np.float64).reshape(t["grad_acc"].shape)
    if not np.isfinite(got).all():
        return float("inf")
    err, tol = np.abs(got - t["grad_acc"]), t["tol_acc"]
    pos = tol > 0
    if (err[~pos] != 0).any():
        return float("inf")
    return float((err[pos] / tol[pos]).max(initial=0.0))
