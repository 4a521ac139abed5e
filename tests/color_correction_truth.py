"""Float64 truth of the frame's colour correction (csrc/color_correction.hip) and of its backward, with and without
the sky composite in front, for tests/test_color_correction_host.py and tests/test_gpu_color_correction.py, plus the
input builders both share.

  x   = rgb                                    or, with the sky inputs,  rgb + clamp(sky, 0, 1) * (1 - acc)
  y_i = A_i0 x_0 + A_i1 x_1 + A_i2 x_2 + A_i3  (clamped to [0,1] in evaluation)
  g_x = A[:, :3]^T g,   grad_A[i][j] = sum_pixels g_i x_j,   grad_A[i][3] = sum_pixels g_i

Without the composite x is the float32 input widened: the truth carries no rounding at all.  With it, the sky part is
tests/sky_truth.py (backward64: the float64 sample s of the float32 ray matrix the kernel is handed, and its tolerance
phi) and x64 = rgb + clip(s, 0, 1) * (1 - acc).

Tolerances (u = 2^-24, the unit roundoff of float32):
  forward   |y - y64| <= 4 u (sum_j |A_ij| |x_j| + |A_i3|) per element.  The value is three products and three
            additions; in any order, fused or not, each of the four terms passes at most four roundings (its product,
            at most three additions), and first-order error analysis gives the bound.  The kernel's three fused
            multiply-adds make three roundings.
  g_x       |g_x - g_x64| <= 3 u sum_i |A_ij| |g_i|: three products, two additions, every term at most three roundings.
  sums      |S - S64| <= (d + 1) u sum |g_i x_j|: one rounding of each product, then a summation tree in which no term
            passes more than d additions (the standard bound of a fixed tree, first order).  d is what the kernel
            documents: 6 (butterfly over the 64 lanes) + 3 (the four waves) + max(0, ceil(nb / 1024) - 1) (the strided
            loop of the final reduction) + 10 (its tree), nb = ceil(W / 64) ceil(H / 4) workgroups.  For j = 3 the term
            is g_i itself.
  with the composite, x carries its own tolerance
            tol_x = (1 - acc) phi + 4 u (|rgb| + |sky (1 - acc)|)
            (phi: sky_truth's sample tolerance; 1 - acc, the product and the sum are one rounding each, with one to
            spare), which enters the forward as sum_j |A_ij| tol_x_j and a sum as sum |g_i| tol_x_j; g_x does not
            depend on x.  A sample within phi of 0 or 1 may clamp either way; the difference is inside phi.
  clamp     clip is 1-Lipschitz and exact: the clamped planes keep the forward's tolerance.
  bytes     (unsigned char)(clip(v) * 255 + bias): a truth value v64 whose v64 * 255 + bias lies within
            255 tol + 2 u 256 of an integer k in 1 .. 255 (the values at which the byte changes) may legitimately give
            either byte ("fragile"); every other byte is determined.
"""
import functools
import hashlib

import numpy as np
import torch

import sky_truth as ST

U = 2.0 ** -24

# H x W of the GPU cases: the kernels tile 64 x 4 like the sky kernels
SHAPES = [(1, 1), (5, 67), (9, 130), (373, 707)]
MATRICES = ["identity", "near", "wide"]


def blocks(H, W):
    return ((W + 63) // 64) * ((H + 3) // 4)


def chain_depth(H, W):
    """d of color_correction.hip's header: the longest chain of additions one of the twelve sums passes through."""
    return 19 + max(0, -(-blocks(H, W) // 1024) - 1)


# ---------------------------------------------------------------------------------------------------------------
# input builders (legacy numpy RandomState: stable across versions)
# ---------------------------------------------------------------------------------------------------------------
def build_affine(kind, seed=0):
    """float32 [3,4]: identity, or eye(4)[:3] + s * uniform(-1, 1) with s = 0.1 ("near") / 1.0 ("wide")."""
    eye = np.eye(4, dtype=np.float32)[:3]
    if kind == "identity":
        return eye.copy()
    s = {"near": 0.1, "wide": 1.0}[kind]
    rng = np.random.RandomState(1000 + seed)
    return (eye + s * rng.uniform(-1.0, 1.0, (3, 4))).astype(np.float32)


def build_image(H, W, seed=0):
    """float32 [3,H,W] in [-0.15, 1.15): slightly outside [0,1] so that the clamp binds."""
    rng = np.random.RandomState(2000 + seed)
    return (rng.uniform(-0.15, 1.15, (3, H, W))).astype(np.float32)


def build_grad(H, W, seed=0):
    rng = np.random.RandomState(3000 + seed)
    return rng.normal(0.0, 1.0, (3, H, W)).astype(np.float32)


def build_case(builder, args):
    """A named input, as the golden fixture records them."""
    return {"affine": build_affine, "image": build_image, "grad": build_grad}[builder](**args)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def sky_case(H, W, mode="composite", fill=0, res=16, seed=0, mdev=False):
    """A sky_truth case of this frame size (corner view: taps across edges and corners, samples that clamp)."""
    return ST._c(res, (H, W), "corner", ST.CORNER, 0.55, mode, fill, mdev, seed)


@functools.lru_cache(maxsize=None)
def sky_inputs(H, W, mode="composite", fill=0, res=16, seed=0):
    """(numpy inputs, x64, tol_x) of a composite in front of the correction; computed once -- treat as read-only.
    inputs: cube, M, acc, mask, jitter (None where the mode has none), rgb, fill."""
    case = sky_case(H, W, mode, fill, res, seed)
    i = {k: (None if v is None else (v.numpy() if isinstance(v, torch.Tensor) else v))
         for k, v in ST.case_inputs(case).items()}
    i["rgb"] = build_image(H, W, seed=77 + seed)
    x64, tol_x = composite64(i, H, W)
    return i, x64, tol_x


def composite64(i, H, W):
    """x64 [3,H,W] and its tolerance for the kernel's float32 composite."""
    t = ST.backward64(i["cube"], i["M"], H, W, np.zeros((3, H, W)), acc=i["acc"], mask=i["mask"], jitter=i["jitter"],
                      fill=i["fill"])
    tr = 1.0 - np.asarray(i["acc"], np.float32).reshape(1, H, W).astype(np.float64)
    sky = np.clip(t["s"], 0.0, 1.0)
    rgb = np.asarray(i["rgb"], np.float64)
    x64 = rgb + sky * tr
    tol_x = np.abs(tr) * t["phi"] + 4.0 * U * (np.abs(rgb) + np.abs(sky * tr))
    return x64, tol_x


# ---------------------------------------------------------------------------------------------------------------
# float64 truth
# ---------------------------------------------------------------------------------------------------------------
def forward64(A, x, tol_x=None, clamp=False):
    """(y64 [3,H,W], tol [3,H,W])."""
    A = np.asarray(A, np.float64)
    x = np.asarray(x, np.float64)
    y = np.einsum("ij,jhw->ihw", A[:, :3], x) + A[:, 3, None, None]
    tol = 4.0 * U * (np.einsum("ij,jhw->ihw", np.abs(A[:, :3]), np.abs(x)) + np.abs(A[:, 3, None, None]))
    if tol_x is not None:
        tol = tol + np.einsum("ij,jhw->ihw", np.abs(A[:, :3]), tol_x)
    return (np.clip(y, 0.0, 1.0) if clamp else y), tol


def backward64(A, x, g, tol_x=None):
    """dict(g_x, tol_g_x [3,H,W]; grad_A, tol_A [3,4])."""
    A = np.asarray(A, np.float64)
    x = np.asarray(x, np.float64)
    g = np.asarray(g, np.float64)
    H, W = x.shape[1:]
    g_x = np.einsum("ij,ihw->jhw", A[:, :3], g)
    tol_g_x = 3.0 * U * np.einsum("ij,ihw->jhw", np.abs(A[:, :3]), np.abs(g))
    x1 = np.concatenate([x, np.ones((1, H, W))], axis=0)
    grad_A = np.einsum("ihw,jhw->ij", g, x1)
    tol_A = (chain_depth(H, W) + 1) * U * np.einsum("ihw,jhw->ij", np.abs(g), np.abs(x1))
    if tol_x is not None:
        tol_A[:, :3] += np.einsum("ihw,jhw->ij", np.abs(g), tol_x)
    return dict(g_x=g_x, tol_g_x=tol_g_x, grad_A=grad_A, tol_A=tol_A)


def ratio(got, truth, tol):
    """worst |got - truth| / tol; a zero tolerance asks for equality; a non-finite value is infinitely wrong."""
    got = np.asarray(got, np.float64).reshape(np.shape(truth))
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - truth)
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    pos = tol > 0
    if (err[~pos] != 0).any():
        return float("inf")
    return float((err[pos] / tol[pos]).max(initial=0.0))


def fragile_bytes(y64, tol, truncate=True):
    """bool [3,H,W]: the byte of this value is not determined by the truth and the forward bound (module docstring)."""
    v = np.asarray(y64, np.float64) * 255.0 + (0.0 if truncate else 0.5)      # unclamped: the byte of a value well
    k = np.rint(v)                                                            # outside [0,1] is 0 or 255 for certain
    return (np.abs(v - k) <= 255.0 * tol + 512.0 * U) & (k >= 1) & (k <= 255)


def bytes64(y64, truncate=True):
    """uint8 [H,W,3] of the truth."""
    v = np.clip(y64, 0.0, 1.0) * 255.0 + (0.0 if truncate else 0.5)
    return np.floor(v).astype(np.uint8).transpose(1, 2, 0)


# ---------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy: shows on the CPU that float32 alone stays inside the bounds
# ---------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32 fma through float64: a * b is exact in float64, the sum rounds once to float64 and once to float32 --
    a double rounding that can differ from a true fma by one float32 ulp in rare ties; inside the bounds either way."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def forward32(A, x):
    A = np.asarray(A, np.float32)
    x = np.asarray(x, np.float32)
    return np.stack([_fma32(A[i, 2], x[2], _fma32(A[i, 1], x[1], _fma32(A[i, 0], x[0], A[i, 3]))) for i in range(3)])


def backward32(A, x, g):
    """g_x as the kernel forms it; the twelve sums over float32 products in the kernel's add order."""
    A = np.asarray(A, np.float32)
    x = np.asarray(x, np.float32)
    g = np.asarray(g, np.float32)
    H, W = x.shape[1:]
    g_x = np.stack([_fma32(A[2, j], g[2], _fma32(A[1, j], g[1], A[0, j] * g[0])) for j in range(3)])
    x1 = np.concatenate([x, np.ones((1, H, W), np.float32)], axis=0)
    gy, gx = (H + 3) // 4, (W + 63) // 64
    grad_A = np.zeros((3, 4), np.float32)
    for i in range(3):
        for j in range(4):
            term = np.zeros((gy * 4, gx * 64), np.float32)
            term[:H, :W] = g[i] * x1[j] if j < 3 else g[i]
            t = term.reshape(gy, 4, gx, 64).transpose(0, 2, 1, 3)            # [by, bx, wave, lane]
            for d in (32, 16, 8, 4, 2, 1):                                   # butterfly: lane l reads l ^ d
                t = t + t[..., np.arange(64) ^ d]
            w = t[..., 0]
            part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
            p = part.reshape(-1)
            slots = np.zeros(1024, np.float32)
            for s in range(0, p.size, 1024):
                chunk = p[s:s + 1024]
                slots[:chunk.size] = slots[:chunk.size] + chunk
            n = 512
            while n >= 1:
                slots[:n] = slots[:n] + slots[n:2 * n]
                n //= 2
            grad_A[i, j] = slots[0]
    return g_x, grad_A
