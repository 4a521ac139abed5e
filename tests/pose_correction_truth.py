"""Float64 truth of the background's pose correction (csrc/pose_correction.hip) and of its backward, for
tests/test_pose_correction_host.py and tests/test_gpu_pose_correction.py, plus the input builders both share.

  q^  = rot / max(|rot|, 1e-12)          F.normalize
  u   = q^ / |q^|,  R = R(u)             quaternion_to_matrix (general_utils.py:125-146)
  xyz'      = R xyz + trans
  rotation' = q^ (x) rotation            quaternion_raw_multiply, NOT normalised behind it (camera_pose.py:112)
  g_xyz = R^T g_xyz',  g_rotation = the product's transpose in b,  g_trans = sum g_xyz',
  g_rot = d q^/d rot^T (d u/d q^^T dR/du^T[sum g_xyz' xyz^T] + sum of the product's transpose in a)

The truth is the same expressions in float64 on the float32 inputs widened; backward64's chain is checked against
float64 autograd through the reference's own lines by the host test.

Tolerances (u = 2^-24, the unit roundoff of float32; first order; every count is the number of roundings on a term's
path, the kernel's divisions and square roots being correctly rounded):
  q^_k      4u |q^_k|: the squared norm's terms pass 1 product and at most 3 additions (4u, relative, positive terms),
            the root halves that and rounds once (3u), the division rounds once.                              Q_ROUND = 4
  u_k       6u |u_k|: the error n1 shares across the components is a scaling and cancels in q^ / |q^|; left are the
            first division's own rounding (1), |q^| computed from those (a weighted mean of them: 1), n2's own error
            (3, as n1) and the second division (1).                                                           U_ROUND = 6
  R_ij      off the diagonal 2 (a b -+ c d): each product carries its two factors' errors and its rounding (2 * 6 + 1),
            the sum rounds once, the doubling is exact: 2 * 14u (|a b| + |c d|).                              R_ROUND = 14
            on the diagonal 1 - 2 (a a + b b): 2 * 14u (a a + b b) likewise, plus u |R_ii| for the subtraction.
  xyz'_i    sum_j tol_R_ij |x_j| + 4u (sum_j |R_ij x_j| + |t_i|): a term passes its product and at most three
            additions.                                                                                        XYZ_ROUND = 4
  rot'_k    8u sum |q^_m b_n| over the component's four terms: q^'s error (4), the product (1), at most three
            additions.                                                                                        QMUL_ROUND = 8
  g_xyz_j   sum_i tol_R_ij |g_i| + 3u sum_i |R_ij g_i|: product and two additions.                            GXYZ_ROUND = 3
  g_rot'n_k 8u sum |q^_m g_n|, as rot'_k.
  sums      a sum of N summands passes a fixed tree in which no summand passes more than d additions (the kernel's
            header): d = 6 (butterfly over the 64 lanes) + 3 (the four waves) + max(0, ceil(nb / 1024) - 1) (the strided
            loop of the finishing workgroup) + 10 (its tree), nb = ceil(N / 256).
              sum g_i          d u sum |g_i|                    the summand is the input itself
              sum g_i x_j      (d + 1) u sum |g_i x_j|          one product
              sum pa_k         (d + 4) u sum sum |b_m g_n|      pa_k: four products, three additions: a term passes 4
  composed  the composed route (compose_math.h compose_one's rigid path on the RAW row) against the same truth: R from ONE
            normalisation has fewer roundings than R_ROUND allows and xyz' the same operation order, so tol_xyz holds; its
            rotation' is normalize(rot (x) b') with b' its own activation of the raw rotation: b' against the b the truth
            is given (4, as q^), the product and three additions (4), the norm and the division behind it (4, as q^),
            and |b| itself, which the truth does not divide by, off 1 by its own rounding (4).             COMPOSED_QMUL_ROUND = 16
            Its pose gradient chains PER ROW and sums with float atomics; against the bar of DESIGN.md section 9,
            |A - T| / S <= max(4 |Y - T| / S, K u), K counts the reduction (6 butterfly levels, 3 LDS additions, one global
            addition per workgroup of the model) and the roundings a row's contribution carries before it (R's 2 * 14,
            the product's 8, the chain's 16): composed_pose_k(N).
  g_rot     chained ONCE from the sums by thread 0; chain64 propagates the sums' tolerances through the chain's
            absolute coefficients and adds, per step, (roundings of the step + the factor's own error) u |term|; the
            counts stand next to each step in chain64.
"""
import hashlib

import numpy as np

U = 2.0 ** -24
Q_ROUND, U_ROUND, R_ROUND, XYZ_ROUND, QMUL_ROUND, GXYZ_ROUND = 4, 6, 14, 4, 8, 3
COMPOSED_QMUL_ROUND = 16

ROWS = ["near", "wide", "norm3", "small"]
BLOCK = 256            # rows per workgroup (PC_THREADS)
REDUCE_THREADS = 1024
# 1 .. 257: inside one wave, the wave and workgroup boundaries; REDUCE_THREADS * BLOCK + 1: the smallest N at which the
# finishing workgroup's per-thread loop takes a second partial; the last: beyond that and no multiple of the workgroup
SIZES = [1, 63, 64, 65, 257, REDUCE_THREADS * BLOCK + 1, REDUCE_THREADS * BLOCK + 3 * BLOCK + 77]


def blocks(N):
    return -(-N // BLOCK)


def chain_depth(N):
    """d of pose_correction.hip's header: the longest chain of additions one of the sixteen sums passes through."""
    return 19 + max(0, -(-blocks(N) // REDUCE_THREADS) - 1)


def composed_pose_k(N):
    """K of the composed route's pose gradient (module docstring)."""
    return (6 + 3 + blocks(N)) + 2 * R_ROUND + QMUL_ROUND + 16


# ---------------------------------------------------------------------------------------------------------------
# input builders (legacy numpy RandomState: stable across versions)
# ---------------------------------------------------------------------------------------------------------------
def build_row(kind, seed=0):
    """(rot float32 [4] raw (w,x,y,z), trans float32 [3]).  near: what training produces, (1,0,0,0) + 0.01 noise and
    centimetres of translation; wide: any rotation, metres; norm3 / small: the wide row's direction at norm 3 / 1e-3
    (both normalisations do work)."""
    rng = np.random.RandomState(4000 + seed)
    if kind == "near":
        rot = np.array([1.0, 0, 0, 0]) + 0.01 * rng.uniform(-1, 1, 4)
        return rot.astype(np.float32), (0.05 * rng.uniform(-1, 1, 3)).astype(np.float32)
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    q *= {"wide": 1.0, "norm3": 3.0, "small": 1e-3}[kind]
    return q.astype(np.float32), rng.uniform(-2, 2, 3).astype(np.float32)


def build_xyz(N, seed=0):
    """float32 [N,3]: a street's extent in metres."""
    return np.random.RandomState(5000 + seed).uniform(-60, 60, (N, 3)).astype(np.float32)


def build_rotation(N, seed=0):
    """float32 [N,4]: activated (unit to rounding) quaternions, what get_rotation hands the correction."""
    q = np.random.RandomState(6000 + seed).normal(0, 1, (N, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def build_grad(N, C, seed=0):
    return np.random.RandomState(7000 + seed).normal(0, 1, (N, C)).astype(np.float32)


def build_case(builder, args):
    """A named input, as the golden fixture records them."""
    return {"row": build_row, "xyz": build_xyz, "rotation": build_rotation, "grad": build_grad}[builder](**args)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------
# float64 truth
# ---------------------------------------------------------------------------------------------------------------
def _matrix(u):
    r, x, y, z = u
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def _matrix_tol(u, R):
    r, x, y, z = np.abs(u)
    off = lambda a, b, c, d: 2 * R_ROUND * U * (a * b + c * d)                                   # noqa: E731
    dia = lambda a, b, Rii: 2 * R_ROUND * U * (a * a + b * b) + U * abs(Rii)                     # noqa: E731
    return np.array([[dia(y, z, R[0, 0]), off(x, y, r, z), off(x, z, r, y)],
                     [off(x, y, r, z), dia(x, z, R[1, 1]), off(y, z, r, x)],
                     [off(x, z, r, y), off(y, z, r, x), dia(x, y, R[2, 2])]])


def row64(rot):
    """dict(q, u, n1, n2, R, tol_R) of a raw row in float64."""
    rot = np.asarray(rot, np.float64)
    n1 = max(np.sqrt((rot * rot).sum()), 1e-12)
    q = rot / n1
    n2 = np.sqrt((q * q).sum())
    u = q / n2
    R = _matrix(u)
    return dict(q=q, u=u, n1=n1, n2=n2, R=R, tol_R=_matrix_tol(u, R))


# the Hamilton product a (x) b as a [4,4,4] sign table: out_k = sum_{m,n} H[k,m,n] a_m b_n
H = np.zeros((4, 4, 4))
for _k, _terms in enumerate([[(0, 0, 1), (1, 1, -1), (2, 2, -1), (3, 3, -1)], [(0, 1, 1), (1, 0, 1), (2, 3, 1), (3, 2, -1)],
                             [(0, 2, 1), (1, 3, -1), (2, 0, 1), (3, 1, 1)], [(0, 3, 1), (1, 2, 1), (2, 1, -1), (3, 0, 1)]]):
    for _m, _n, _s in _terms:
        H[_k, _m, _n] = _s


def forward64(rot, trans, xyz=None, rotation=None):
    """dict(xyz, tol_xyz [N,3]; rotation, tol_rotation [N,4]) -- the entries of the inputs that are given."""
    p = row64(rot)
    out = {}
    if xyz is not None:
        x = np.asarray(xyz, np.float64)
        t = np.asarray(trans, np.float64)
        out["xyz"] = x @ p["R"].T + t
        out["tol_xyz"] = np.abs(x) @ p["tol_R"].T + XYZ_ROUND * U * (np.abs(x) @ np.abs(p["R"]).T + np.abs(t))
    if rotation is not None:
        b = np.asarray(rotation, np.float64)
        out["rotation"] = np.einsum("kmn,m,in->ik", H, p["q"], b)
        out["tol_rotation"] = QMUL_ROUND * U * np.einsum("kmn,m,in->ik", np.abs(H), np.abs(p["q"]), np.abs(b))
    return out


def chain64(p, S, tol_S, P, tol_P):
    """g_rot [4] and its tolerance from the sums S [3,3] = sum g x^T and P [4] = sum of the product's transpose in a,
    by the finishing thread's steps (float64 values; the counts are the float32 kernel's)."""
    r, x, y, z = p["u"]
    # gu_k = 2 * sum_m c_m S_m: per term the factor's error (6), its product (1), at most 7 additions, one more product
    # for the doubled ones, the final doubling exact: 16
    C = np.zeros((4, 3, 3))
    C[0] = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    C[1] = [[0, y, z], [y, -2 * x, -r], [z, r, -2 * x]]
    C[2] = [[-2 * y, x, r], [x, 0, z], [-r, z, -2 * y]]
    C[3] = [[-2 * z, -r, x], [r, -2 * z, y], [x, y, 0]]
    gu = 2 * np.einsum("kij,ij->k", C, S)
    tol_gu = 2 * (np.einsum("kij,ij->k", np.abs(C), tol_S) + 16 * U * np.einsum("kij,ij->k", np.abs(C), np.abs(S)))
    # along_u = sum u_k gu_k: the factor's error (6), product (1), three additions: 10
    au = (p["u"] * gu).sum()
    tol_au = (np.abs(p["u"]) * tol_gu).sum() + 10 * U * np.abs(p["u"] * gu).sum()
    # inner = gu_k - u_k along_u: the product carries u's error and its rounding (7); the subtraction rounds once
    inner = gu - p["u"] * au
    tol_inner = tol_gu + np.abs(p["u"]) * tol_au + 7 * U * np.abs(p["u"] * au) + U * (np.abs(gu) + np.abs(p["u"] * au))
    # / n2: n2's error (3) and the division (1); + P_k: one rounding
    gq = inner / p["n2"] + P
    tol_gq = tol_inner / p["n2"] + 4 * U * np.abs(inner / p["n2"]) + tol_P + U * (np.abs(inner / p["n2"]) + np.abs(P))
    # along_q = sum q^_k gq_k: q^'s error (4), product (1), three additions: 8
    aq = (p["q"] * gq).sum()
    tol_aq = (np.abs(p["q"]) * tol_gq).sum() + 8 * U * np.abs(p["q"] * gq).sum()
    # (gq_k - q^_k along_q) / n1: product with q^'s error (5), subtraction (1); n1's error (3) and the division (1)
    last = gq - p["q"] * aq
    tol_last = tol_gq + np.abs(p["q"]) * tol_aq + 5 * U * np.abs(p["q"] * aq) + U * (np.abs(gq) + np.abs(p["q"] * aq))
    return last / p["n1"], tol_last / p["n1"] + 4 * U * np.abs(last / p["n1"])


def chain_matrix(p):
    """L [4,13]: g_rot = L (S.ravel(), P) -- the chain is linear in the sums, so a row's contribution to g_rot is L
    applied to the row's own thirteen numbers."""
    L = np.zeros((4, 13))
    for k in range(13):
        e = np.zeros(13)
        e[k] = 1.0
        L[:, k] = chain64(p, e[:9].reshape(3, 3), np.zeros((3, 3)), e[9:], np.zeros(4))[0]
    return L


def row_contributions(rot, xyz, rotation, g_xyz_out, g_rotation_out):
    """(c_rot [N,4], c_trans [N,3]): the float64 per-row contributions to g_rot / g_trans (their sums over the rows
    are backward64's values)."""
    p = row64(rot)
    g, x = np.asarray(g_xyz_out, np.float64), np.asarray(xyz, np.float64)
    gr, b = np.asarray(g_rotation_out, np.float64), np.asarray(rotation, np.float64)
    V = np.concatenate([np.einsum("ia,ij->iaj", g, x).reshape(len(g), 9), np.einsum("kmn,in,ik->im", H, b, gr)], 1)
    return V @ chain_matrix(p).T, g


def backward64(rot, xyz=None, rotation=None, g_xyz_out=None, g_rotation_out=None, depth=None):
    """dict(g_xyz, tol_g_xyz; g_rotation, tol_g_rotation; g_trans, tol_g_trans [3]; g_rot, tol_g_rot [4]; S, P).  An
    absent upstream gradient counts as zero.  depth: the longest chain of additions of a sum; default the kernel's
    (chain_depth); N - 1 covers ANY order of summation (the reference's matmul backward on the CPU, whose order
    PyTorch leaves open)."""
    p = row64(rot)
    out = {}
    S, tol_S, P, tol_P = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(4), np.zeros(4)
    N = len(g_xyz_out) if g_xyz_out is not None else len(g_rotation_out)
    d = chain_depth(N) if depth is None else depth
    out["g_trans"], out["tol_g_trans"] = np.zeros(3), np.zeros(3)
    if g_xyz_out is not None:
        g = np.asarray(g_xyz_out, np.float64)
        x = np.asarray(xyz, np.float64)
        out["g_xyz"] = g @ p["R"]
        out["tol_g_xyz"] = np.abs(g) @ p["tol_R"] + GXYZ_ROUND * U * (np.abs(g) @ np.abs(p["R"]))
        out["g_trans"], out["tol_g_trans"] = g.sum(0), d * U * np.abs(g).sum(0)
        S, tol_S = g.T @ x, (d + 1) * U * (np.abs(g).T @ np.abs(x))
    if g_rotation_out is not None:
        g = np.asarray(g_rotation_out, np.float64)
        b = np.asarray(rotation, np.float64)
        out["g_rotation"] = np.einsum("kmn,m,ik->in", H, p["q"], g)
        out["tol_g_rotation"] = QMUL_ROUND * U * np.einsum("kmn,m,ik->in", np.abs(H), np.abs(p["q"]), np.abs(g))
        P = np.einsum("kmn,in,ik->m", H, b, g)
        tol_P = (d + 4) * U * np.einsum("kmn,in,ik->m", np.abs(H), np.abs(b), np.abs(g))
    out["g_rot"], out["tol_g_rot"] = chain64(p, S, tol_S, P, tol_P)
    out["S"], out["P"] = S, P
    return out


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


# ---------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy, operation by operation (numpy rounds each float32 operation once)
# ---------------------------------------------------------------------------------------------------------------
F = np.float32


def row32(rot, plant=None):
    """The kernel's pose_row.  plant: a one-line error for the host test ("no_normalize": F.normalize dropped, the
    raw row goes on -- quaternion_to_matrix's own division still mends R, the product is off by |rot|)."""
    w, x, y, z = [F(v) for v in np.asarray(rot, F)]
    n1 = max(np.sqrt(((w * w + x * x) + y * y) + z * z), F(1e-12))
    q = np.array([w, x, y, z], F) if plant == "no_normalize" else np.array([w / n1, x / n1, y / n1, z / n1], F)
    n2 = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    u = np.array([q[0] / n2, q[1] / n2, q[2] / n2, q[3] / n2], F)
    r, qx, qy, qz = u
    one, two = F(1), F(2)
    R = np.array([[one - two * (qy * qy + qz * qz), two * (qx * qy - r * qz), two * (qx * qz + r * qy)],
                  [two * (qx * qy + r * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - r * qx)],
                  [two * (qx * qz - r * qy), two * (qy * qz + r * qx), one - two * (qx * qx + qy * qy)]], F)
    return dict(q=q, u=u, n1=F(n1), n2=F(n2), R=R)


def _qmul32(a, b):
    """quaternion_raw_multiply(a, b), left to right; a [4], b [N,4] (or the other way round), float32."""
    aw, ax, ay, az = [a[..., k] for k in range(4)]
    bw, bx, by, bz = [b[..., k] for k in range(4)]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1).astype(F)


def forward32(rot, trans, xyz=None, rotation=None, plant=None):
    """(xyz' or None, rotation' or None).  plant: "no_normalize" (row32), "normalized_product" (the product
    normalised behind it, compose_one's form)."""
    p = row32(rot, plant)
    R, t = p["R"], np.asarray(trans, F)
    ox = orot = None
    if xyz is not None:
        x = np.asarray(xyz, F)
        ox = np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], 1)
    if rotation is not None:
        orot = _qmul32(p["q"], np.asarray(rotation, F))
        if plant == "normalized_product":
            orot = (orot / np.sqrt((orot * orot).sum(1, keepdims=True))).astype(F)
    return ox, orot


def _tree32(v):
    """The kernel's fixed-order sum of float32 [N]: 256 rows a workgroup, butterfly over the 64 lanes of a wave, the four
    waves in ascending order, then the finishing workgroup's strided loop and tree of halves."""
    nb = blocks(len(v))
    t = np.zeros(nb * BLOCK, F)
    t[:len(v)] = v
    t = t.reshape(nb, 4, 64)
    for d in (32, 16, 8, 4, 2, 1):                                   # butterfly: lane l reads l ^ d
        t = t + t[..., np.arange(64) ^ d]
    w = t[..., 0]
    part = ((F(0) + w[:, 0]) + w[:, 1] + w[:, 2]) + w[:, 3]
    slots = np.zeros(REDUCE_THREADS, F)
    for s in range(0, part.size, REDUCE_THREADS):
        chunk = part[s:s + REDUCE_THREADS]
        slots[:chunk.size] = slots[:chunk.size] + chunk
    n = REDUCE_THREADS // 2
    while n >= 1:
        slots[:n] = slots[:n] + slots[n:2 * n]
        n //= 2
    return slots[0]


def backward32(rot, xyz=None, rotation=None, g_xyz_out=None, g_rotation_out=None, plant=None):
    """dict(g_xyz, g_rotation (None when absent), g_trans [3], g_rot [4]) as the kernels form them.  plant: "R_for_RT"
    (g_xyz = R g), "no_projection" (the first normalisation's projection dropped from g_rot), "trans_from_rotation"
    (g_trans summed from the rotation's upstream gradient)."""
    p = row32(rot)
    R, q, u = p["R"], p["q"], p["u"]
    out = dict(g_xyz=None, g_rotation=None)
    N = len(g_xyz_out) if g_xyz_out is not None else len(g_rotation_out)
    v = np.zeros((16, N), F)
    if g_xyz_out is not None:
        g, x = np.asarray(g_xyz_out, F), np.asarray(xyz, F)
        M = R.T if plant == "R_for_RT" else R
        out["g_xyz"] = np.stack([(M[0, j] * g[:, 0] + M[1, j] * g[:, 1]) + M[2, j] * g[:, 2] for j in range(3)], 1)
        for a in range(3):
            for j in range(3):
                v[3 * a + j] = g[:, a] * x[:, j]
            v[9 + a] = g[:, a]
    if g_rotation_out is not None:
        g, b = np.asarray(g_rotation_out, F), np.asarray(rotation, F)
        gw, gx, gy, gz = [g[:, k] for k in range(4)]
        aw, ax, ay, az = q
        out["g_rotation"] = np.stack([aw * gw + ax * gx + ay * gy + az * gz, -ax * gw + aw * gx + az * gy - ay * gz,
                                      -ay * gw - az * gx + aw * gy + ax * gz, -az * gw + ay * gx - ax * gy + aw * gz], 1)
        bw, bx, by, bz = [b[:, k] for k in range(4)]
        v[12] = bw * gw + bx * gx + by * gy + bz * gz
        v[13] = -bx * gw + bw * gx - bz * gy + by * gz
        v[14] = -by * gw + bz * gx + bw * gy - bx * gz
        v[15] = -bz * gw - by * gx + bx * gy + bw * gz
        if plant == "trans_from_rotation":
            for a in range(3):
                v[9 + a] = g[:, a]
    S = np.array([_tree32(v[k]) for k in range(16)], F)
    out["g_trans"] = S[9:12].copy()
    r, x, y, z = u
    two = F(2)
    gu = np.array([
        two * (((((x * S[7] - x * S[5]) + y * S[2]) - y * S[6]) + z * S[3]) - z * S[1]),
        two * (((((((y * S[1] + y * S[3]) + z * S[2]) + z * S[6]) + r * S[7]) - r * S[5]) - two * (x * S[4])) -
               two * (x * S[8])),
        two * (((((((x * S[1] + x * S[3]) + z * S[5]) + z * S[7]) + r * S[2]) - r * S[6]) - two * (y * S[0])) -
               two * (y * S[8])),
        two * (((((((x * S[2] + x * S[6]) + y * S[5]) + y * S[7]) + r * S[3]) - r * S[1]) - two * (z * S[0])) -
               two * (z * S[4]))], F)
    au = ((r * gu[0] + x * gu[1]) + y * gu[2]) + z * gu[3]
    gq = np.array([(gu[k] - u[k] * au) / p["n2"] + S[12 + k] for k in range(4)], F)
    aq = ((q[0] * gq[0] + q[1] * gq[1]) + q[2] * gq[2]) + q[3] * gq[3]
    if plant == "no_projection":
        aq = F(0)
    out["g_rot"] = np.array([(gq[k] - q[k] * aq) / p["n1"] for k in range(4)], F)
    return out
