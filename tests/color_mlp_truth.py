"""Float64 truth of the use_mlp colour correction (csrc/color_mlp.hip: camera pose -> the two 3x4 matrices, the
regulariser and the gradients of the sixteen parameter tensors), its derived bounds, the kernel's arithmetic restated
in float32 numpy, and the input builders, for tests/test_color_mlp_host.py, tests/test_gpu_color_mlp.py and
tests/golden/make_golden_color_mlp.py.

  c2w = ego_pose @ extrinsic;  q = matrix_to_quaternion(c2w[:3,:3]) (first largest q_abs, no sign standardisation);
  r = quaternion_to_axis_angle(q);  x = [r, c2w[:3,3]]
  h1 = relu(W1 x + b1), h2 = relu(W2 h1 + b2), h3 = relu(W3 h2 + b3), A = view(W4 h3 + b4, 3, 4) + eye(4)[:3]
  reg = mean(|A - I| + |A_sky - I|)

The truth evaluates the same formulas, branch for branch, in float64 on the float32 inputs widened.

Bounds (u = 2^-24).
  x        A closed bound through atan2 is awkward; the project's other yardstick is used (profiles/tracks_parity.json):
           a float32 evaluation may lie at most 4 times as far from the truth as the larger of the reference's own
           recorded float32 distance and 8 ulps of the largest component (distances: max over the six components).
           That yardstick, tol_x, is far too coarse to carry through three layers (8 ulps of a translation of 300 m
           is 2.4e-4), so the layers' input error e_0 is pose_bound: a first-order running error bound of the float32
           evaluation, step by step, per component; x is held against it as well.
  layers   pre_l = W_l h_{l-1} + b_l with k inputs, accumulated in any order, fused or not: every term passes at most
           k + 1 roundings (its product, at most k additions), so to first order
             e_l = |W_l| e_{l-1} + (k + 2) u (|W_l| |h_{l-1}| + |b_l|)            (relu is 1-Lipschitz: same e_l for h_l)
           and e_A = e_4 + u |A| for the "+ I".
  masks    a unit whose float64 pre-activation exceeds its own e_l in magnitude has the same relu mask in float32;
           gradient cases must have |pre| > 4 e_l on EVERY unit (mask_margin), else the gradient is discontinuous
           inside the rounding error and no bound holds.
  reg      24 terms |A - I|, each within e_A + u |A - I|, 23 additions and a division:
             e_reg = mean-sum of e_A over both matrices + 26 u reg
  backward (masks fixed)  d4 = grad_affine + grad_reg sign(A - I) / 12: exact without the regulariser, else two
           roundings: dd_4 = 2 u |d4| (and the sign must be stable: |A64 - I| > 2 e_A, sign_margin).  Going down,
             gW_l = sum_t d_l (x) h_{l-1}:  sum_t (dd_l (x) |h| + |d_l| (x) e_{l-1}) + (T + 1) u sum_t |d_l| (x) |h|
             gb_l = sum_t d_l:              sum_t dd_l + T u sum_t |d_l|
             dh   = W_l^T d_l (n outputs):  |W_l|^T dd_l + (n + 1) u |W_l|^T |d_l|,   masked like d_{l-1}
"""
import collections
import functools
import hashlib

import numpy as np

U = 2.0 ** -24
EYE = np.eye(4)[:3].reshape(12)
SHAPES = [(64, 6), (64, 64), (64, 64), (12, 64)]
NETS = ("affine_trans", "affine_trans_sky")
KEYS = tuple("%s.%d.%s" % (net, layer, kind) for net in NETS for layer in (0, 2, 4, 6) for kind in ("weight", "bias"))

# weight seed of the cases; every pose below satisfies mask_margin and sign_margin with it (the host test asserts it)
SEED = 7


# ---------------------------------------------------------------------------------------------------------------
# input builders (legacy numpy RandomState: stable across versions)
# ---------------------------------------------------------------------------------------------------------------
def build_params(seed=SEED, zero_last=False):
    """The sixteen tensors under the state-dict keys, float32: nn.Linear's default initialisation restated --
    weight and bias uniform in +-1/sqrt(fan_in) -- with a NON-zero last layer unless ``zero_last`` (a fresh module)."""
    rng = np.random.RandomState(4000 + seed)
    out = collections.OrderedDict()
    for net in NETS:
        for layer, (o, i) in zip((0, 2, 4, 6), SHAPES):
            b = 1.0 / np.sqrt(i)
            w, bias = rng.uniform(-b, b, (o, i)), rng.uniform(-b, b, (o,))
            if zero_last and layer == 6:
                w, bias = w * 0.0, bias * 0.0
            out["%s.%d.weight" % (net, layer)] = w.astype(np.float32)
            out["%s.%d.bias" % (net, layer)] = bias.astype(np.float32)
    return out


def _axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _quat(w, x, y, z):
    q = np.array([w, x, y, z], np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _mat(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.astype(np.float32)


# the extrinsic every "shared_*" pose uses: a camera looking along the ego's x axis, slightly pitched
_CAMERA = _axis_angle((0.1, 0.2, 1.0), 0.03) @ np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])

# name -> (how, rotation of c2w).  "exact": ego = [R | t], extrinsic = [I | t2], so c2w's rotation block is R to the
# bit (ties stay ties).  "split": ego = [Ra | t], extrinsic = [Ra^T R | t2], both generic.
POSES = collections.OrderedDict([
    ("identity", ("exact", np.eye(3))),                                        # 1: result exactly zero
    ("small_2.5e-7", ("exact", _axis_angle((1, -2, 2), 2.5e-7))),              # 2: small-angle divisor
    ("above_4e-6", ("exact", _axis_angle((2, 1, -2), 4e-6))),                  # 3: the other divisor
    ("dominant_r", ("split", _quat(0.80, 0.30, -0.40, 0.33))),                 # 4-7: the four candidate rows
    ("dominant_i", ("split", _quat(0.30, 0.80, 0.33, -0.40))),
    ("dominant_j", ("split", _quat(-0.40, 0.33, 0.80, 0.30))),
    ("dominant_k", ("split", _quat(0.33, -0.40, 0.30, -0.80))),
    ("tie_all_120", ("exact", np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]))),      # 8: all four tie; every row
    #   of this matrix gives (.5,.5,.5,.5), so a wrong pick cannot show here -- it shows on the inverse rotation:
    ("tie_all_m120", ("exact", np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]))),     #    r row: (.5,-.5,-.5,-.5)
    ("tie_ij_180", ("exact", np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]]))),      # 9: i/j tie, rows equal again;
    ("tie_ij_180_opposed", ("exact", np.array([[0.0, -1, 0], [-1, 0, 0], [0, 0, -1]]))),   # about (1,-1,0): opposite
    ("half_turn_x", ("exact", np.diag([1.0, -1.0, -1.0]))),                    # 10: q_w = 0, angle pi
    ("negative_real", ("exact", _axis_angle((1, 0, 0), np.deg2rad(-160.0)))),  # 11: real part < 0, norm > pi
] + [("shared_%d" % i, ("shared", None)) for i in range(5)])                   # 12: one extrinsic for all


def build_pose(name):
    """(ego_pose [4,4], extrinsic [4,4]) float32; translations up to a few hundred metres."""
    how, R = POSES[name]
    rng = np.random.RandomState(5000 + list(POSES).index(name))
    t, t2 = rng.uniform(-300.0, 300.0, 3), rng.uniform(-2.0, 2.0, 3)
    if how == "exact":
        return _mat(R, t), _mat(np.eye(3), t2)
    if how == "split":
        Ra = _quat(*rng.normal(size=4))
        return _mat(Ra, t), _mat(Ra.T @ R, t2)
    return _mat(_quat(*rng.normal(size=4)), t), _mat(_CAMERA, (1.5, 0.0, 2.1))


# name -> (pose names, extrinsic shared as [1,4,4])
BATCHES = collections.OrderedDict([(n, ([n], False)) for n in POSES] + [
    ("T2_shared", (["shared_0", "shared_1"], True)),
    ("T5_shared", (["shared_%d" % i for i in range(5)], True)),
    ("T5_mixed", (["negative_real", "tie_ij_180_opposed", "small_2.5e-7", "dominant_k", "half_turn_x"], False)),
])


def build_batch(name):
    """(ego_pose [T,4,4], extrinsic [T,4,4] or [1,4,4])."""
    names, shared = BATCHES[name]
    poses = [build_pose(n) for n in names]
    ego, ext = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    if shared:
        assert all(np.array_equal(e, ext[0]) for e in ext)
        ext = ext[:1]
    return ego, ext


def build_grad_affine(T, seed=0):
    return np.random.RandomState(6000 + seed).normal(0.0, 1.0, (T, 2, 3, 4)).astype(np.float32)


def build_grad_reg(T, seed=0):
    return np.random.RandomState(7000 + seed).normal(0.0, 1.0, (T,)).astype(np.float32)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def layers(params, net):
    return [(params["%s.%d.weight" % (net, l)], params["%s.%d.bias" % (net, l)]) for l in (0, 2, 4, 6)]


# ---------------------------------------------------------------------------------------------------------------
# the pose vector: one routine for the float64 truth and the float32 restatement (dtype decides), with the planted
# errors of tests/test_color_mlp_host.py as switches
# ---------------------------------------------------------------------------------------------------------------
def pose_vector(ego, ext, dtype, standardise=False, last_on_tie=False, drop_translation=False, small_below=1e-6):
    f = dtype
    e, m = np.asarray(ego, f), np.asarray(ext, f)
    c = np.zeros((3, 4), f)
    for i in range(3):
        for j in range(4):
            a = f(e[i, 0] * m[0, j])
            for k in (1, 2, 3):
                a = f(a + f(e[i, k] * m[k, j]))
            c[i, j] = a
    (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = c[0, :3], c[1, :3], c[2, :3]
    one = f(1.0)
    s = [one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22]
    q_abs = [np.sqrt(v) if v > 0 else f(0.0) for v in s]
    best = 0
    for i in (1, 2, 3):
        if q_abs[i] >= q_abs[best] if last_on_tie else q_abs[i] > q_abs[best]:
            best = i
    rows = [[q_abs[0] * q_abs[0], m21 - m12, m02 - m20, m10 - m01],
            [m21 - m12, q_abs[1] * q_abs[1], m10 + m01, m02 + m20],
            [m02 - m20, m10 + m01, q_abs[2] * q_abs[2], m12 + m21],
            [m10 - m01, m20 + m02, m21 + m12, q_abs[3] * q_abs[3]]]
    den = f(2.0) * max(q_abs[best], f(0.1))
    q = [f(v / den) for v in rows[best]]
    if standardise and q[0] < 0:
        q = [-v for v in q]
    n = np.sqrt(f(f(q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]))
    half = np.arctan2(n, q[0])
    angle = f(2.0) * half
    if abs(angle) < f(small_below):
        div = f(0.5) - f(angle * angle) / f(48.0)
    else:
        div = np.sin(half) / angle
    x = np.array([q[1] / div, q[2] / div, q[3] / div, c[0, 3], c[1, 3], c[2, 3]], f)
    if drop_translation:
        x[3:] = 0
    return x


def pose_bound(ego, ext):
    """e_x [6]: a first-order running error bound of a float32 evaluation of pose_vector against the float64 one, on
    the branch the float64 one takes (the cases keep both evaluations on one branch: margins or exact ties).  Every
    rounded operation adds u |result|; a sum of n terms adds n u sum |terms|; atan2f may be off by 8 u |result| and
    sinf by 4 u (the device library documents a few ulps for both)."""
    e, m = np.abs(np.asarray(ego, np.float64)), np.abs(np.asarray(ext, np.float64))
    c = np.asarray(ego, np.float64)[:3] @ np.asarray(ext, np.float64)
    ec = 4.0 * U * (e[:3] @ m)                                           # four products, three additions
    d, ed = np.diag(c[:, :3]), np.diag(ec[:, :3])
    signs = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    s = 1.0 + signs @ d
    es = ed.sum() + 3.0 * U * (1.0 + np.abs(d).sum())
    q_abs = np.sqrt(np.maximum(s, 0.0))
    best = int(np.argmax(q_abs))                                         # the first largest
    a = q_abs[best]
    ea = es / (2.0 * a) + U * a                                          # s[best] >= 1: the four sum to 4
    pair = {(0, 1): (2, 1, 1, 2, -1), (0, 2): (0, 2, 2, 0, -1), (0, 3): (1, 0, 0, 1, -1),
            (1, 2): (1, 0, 0, 1, 1), (1, 3): (0, 2, 2, 0, 1), (2, 3): (1, 2, 2, 1, 1)}
    row, erow = np.zeros(4), np.zeros(4)
    for k in range(4):
        if k == best:
            row[k], erow[k] = a * a, 2.0 * a * ea + U * a * a
        else:
            i0, j0, i1, j1, sg = pair[(min(k, best), max(k, best))]
            row[k] = c[i0, j0] + sg * c[i1, j1]
            erow[k] = ec[i0, j0] + ec[i1, j1] + U * (abs(c[i0, j0]) + abs(c[i1, j1]))
    den, eden = 2.0 * max(a, 0.1), 2.0 * ea
    q = row / den
    eq = erow / den + np.abs(q) * eden / den + U * np.abs(q)
    n = np.sqrt((q[1:] ** 2).sum())
    en = np.sqrt((eq[1:] ** 2).sum()) + 3.0 * U * n                      # the norm is 1-Lipschitz; its own roundings
    half = np.arctan2(n, q[0])
    ehalf = (en * abs(q[0]) + eq[0] * n) / (n * n + q[0] * q[0]) + 8.0 * U * abs(half)
    angle, eangle = 2.0 * half, 2.0 * ehalf
    if abs(angle) < 1e-6:
        div = 0.5 - angle * angle / 48.0
        ediv = 2.0 * abs(angle) * eangle / 48.0 + 3.0 * U * 0.5
    else:
        div = np.sin(half) / angle
        ediv = (abs(np.cos(half)) * ehalf + 4.0 * U * abs(np.sin(half))) / abs(angle) \
            + abs(div) * eangle / abs(angle) + U * abs(div)
    r = q[1:] / div
    er = eq[1:] / abs(div) + np.abs(r) * ediv / abs(div) + U * np.abs(r)
    return np.concatenate([er, ec[:, 3]])


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def tol_x(x64, ref_distance=0.0):
    """The 4x yardstick of the module docstring."""
    return 4.0 * max(float(ref_distance), 8.0 * ulp32(np.abs(x64).max()))


# ---------------------------------------------------------------------------------------------------------------
# float64 truth with its bounds
# ---------------------------------------------------------------------------------------------------------------
def forward64(params, x64, e_x):
    """One camera.  dict per quantity, each [2, ...] over the networks: pre (list of 4), e (list of 4), h (list of 4
    inputs h_0 = x .. h_3), A, e_A [2,12]; reg, e_reg."""
    out = dict(pre=[], e=[], h=[], A=[], e_A=[])
    for net in NETS:
        h, e = np.asarray(x64, np.float64), np.asarray(e_x, np.float64)
        pres, es, hs = [], [], []
        for l, (W, b) in enumerate(layers(params, net)):
            W, b = W.astype(np.float64), b.astype(np.float64)
            hs.append(h)
            pre = W @ h + b
            e = np.abs(W) @ e + (W.shape[1] + 2) * U * (np.abs(W) @ np.abs(h) + np.abs(b))
            pres.append(pre)
            es.append(e)
            h = np.maximum(pre, 0.0)
        A = pres[3] + EYE
        out["pre"].append(pres), out["e"].append(es), out["h"].append(hs)
        out["A"].append(A), out["e_A"].append(es[3] + U * np.abs(A))
    out["A"], out["e_A"] = np.stack(out["A"]), np.stack(out["e_A"])
    dev = np.abs(out["A"] - EYE)
    out["reg"] = dev.sum() / 12.0
    out["e_reg"] = out["e_A"].sum() / 12.0 + 26.0 * U * out["reg"]
    return out


def mask_margin(fw):
    """min over every relu unit of both networks of |pre| / e: gradient cases need > 4."""
    return min(float((np.abs(fw["pre"][n][l]) / fw["e"][n][l]).min()) for n in range(2) for l in range(3))


def sign_margin(fw):
    """min over the 24 outputs of |A - I| / e_A: cases with grad_reg need > 2."""
    return float((np.abs(fw["A"] - EYE) / fw["e_A"]).min())


def backward64(params, fws, grad_affine=None, grad_reg=None):
    """fws: forward64 of every camera of the batch.  ({key: gradient}, {key: tolerance})."""
    T = len(fws)
    grads, tols = {}, {}
    for n, net in enumerate(NETS):
        lay = [(W.astype(np.float64), b) for W, b in layers(params, net)]
        gW = [np.zeros(s) for s in SHAPES]
        tW = [np.zeros(s) for s in SHAPES]
        aW = [np.zeros(s) for s in SHAPES]
        gb, tb, ab = ([np.zeros(s[0]) for s in SHAPES] for _ in range(3))
        for t, fw in enumerate(fws):
            d = np.zeros(12) if grad_affine is None else np.asarray(grad_affine[t, n], np.float64).reshape(12)
            dd = np.zeros(12)
            if grad_reg is not None:
                d = d + float(grad_reg[t]) * np.sign(fw["A"][n] - EYE) / 12.0
                dd = 2.0 * U * np.abs(d)
            for l in (3, 2, 1, 0):
                W = lay[l][0]
                h = fw["h"][n][l]
                e_h = fw["e"][n][l - 1] if l else fw["e_x"]
                gW[l] += np.outer(d, h)
                tW[l] += np.outer(dd, np.abs(h)) + np.outer(np.abs(d), e_h)
                aW[l] += np.outer(np.abs(d), np.abs(h))
                gb[l] += d
                tb[l] += dd
                ab[l] += np.abs(d)
                if l:
                    mask = fw["pre"][n][l - 1] > 0
                    dd = (np.abs(W).T @ dd + (W.shape[0] + 1) * U * (np.abs(W).T @ np.abs(d))) * mask
                    d = (W.T @ d) * mask
        for l, layer in enumerate((0, 2, 4, 6)):
            grads["%s.%d.weight" % (net, layer)] = gW[l]
            tols["%s.%d.weight" % (net, layer)] = tW[l] + (T + 1) * U * aW[l]
            grads["%s.%d.bias" % (net, layer)] = gb[l]
            tols["%s.%d.bias" % (net, layer)] = tb[l] + T * U * ab[l]
    return grads, tols


@functools.lru_cache(maxsize=None)
def truth(batch, seed=SEED, zero_last=False, with_reg=True):
    """The float64 truth of one batch with the named upstream gradients; computed once -- treat as read-only."""
    params = build_params(seed, zero_last)
    ego, ext = build_batch(batch)
    T = ego.shape[0]
    ga, gr = build_grad_affine(T, seed=T), (build_grad_reg(T, seed=T) if with_reg else None)
    fws = []
    for t in range(T):
        m = ext[t if ext.shape[0] > 1 else 0]
        x64, e_x = pose_vector(ego[t], m, np.float64), pose_bound(ego[t], m)
        fw = forward64(params, x64, e_x)
        fw["x"], fw["e_x"] = x64, e_x
        fws.append(fw)
    grads, tols = backward64(params, fws, ga, gr)
    return dict(params=params, ego=ego, ext=ext, grad_affine=ga, grad_reg=gr, fws=fws, grads=grads, tols=tols)


def ratio(got, want, tol):
    """worst |got - want| / tol; a zero tolerance asks for equality; a non-finite value is infinitely wrong."""
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    pos = tol > 0
    if (err[~pos] != 0).any():
        return float("inf")
    return float((err[pos] / tol[pos]).max(initial=0.0))


# ---------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic in float32 numpy, operation for operation (color_mlp.hip's header)
# ---------------------------------------------------------------------------------------------------------------
def _dense32(W, b, h):
    acc = b.astype(np.float32).copy()
    for k in range(W.shape[1]):
        acc = acc + W[:, k] * np.float32(h[k])          # a rounded multiply, a rounded add, k ascending
    return acc


def forward32(params, x, swap=False, no_identity=False, transpose_last=False):
    """x: float32 [6] (the restated pose vector, or the kernel's own x output).  (A [2,12], hidden [2,3,64], reg)."""
    A, hidden = [], []
    eye = np.zeros(12, np.float32) if no_identity else EYE.astype(np.float32)
    for net in (NETS[::-1] if swap else NETS):
        h = np.asarray(x, np.float32)
        hs = []
        for l, (W, b) in enumerate(layers(params, net)):
            if l == 3 and transpose_last:
                W = np.ascontiguousarray(W.reshape(64, 12).T)      # the buffer read as [in,out]
            pre = _dense32(W, b, h)
            if l < 3:
                h = np.where(pre > 0, pre, np.float32(0.0)).astype(np.float32)
                hs.append(h)
        A.append(pre + eye)
        hidden.append(np.stack(hs))
    A = np.stack(A)
    dev = np.abs(A - EYE.astype(np.float32))
    s = np.float32(0.0)
    for i in range(12):
        s = s + (dev[0, i] + dev[1, i])
    return A, np.stack(hidden), np.float32(s / np.float32(12.0))


def backward32(params, xs, hiddens, affines, grad_affine=None, grad_reg=None, mask_ge=False):
    """xs [T,6], hiddens [T,2,3,64], affines [T,2,12] (the forward's outputs) -> {key: float32 gradient}."""
    T = len(xs)
    out = {}
    eye = EYE.astype(np.float32)
    for n, net in enumerate(NETS):
        lay = layers(params, net)
        gW = [np.zeros(s, np.float32) for s in SHAPES]
        gb = [np.zeros(s[0], np.float32) for s in SHAPES]
        for t in range(T):
            d = np.zeros(12, np.float32) if grad_affine is None else \
                np.asarray(grad_affine[t, n], np.float32).reshape(12).copy()
            if grad_reg is not None:
                sg = np.sign(np.asarray(affines[t][n], np.float32).reshape(12) - eye).astype(np.float32)
                d = d + (np.float32(grad_reg[t]) * sg) / np.float32(12.0)
            hs = [np.asarray(xs[t], np.float32)] + [np.asarray(hiddens[t][n][l], np.float32) for l in range(3)]
            for l in (3, 2, 1, 0):
                gW[l] = gW[l] + np.outer(d, hs[l]).astype(np.float32)
                gb[l] = gb[l] + d
                if l:
                    W = lay[l][0]
                    dh = np.zeros(W.shape[1], np.float32)
                    for o in range(W.shape[0]):
                        dh = dh + W[o] * d[o]
                    keep = hs[l] >= 0 if mask_ge else hs[l] > 0
                    d = np.where(keep, dh, np.float32(0.0)).astype(np.float32)
        for l, layer in enumerate((0, 2, 4, 6)):
            out["%s.%d.weight" % (net, layer)] = gW[l]
            out["%s.%d.bias" % (net, layer)] = gb[l]
    return out
