"""Float64 truths and error bounds of the LPIPS backward (gaussianrpg_amd/lpips.py ``LPIPS.loss``, csrc/lpips_bwd.hip),
for tests/test_lpips_bwd_host.py, tests/test_gpu_lpips_bwd.py, tools/lpips_bwd_parity.py and
tests/golden/make_golden_lpips_bwd.py.  The builders, the tables and the cases are tests/lpips_truth.py's.

The three leaves are restated in float64 -- convolution backward-data, the pool's gather, the distance's derivative --
and the whole gradient is the chain of those leaves in the order csrc/lpips_bwd.hip enqueues them.

The whole-gradient truth is CONDITIONAL on the forward's decisions.  The ReLU masks (act > 0) and the pool winners
(the first row-major maximum of every window) of the x side are inputs: the float64 forward forces them -- pre * mask,
and a gather at the given index -- and the backward selects by the same masks and scatters to the same winners.  The y
side keeps its own decisions: it enters only as continuous constants.  Without this, one activation whose sign differs
between a float32 forward and the float64 one moves the gradient by about 1e-3 relative; with the decisions forced,
a comparison sees rounding only.  With float64's own decisions the chain equals plain float64 autograd
(test_lpips_bwd_host).

Error bounds of the leaves (u = 2^-24; first order in u)
--------------------------------------------------------
convolution backward-data.  A produced element is a sum of K products w * g, K = the number of enumerated taps:
C_out * k * k at stride 1 (zeros outside the gradient's plane included), C_out * ceil(k / s)^2 at stride s.  As in
lpips_truth (tests/detector_truth.py), any order that sends no product through more than K + 2 roundings -- the
kernel's fma chains over blocks of 32 and the block sums in order, or one fma chain -- gives |d acc| <= (K + 2) u S,
S = sum |w| |g|.  Epilogue: adding the tap's gradient rounds once, u |acc + tap| <= u (|acc| + |tap|); the select
rounds nothing; the division by std_c (std_c a float32 constant, used as such by the truth) rounds once:
(E + u |acc|) / std_c.

pool.  An element is covered by at most 2 x 2 windows: at most 4 additions from zero, then the tap's: each rounds at
most u times a partial sum of magnitude at most T = sum |terms|: E <= 5 u T.  (The first addition, onto 0, is exact; the
slack is kept.)

distance, per pixel, with the features exact (a leaf test feeds float32 features).  r_n = (C / 2 + 2) u bounds the
relative error of nxe = sqrtf(sum x^2) + eps (C fma roundings on a sum of non-negative terms, halved by the root, the
root's rounding and the addition's), r_a = r_n + u that of a_c = x_c / nxe; likewise b_c.
  d_c = a_c - b_c:              |dd_c| <= r_a (|a_c| + |b_c|) + u |d_c|
  q_c = (2 w_c) d_c:            |dq_c| <= 2 |w_c| |dd_c| + u |q_c|                        (2 w_c is exact)
  t1_c = q_c / nxe:             |dt1_c| <= |dq_c| / nxe + (r_n + u) |t1_c|
  dot = sum_c q_c x_c (fma):    |ddot| <= sum_c |dq_c| |x_c| + C u sum_c |q_c x_c|
  coef = dot / ((nxe nxe) nx):  the denominator carries 2 r_n + u, then r_n + u, the division u:
                                |dcoef| <= |ddot| / D + (3 r_n + 3 u) |coef|
  t2_c = x_c coef:              |dt2_c| <= |x_c| |dcoef| + u |t2_c|
  g_c = sc (t1_c - t2_c), sc = grad_pair / HW one rounding, the difference one, the product one:
                                |dg_c| <= |sc| (|dt1_c| + |dt2_c| + u |t1_c - t2_c|) + 2 u |g_c|
The select x_c > 0 rounds nothing.

Acceptance of the whole gradient (against the reference, tests/golden/ref_lpips_bwd.json -- never against the code
under test): per case, the relative L2 distance of the gradient from the conditional truth at the forward's own
decisions is at most MARGIN x the distance the reference's own float32 autograd keeps from the conditional truth at
ITS decisions, and the worst element's distance at most MARGIN x the reference's worst.
"""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_truth as T

U = T.U
MARGIN = T.MARGIN
STD32 = tuple(float(np.float32(v)) for v in T.STD)

# the planted errors the acceptance bound must reject; value: which nets' cases can show it at the whole-net level
VARIANTS = {
    "correlation": ("alex", "vgg"),            # correlation in place of the flipped convolution
    "norm_constant": ("alex", "vgg"),          # the norm treated as a constant
    "missing_std": ("alex", "vgg"),            # no 1 / std in the image's gradient
    "missing_hw": ("alex", "vgg"),             # no 1 / (H_l W_l)
    "tap_wrong_layer": ("alex", "vgg"),        # a tap's gradient added one convolution off
}
# planted at a leaf (no whole-net case can show them: no CASE's size leaves a row under no window -- h % 4 == 2 -- or
# holds two equal positive maxima in one window, or a NaN): conv_bwd's "stride_remainder" (rows / columns under no
# window given a neighbour's gradient) and "relu_product" (the ReLU as a product), pool_bwd's "pool_last_max"
MOVED_TAP = {"alex": (3, 4), "vgg": (1, 0)}    # tap_wrong_layer: the tap of convolution [0] is added at convolution [1]


def t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(dtype)


# ---- decisions ----

def first_max_index(act, k):
    """[B, C, ho, wo] int64: per window of MaxPool2d(k, 2), the flat index (y * W + x) of the FIRST maximum in
    row-major order -- F.max_pool2d's winner (torch.argmax returns the first of equal maxima)."""
    B, C, H, W = act.shape
    win = act.unfold(2, k, 2).unfold(3, k, 2)                      # [B, C, ho, wo, k, k]
    ho, wo = win.shape[2], win.shape[3]
    arg = win.reshape(B, C, ho, wo, k * k).argmax(-1)
    dy, dx = arg // k, arg % k
    oy = torch.arange(ho).view(1, 1, ho, 1)
    ox = torch.arange(wo).view(1, 1, 1, wo)
    return (2 * oy + dy) * W + 2 * ox + dx


def last_max_index(act, k):
    """the planted error: the LAST maximum of a window"""
    B, C, H, W = act.shape
    win = act.unfold(2, k, 2).unfold(3, k, 2)
    ho, wo = win.shape[2], win.shape[3]
    arg = k * k - 1 - win.reshape(B, C, ho, wo, k * k).flip(-1).argmax(-1)
    dy, dx = arg // k, arg % k
    oy = torch.arange(ho).view(1, 1, ho, 1)
    ox = torch.arange(wo).view(1, 1, 1, wo)
    return (2 * oy + dy) * W + 2 * ox + dx


def plan(net):
    """The launches' layers up to the fifth tap: dicts with kind, the geometry, ``conv`` / ``pool`` (its number) and
    ``tap`` (or None), as csrc/lpips.hip's net_layers."""
    out, conv, pool = [], 0, 0
    for i, L in enumerate(T.LAYERS[net][:T.TARGETS[net][-1]], 1):
        if L[0] == "conv":
            out.append(dict(kind="conv", index=i - 1, c_in=L[1], c_out=L[2], k=L[3], stride=L[4], pad=L[5], conv=conv, tap=None))
            conv += 1
        elif L[0] == "pool":
            out.append(dict(kind="pool", k=L[1], pool=pool, tap=None))
            pool += 1
        elif i in T.TARGETS[net]:
            out[-1]["tap"] = T.TARGETS[net].index(i)
    return out


def decisions_of(net, acts):
    """(masks, winners) of kept post-ReLU activations [one per convolution]: act > 0, and every pool's first maxima."""
    acts = [torch.as_tensor(a) for a in acts]
    masks = [a > 0 for a in acts]
    winners, last = [], None
    for l in plan(net):
        if l["kind"] == "conv":
            last = acts[l["conv"]]
        else:
            winners.append(first_max_index(last, l["k"]))
    return masks, winners


# ---- the leaves ----

def conv_bwd(gout, w, k, s, p, hw_in, mask=None, tap=None, std=False, variant=None, dtype=torch.float64):
    """(grad_in, bound): convolution backward-data of gout [B, C_out, ho, wo] with OIHW weights, then the epilogue:
    ``mask`` (the ReLU output's act > 0) selects, ``tap`` is added before it, ``std`` divides channel c by std_c."""
    gout, w = t(gout, dtype), t(w, dtype)
    opad = (hw_in[0] - ((gout.shape[2] - 1) * s - 2 * p + k), hw_in[1] - ((gout.shape[3] - 1) * s - 2 * p + k))
    wt = w.flip(2, 3) if variant == "correlation" else w
    acc = F.conv_transpose2d(gout, wt, stride=s, padding=p, output_padding=opad)
    S = F.conv_transpose2d(gout.abs(), w.abs(), stride=s, padding=p, output_padding=opad)
    if variant == "stride_remainder" and s > 1:
        cov_h = min(hw_in[0], (gout.shape[2] - 1) * s + k - p)      # rows [0, cov_h) lie under a window
        cov_w = min(hw_in[1], (gout.shape[3] - 1) * s + k - p)
        acc = acc.clone()
        if cov_h < hw_in[0]:
            acc[:, :, cov_h:] = acc[:, :, cov_h - 1:cov_h]
        if cov_w < hw_in[1]:
            acc[:, :, :, cov_w:] = acc[:, :, :, cov_w - 1:cov_w]
    K = w.shape[0] * (-(-k // s)) ** 2
    E = (K + 2) * U * S
    out = acc
    if tap is not None:
        tap = t(tap, dtype)
        out = acc + tap
        E = E + U * (acc.abs() + tap.abs())
    if mask is not None:
        if variant == "relu_product":
            out = out * t(mask, dtype)
        else:
            out = torch.where(torch.as_tensor(mask), out, torch.zeros_like(out))
            E = torch.where(torch.as_tensor(mask), E, torch.zeros_like(E))
    if std and variant != "missing_std":
        sd = t(np.asarray(T.STD, np.float32), dtype).view(1, 3, 1, 1)
        E = (E + U * acc.abs()) / sd
        out = out / sd
    return out, E.to(torch.float64)


def pool_bwd(act, gout, k, mask=None, tap=None, winners=None, variant=None, dtype=torch.float64):
    """(grad_in, bound): MaxPool2d(k, 2) backward onto its input ``act`` (a ReLU output), every window's gradient to
    its winner (given, or the first maximum of ``act``), then the tap's gradient and the select."""
    act, gout = t(act, dtype), t(gout, dtype)
    if winners is None:
        winners = last_max_index(act, k) if variant == "pool_last_max" else first_max_index(act, k)
    B, C, H, W = act.shape
    flat = torch.zeros(B, C, H * W, dtype=dtype)
    flat.scatter_add_(2, winners.reshape(B, C, -1), gout.reshape(B, C, -1))
    mag = torch.zeros(B, C, H * W, dtype=dtype)
    mag.scatter_add_(2, winners.reshape(B, C, -1), gout.abs().reshape(B, C, -1))
    out, mag = flat.view(B, C, H, W), mag.view(B, C, H, W)
    if tap is not None:
        out, mag = out + t(tap, dtype), mag + t(tap, dtype).abs()
    if mask is None:
        mask = act > 0
    mask = torch.as_tensor(mask)
    out = torch.where(mask, out, torch.zeros_like(out))
    return out, torch.where(mask, 5 * U * mag, torch.zeros_like(mag)).to(torch.float64)


def distance_bwd(fx, fy, w, grad_pairs, mask=None, variant=None, dtype=torch.float64):
    """(grad [P, C, H, W], bound): the gradient of sum_p grad_pairs[p] * mean_pixels(s) to fx, 0 where the select
    (``mask``, or fx > 0: a tap is a ReLU's output) is off.  The norm's derivative at an all-zero vector is 0."""
    fx, fy, w = t(fx, dtype), t(fy, dtype), t(w, dtype).reshape(1, -1, 1, 1)
    gp = t(grad_pairs, dtype).reshape(-1, 1, 1, 1)
    C, hw = fx.shape[1], fx.shape[2] * fx.shape[3]
    eps = torch.tensor(T.EPS, dtype=dtype)
    nx = torch.sqrt((fx * fx).sum(1, keepdim=True))
    nxe, nye = nx + eps, torch.sqrt((fy * fy).sum(1, keepdim=True)) + eps
    a, b = fx / nxe, fy / nye
    d = a - b
    q = (2 * w) * d
    t1 = q / nxe
    dot = (q * fx).sum(1, keepdim=True)
    D = (nxe * nxe) * nx
    coef = torch.where(nx > 0, dot / torch.where(nx > 0, D, torch.ones_like(D)), torch.zeros_like(dot))
    if variant == "norm_constant":
        coef = torch.zeros_like(coef)
    t2 = fx * coef
    sc = gp if variant == "missing_hw" else gp / hw
    g = sc * (t1 - t2)
    # the bound of the module's docstring
    r_n = (C / 2 + 2) * U
    r_a = r_n + U
    dd = r_a * (a.abs() + b.abs()) + U * d.abs()
    dq = 2 * w.abs() * dd + U * q.abs()
    dt1 = dq / nxe + (r_n + U) * t1.abs()
    ddot = (dq * fx.abs()).sum(1, keepdim=True) + C * U * (q * fx).abs().sum(1, keepdim=True)
    dcoef = torch.where(nx > 0, ddot / torch.where(nx > 0, D, torch.ones_like(D)), torch.zeros_like(dot)) + (3 * r_n + 3 * U) * coef.abs()
    dt2 = fx.abs() * dcoef + U * t2.abs()
    E = sc.abs() * (dt1 + dt2 + U * (t1 - t2).abs()) + 2 * U * g.abs()
    if mask is None:
        mask = fx > 0
    mask = torch.as_tensor(mask)
    return torch.where(mask, g, torch.zeros_like(g)), torch.where(mask, E, torch.zeros_like(E)).to(torch.float64)


# ---- the whole gradient ----

def forward64(net, features, x, masks=None, winners=None):
    """The float64 forward with forced decisions (None: its own).  Returns dict(acts [post-ReLU, one per convolution],
    masks, winners, taps)."""
    h = T.zscore64(x)
    acts, used_m, used_w, taps = [], [], [], []
    for l in plan(net):
        if l["kind"] == "conv":
            pre = F.conv2d(h, T.t64(features["%d.weight" % l["index"]]), T.t64(features["%d.bias" % l["index"]]),
                           stride=l["stride"], padding=l["pad"])
            m = torch.as_tensor(masks[l["conv"]]) if masks is not None else pre > 0
            h = pre * m
            acts.append(h)
            used_m.append(m)
        else:
            idx = winners[l["pool"]] if winners is not None else first_max_index(h, l["k"])
            B, C = h.shape[:2]
            h = h.flatten(2).gather(2, idx.reshape(B, C, -1)).view(B, C, idx.shape[2], idx.shape[3])
            used_w.append(idx)
        if l["tap"] is not None:
            taps.append(h)
    return dict(acts=acts, masks=used_m, winners=used_w, taps=taps)


def grad64(net, features, lin, x, y, grad_pairs=None, masks=None, winners=None, variant=None):
    """d sum_p grad_pairs[p] * value_p / d x [P, 3, H, W] in float64: the chain of the leaves in the order of
    csrc/lpips_bwd.hip, at the x side's decisions ``masks`` / ``winners`` (None: float64's own).  variant: one planted
    error (VARIANTS), None for the truth."""
    P = x.shape[0]
    gp = np.ones(P) if grad_pairs is None else grad_pairs
    fx, fy = forward64(net, features, x, masks, winners), forward64(net, features, y)
    L = plan(net)
    conv_layer = {l["conv"]: l for l in L if l["kind"] == "conv"}
    lin_of = lambda tp: lin["lin%d.model.1.weight" % tp].reshape(-1)
    moved = MOVED_TAP[net] if variant == "tap_wrong_layer" else (None, None)
    dvar = variant if variant in ("norm_constant", "missing_hw") else None

    def tapgrad(conv, mask_conv=None):
        tp = conv_layer[conv]["tap"]
        m = fx["masks"][conv if mask_conv is None else mask_conv]
        return distance_bwd(fx["taps"][tp], fy["taps"][tp], lin_of(tp), gp, mask=m, variant=dvar)[0]

    def tap_on(conv):   # the tap gradient added where a produced gradient lands on convolution `conv`'s output
        out = None
        if conv_layer[conv]["tap"] is not None and conv != moved[0]:
            out = tapgrad(conv)
        if conv == moved[1]:
            extra = tapgrad(moved[0], mask_conv=conv)
            out = extra if out is None else out + extra
        return out

    g = tap_on(L[-1]["conv"])
    hw_of = [tuple(x.shape[2:])] + [tuple(a.shape[2:]) for a in fx["acts"]]
    for i in range(len(L) - 1, -1, -1):
        l = L[i]
        prev = L[i - 1] if i > 0 else None
        on_relu = prev is not None and prev["kind"] == "conv"
        mask = fx["masks"][prev["conv"]] if on_relu else None
        tap = tap_on(prev["conv"]) if on_relu else None
        if l["kind"] == "pool":
            g = pool_bwd(fx["acts"][prev["conv"]], g, l["k"], mask=mask, tap=tap, winners=fx["winners"][l["pool"]])[0]
        else:
            hw_in = tuple(x.shape[2:]) if i == 0 else (tuple(fx["acts"][prev["conv"]].shape[2:]) if on_relu else
                                                        tuple(fx["winners"][prev["pool"]].shape[2:]))
            g = conv_bwd(g, features["%d.weight" % l["index"]], l["k"], l["stride"], l["pad"], hw_in, mask=mask, tap=tap,
                         std=i == 0, variant=variant if variant in ("correlation", "missing_std") else None)[0]
    return g


def autograd64(net, features, lin, x, y, grad_pairs=None):
    """The same gradient by plain float64 autograd over tests/lpips_truth.py's forward: no forced decision."""
    xv = T.t64(x).clone().requires_grad_(True)
    gp = T.t64(np.ones(x.shape[0]) if grad_pairs is None else grad_pairs)
    fx, fy = T.features64(net, features, xv), T.features64(net, features, y)
    total = 0
    for l, (a, b) in enumerate(zip(fx, fy)):
        w = T.t64(lin["lin%d.model.1.weight" % l]).reshape(1, -1, 1, 1)
        s = (w * (T.normalize64(a) - T.normalize64(b)) ** 2).sum(1)
        total = total + (s.mean((1, 2)) * gp).sum()
    return torch.autograd.grad(total, xv)[0]


def restatement32(net, features, lin, x, y):
    """A plain CPU torch float32 restatement with autograd: (gradient of the summed values to x, its post-ReLU
    activations).  Not the reference's modules; for reproducing the order of magnitude of the recorded figures."""
    xv = torch.as_tensor(x).clone().requires_grad_(True)
    mean = torch.tensor(T.MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(T.STD, dtype=torch.float32).view(1, 3, 1, 1)

    def feats(img, keep):
        h, taps = (img - mean) / std, []
        for l in plan(net):
            if l["kind"] == "conv":
                h = F.relu(F.conv2d(h, features["%d.weight" % l["index"]], features["%d.bias" % l["index"]],
                                    stride=l["stride"], padding=l["pad"]))
                if keep is not None:
                    keep.append(h.detach().clone())
            else:
                h = F.max_pool2d(h, l["k"], 2)
            if l["tap"] is not None:
                taps.append(h)
        return taps

    acts = []
    fx = feats(xv, acts)
    with torch.no_grad():
        fy = feats(torch.as_tensor(y), None)
    total = 0
    norm = lambda f: f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)
    for l, (a, b) in enumerate(zip(fx, fy)):
        total = total + (lin["lin%d.model.1.weight" % l] * (norm(a) - norm(b)) ** 2).sum(1, keepdim=True).mean((2, 3)).sum()
    return torch.autograd.grad(total, xv)[0], acts


# ---- acceptance ----

def figures(got, truth):
    """(relative L2 distance, worst element's distance) of a gradient from the truth"""
    got, truth = T.t64(got), T.t64(truth)
    d = got - truth
    return float(torch.linalg.norm(d.reshape(-1)) / torch.linalg.norm(truth.reshape(-1))), float(d.abs().max())


def acceptance(golden_case, got, truth):
    """{"rel_l2", "worst"}: each figure over the reference's recorded one; accepted iff both <= MARGIN (a NaN is not)."""
    rel, worst = figures(got, truth)
    return dict(rel_l2=rel / golden_case["rel_l2"], worst=worst / golden_case["worst"])


def within(acc) -> bool:
    return bool(acc["rel_l2"] <= MARGIN and acc["worst"] <= MARGIN)
