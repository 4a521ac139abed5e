"""Builders, float64 truths and error bounds of LPIPS (gaussianrpg_amd/lpips.py, csrc/lpips.hip), for
tests/test_lpips_host.py, tests/test_gpu_lpips.py, tools/lpips_parity.py and tests/golden/make_golden_lpips.py.  CPU
torch float64 and numpy; legacy ``numpy.random.RandomState`` (stable).  No weight file exists in the repository: the
backbones are the two tables below with weights from a seed.

Error bounds (u = 2^-24, the unit roundoff of float32; all first order in u)
---------------------------------------------------------------------------
conv + ReLU.  tests/detector_truth.py derives |err_pre| <= (K + 2) u S for any summation order that sends no product
through more than K + 2 roundings, S = |b| + sum_k |w_k x_k|; the kernel's order (fma chains over blocks of 32 k from
zero, the block sums added in order onto the bias) is one.  In the z-scored first layer a gathered value
z = (x - mean) / std carries two roundings, |dz| <= 2u |z|, which every product inherits: (K + 4) u S with S over |z|.
ReLU has slope at most 1 and rounds nothing: the bound passes through unchanged.

distance, per pixel.  Inputs x_c, y_c exact (the leaf test feeds the same float32 features to both sides).
  sx = sum_c x_c^2 as an fma chain: C roundings, each at most u sx (all terms are non-negative) -- at most (C + 1) u sx
  with the slack the issue's wording counts; the root halves a relative error and rounds once; + eps rounds once and
  the division once:  |da_c| <= ((C + 1) / 2 + 1 + 2) u |a_c| <= (C / 2 + 4) u |a_c| =: r |a_c|, likewise b_c.
  t_c = w_c (a_c - b_c)^2 inherits 2 |w_c| |a_c - b_c| (|da_c| + |db_c|) and makes three roundings of its own
  (difference, square, product): |dt_c| <= 2 |w_c| |a_c - b_c| r (|a_c| + |b_c|) + 3u |t_c|.
  s = sum_c t_c in order: C additions, each at most u times a partial sum of magnitude at most T = sum_c |t_c|.
  E_s = sum_c |dt_c| + C u T.
distance, the mean over the pixels: a workgroup owns px = 32 / 16 / 8 pixels (C <= 192 / <= 384 / more), so there are
nblk = ceil(HW / px) slots; the workgroup's butterfly (6 levels) and its 4 waves, the slots added per thread
(ceil(nblk / 1024) of them) and the tree (10 levels), then one division: D = 6 + 4 + ceil(nblk / 1024) + 10 + 1
roundings, each at most u times the sum of |s|:  E_mean = mean(E_s) + D u mean(|s|).

pools: data movement, exact -- compared bit for bit.

Acceptance bounds of the whole net (against the reference, tests/golden/ref_lpips.json -- never against the code under
test): per net and tap the relative L2 distance of the per-pixel maps s from the float64 truth, pooled over the net's
cases, is at most MARGIN x the reference's own; a pair's value lies within MARGIN x sum_taps (the reference's recorded
mean absolute map error) of the truth.
"""
import hashlib
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
U = 2.0 ** -24
MARGIN = 4.0
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = float(np.float32(1e-10))

# torchvision's ``features`` stacks, written out: C = Conv(c_in, c_out, k, stride, pad), R = ReLU, P = MaxPool(k, stride)
_ALEX = "C3,64,11,4,2 R P3,2 C64,192,5,1,2 R P3,2 C192,384,3,1,1 R C384,256,3,1,1 R C256,256,3,1,1 R P3,2"
_VGG16 = ("C3,64,3,1,1 R C64,64,3,1,1 R P2,2 C64,128,3,1,1 R C128,128,3,1,1 R P2,2 "
          "C128,256,3,1,1 R C256,256,3,1,1 R C256,256,3,1,1 R P2,2 "
          "C256,512,3,1,1 R C512,512,3,1,1 R C512,512,3,1,1 R P2,2 "
          "C512,512,3,1,1 R C512,512,3,1,1 R C512,512,3,1,1 R P2,2")


def _parse(text):
    kinds = {"C": "conv", "R": "relu", "P": "pool"}
    return tuple((kinds[tok[0]],) + tuple(int(v) for v in tok[1:].split(",") if v) for tok in text.split())


LAYERS = {"alex": _parse(_ALEX), "vgg": _parse(_VGG16)}
TARGETS = {"alex": (2, 5, 8, 10, 12), "vgg": (4, 9, 16, 23, 30)}       # counted from 1 (networks.py:82, 93)
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
WEIGHT_SEED = {"alex": 31, "vgg": 32}

# the whole-net cases: name -> (net, pairs, h, w, input seed)
CASES = {
    "alex_1x31x31": ("alex", 1, 31, 31, 1),       # the minimum: taps 7x7, 3x3, 1x1, 1x1, 1x1
    "alex_1x35x47": ("alex", 1, 35, 47, 2),
    "alex_2x67x93": ("alex", 2, 67, 93, 3),
    "alex_2x99x131": ("alex", 2, 99, 131, 4),
    "vgg_1x16x16": ("vgg", 1, 16, 16, 5),         # the minimum
    "vgg_2x24x40": ("vgg", 2, 24, 40, 6),
}
# the planted contract errors the acceptance bounds must catch (test_lpips_host); net: which cases can show it
VARIANTS = {
    "conv1_pad_k_half": "alex",      # conv1 padded by 5 (k / 2) instead of 2
    "zscore_of_padding": None,       # the z-score applied to the padded taps too
    "tap_before_relu": None,
    "ceil_mode_pool": None,
    "normalise_difference": None,    # normalising fx - fy instead of fx and fy
    "abs_difference": None,          # w |a - b| instead of w (a - b)^2
    "vgg_fifth_pool": "vgg",         # the fifth pool run before its tap
}
VGG_POOL5_CASE = ("vgg", 1, 32, 32, 7)   # a size at which a fifth pool is possible at all (tap 5 is 2 x 2)


# ---- builders ----

def build_features(net: str, seed=None) -> dict:
    """The state dict of ``features`` (keys ``<i>.weight`` / ``<i>.bias``), float32: weights N(0, 2 / fan_in) -- ReLU
    halves the second moment, so the activations stay O(1) -- and biases N(0, 0.1)."""
    rs = np.random.RandomState(WEIGHT_SEED[net] if seed is None else seed)
    sd = {}
    for i, L in enumerate(LAYERS[net]):
        if L[0] != "conv":
            continue
        _, c_in, c_out, k, _, _ = L
        sd["%d.weight" % i] = torch.from_numpy((rs.normal(0, 1, (c_out, c_in, k, k)) * np.sqrt(2.0 / (c_in * k * k))).astype(np.float32))
        sd["%d.bias" % i] = torch.from_numpy(rs.normal(0, 0.1, c_out).astype(np.float32))
    return sd


def build_lin(net: str, seed=None) -> dict:
    """The weight file's state dict (keys ``lin<l>.model.1.weight``, [1, C, 1, 1]): U(0, 1) per channel."""
    rs = np.random.RandomState(1000 + (WEIGHT_SEED[net] if seed is None else seed))
    return {"lin%d.model.1.weight" % l: torch.from_numpy(rs.uniform(0, 1, (1, c, 1, 1)).astype(np.float32))
            for l, c in enumerate(CHANNELS[net])}


def renamed(lin: dict) -> dict:
    """``get_state_dict``'s renaming (utils.py:24-29): 'lin' and 'model.' removed from every key."""
    return {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}


def build_pair(pairs: int, h: int, w: int, seed: int):
    """(x, y) float32 [pairs, 3, h, w]: x multiples of 1/255; y = x + N(0, 0.1), clamped to [0, 1] and re-quantised."""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 256, (pairs, 3, h, w))
    x = (q.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    noisy = np.clip(q / 255.0 + rs.normal(0, 0.1, q.shape), 0.0, 1.0)
    y = (np.round(noisy * 255.0).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    return x, y


def case_inputs(name: str):
    """(net, features, lin, x, y) of a whole-net case."""
    net, pairs, h, w, seed = CASES[name] if isinstance(name, str) else name
    x, y = build_pair(pairs, h, w, seed)
    return net, build_features(net), build_lin(net), x, y


def sha256(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def weights_hash(net: str) -> str:
    return sha256(*[v.numpy() for v in build_features(net).values()], *[v.numpy() for v in build_lin(net).values()])


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)) if not isinstance(a, torch.Tensor) else a.to(torch.float64)


# ---- leaf truths (float64) ----

def zscore64(x):
    mean = t64(np.asarray(MEAN, np.float32))[None, :, None, None]
    std = t64(np.asarray(STD, np.float32))[None, :, None, None]
    return (t64(x) - mean) / std


def conv_relu64(x, w, b, k, s, p, zscore=False):
    """(out, bound): relu(b + conv(x)) in float64 and the per-element bound of the float32 evaluation."""
    x, w, b = t64(x), t64(w), t64(b)
    if zscore:
        x = zscore64(x)
    pre = F.conv2d(x, w, b, stride=s, padding=p)
    K = w.shape[1] * k * k
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=s, padding=p)
    return F.relu(pre), (K + (4 if zscore else 2)) * U * S


def normalize64(f):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + EPS)


def distance64(fx, fy, w, variant=None):
    """One tap: (s [P, H, W], mean [P], E_s [P, H, W], E_mean [P]) for features fx, fy [P, C, H, W] and w [C]."""
    fx, fy, w = t64(fx), t64(fy), t64(w).reshape(1, -1, 1, 1)
    C, hw = fx.shape[1], fx.shape[2] * fx.shape[3]
    if variant == "normalise_difference":
        a, b = normalize64(fx - fy), torch.zeros_like(fx)
    else:
        a, b = normalize64(fx), normalize64(fy)
    d = a - b
    t = w * d.abs() if variant == "abs_difference" else w * d * d
    s = t.sum(1)
    r = (C / 2 + 4) * U
    dt = 2 * w.abs() * d.abs() * r * (a.abs() + b.abs()) + 3 * U * t.abs()
    E_s = dt.sum(1) + C * U * t.abs().sum(1)
    nblk = -(-hw // (32 if C <= 192 else 16 if C <= 384 else 8))
    D = 6 + 4 + -(-nblk // 1024) + 10 + 1
    E_mean = E_s.mean((1, 2)) + D * U * s.abs().mean((1, 2))
    return s, s.mean((1, 2)), E_s, E_mean


# ---- the whole computation (float64) ----

def features64(net, features, x, variant=None):
    """The five taps of ``BaseNet.forward`` BEFORE normalize_activation, float64."""
    x = t64(x)
    if variant == "zscore_of_padding":      # conv1 sees the z-score of a zero-padded image: -mean / std in the border
        p = LAYERS[net][0][5]
        x = zscore64(F.pad(x, (p, p, p, p)))
    else:
        x = zscore64(x)
    taps, prev = [], None
    for i, L in enumerate(LAYERS[net], 1):
        if L[0] == "conv":
            pad = L[5]
            if i == 1 and variant == "zscore_of_padding":
                pad = 0
            if i == 1 and variant == "conv1_pad_k_half":
                pad = L[3] // 2
            x = F.conv2d(x, t64(features["%d.weight" % (i - 1)]), t64(features["%d.bias" % (i - 1)]), stride=L[4], padding=pad)
        elif L[0] == "relu":
            prev, x = x, F.relu(x)
        else:
            if variant == "vgg_fifth_pool" and i == len(LAYERS[net]):
                taps.append(F.max_pool2d(x, L[1], L[2]))
                break
            x = F.max_pool2d(x, L[1], L[2], ceil_mode=variant == "ceil_mode_pool")
        if i in TARGETS[net] and not (variant == "vgg_fifth_pool" and i == TARGETS[net][-1]):
            taps.append(prev if variant == "tap_before_relu" else x)
        if len(taps) == 5:
            break
    return taps


def truth64(net, features, lin, x, y, variant=None):
    """{"maps": [s [P, H_l, W_l]], "taps": [P, 5], "values": [P], "total": float} of the whole computation in float64.
    variant: one planted contract error (VARIANTS), None for the truth."""
    fx, fy = features64(net, features, x, variant), features64(net, features, y, variant)
    maps, terms = [], []
    for l, (a, b) in enumerate(zip(fx, fy)):
        s, m, _, _ = distance64(a, b, lin["lin%d.model.1.weight" % l].reshape(-1), variant)
        maps.append(s)
        terms.append(m)
    taps = torch.stack(terms, 1)
    values = taps.sum(1)
    return dict(maps=maps, taps=taps, values=values, total=float(values.sum()))


# ---- the acceptance bounds ----

def rel_l2(got, want) -> float:
    got, want = t64(got), t64(want)
    return float(torch.linalg.norm((got - want).reshape(-1)) / torch.linalg.norm(want.reshape(-1)))


def pooled_map_figures(pairs_of_maps):
    """(relative L2, mean absolute error) of [(got, want)] pooled: sqrt(sum |got - want|^2 / sum |want|^2) and
    sum |got - want| / elements.  Maps of different shapes (a planted error can change them) are cut to the common
    top-left corner."""
    num = den = ab = 0.0
    count = 0
    for got, want in pairs_of_maps:
        got, want = t64(got), t64(want)
        if got.shape != want.shape:
            hh, ww = min(got.shape[-2], want.shape[-2]), min(got.shape[-1], want.shape[-1])
            got, want = got[..., :hh, :ww], want[..., :hh, :ww]
        d = got - want
        num += float((d * d).sum())
        den += float((want * want).sum())
        ab += float(d.abs().sum())
        count += d.numel()
    return (num / den) ** 0.5, ab / max(count, 1)


def acceptance(net, golden, results):
    """results: {case: (maps, values, truth)} with every case of ``net``.  Returns {"map_ratio": [5], "value_ratio":
    {case: [per pair]}}: each figure over its bound's reference part, so the bounds hold iff every ratio <= MARGIN."""
    ref = golden["nets"][net]
    ratios = []
    for l in range(5):
        got, _ = pooled_map_figures([(maps[l], truth["maps"][l]) for maps, _, truth in results.values()])
        ratios.append(got / ref["map_rel_l2"][l])
    budget = sum(ref["map_mean_abs"])
    values = {case: [float(v) / budget for v in (t64(vals) - truth["values"]).abs()] for case, (_, vals, truth) in results.items()}
    return dict(map_ratio=ratios, value_ratio=values)


def within(acc) -> bool:
    return all(r <= MARGIN for r in acc["map_ratio"]) and all(r <= MARGIN for v in acc["value_ratio"].values() for r in v)
