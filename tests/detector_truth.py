"""Builders, float64 truths and error bounds of the detector's network (gaussianrpg_amd/detector.py,
csrc/detector.hip), for tests/test_detector_host.py, tests/test_gpu_detector.py and
tests/golden/make_golden_detector.py.  CPU torch float64 and numpy; legacy ``numpy.random.RandomState`` (stable).

Error bounds (u = 2^-24, the unit roundoff of float32; all first order in u)
---------------------------------------------------------------------------
conv, before the activation.  A plain chain acc = b; acc = fma(w_k, x_k, acc) for k = 0..K-1 makes K roundings, each at
most u times the magnitude of a partial sum, and every partial sum is at most S = |b| + sum_k |w_k x_k| in magnitude.
So |err_pre| <= K u S; the bound used is E = (K + 2) u S (two roundings of slack for the higher-order terms).  Any
other summation order of the same products obeys it as long as no product passes through more than K + 2 roundings:
the reference's, and the kernel's -- fma chains over blocks of 32 k from zero, the block sums added in order onto the
bias: at most 32 + ceil(K / 32) <= K + 2 roundings on a product's way.

SiLU, y = x * (1 / (1 + exp(-x))).  With e = expf(-x) at most 1 ulp off (the device library's stated accuracy; 1 ulp is
at most 2u relative): d = 1 + e carries 2u e / (1 + e) <= 2u inherited plus u of its own rounding, the correctly
rounded division adds u and the product u: the float32 evaluation AT the computed x is within 5u |y|.  The computed x
itself is off by err_pre, which the slope of SiLU, inside [-0.1, 1.1], passes on as at most 1.1 E.  Together
|err_y| <= 1.1 E + 5u |y|.  Without an activation |err_y| <= E.

residual, out = r + y: one more rounding, |err| <= |err_y| + u |r + y|.

BatchNorm folding, w' = w * (g / sqrt(eps + var)), b' = beta - g * mean / sqrt(var + eps), each step one float32
operation: the sum eps + var (u), halved by the square root, the square root (u), the division (u) and the product
(u) give 3.5u: |err_w'| <= 4u |w'|.  The subtracted term t = g * mean / sqrt(..) has product (u), square root with its
argument (1.5u) and division (u): 3.5u, bound 4u |t|, and the subtraction rounds once: |err_b'| <= 4u |t| + u |b'|.

pool, Focus gather, upsample, every concat placement: data movement, exact -- compared bit for bit.
"""
import hashlib
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
YAML = os.path.join(GOLDEN, "ref_yolov5s.yaml")
U = 2.0 ** -24

# the whole-network cases: name -> (narrowed model?, bs, h, w, weight seed, input seed)
CASES = {
    "narrow_32x32": (True, 1, 32, 32, 11, 1),
    "narrow_2x64x96": (True, 2, 64, 96, 11, 2),
    "yolov5s_64x64": (False, 1, 64, 64, 12, 3),
}


def load_cfg(narrow: bool) -> dict:
    """The reference's yolov5s.yaml (a settings-only fixture); narrow: width_multiple 0.25 and nc 3."""
    import yaml
    with open(YAML) as f:
        cfg = yaml.safe_load(f)
    if narrow:
        cfg["width_multiple"] = 0.25
        cfg["nc"] = 3
    return cfg


def spec_of(narrow: bool):
    from gaussianrpg_amd.detector import DetectorSpec
    return DetectorSpec.from_yaml(load_cfg(narrow))


# ---- builders ----

def build_weights(spec, seed: int) -> dict:
    """The UNFUSED state dict of the reference's model for ``spec``, float32, keys ``model.<i>...`` in the reference's
    order.  Conv weights N(0, 3 / fan_in) (SiLU roughly halves the second moment of a centred input, so the
    activations stay O(1) through sixty layers); BatchNorm weight U(0.6, 1.4), bias N(0, 0.2), running mean N(0, 0.2),
    running variance U(0.5, 1.5): folding changes every weight and bias.  Detect: N(0, 1 / fan_in), bias N(0, 1)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in spec.state_dict_shapes(False):
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            v = np.zeros((), np.int64)
        elif leaf in ("anchors", "anchor_grid"):
            ag = spec.anchor_grid.astype(np.float32)
            v = (ag / np.asarray(spec.stride, np.float32)[:, None, None] if leaf == "anchors" else ag).reshape(shape)
        elif ".bn." in key:
            n = shape[0]
            v = {"weight": lambda: rs.uniform(0.6, 1.4, n), "bias": lambda: rs.normal(0, 0.2, n),
                 "running_mean": lambda: rs.normal(0, 0.2, n), "running_var": lambda: rs.uniform(0.5, 1.5, n)}[leaf]()
        elif leaf == "weight":
            fan_in = shape[1] * shape[2] * shape[3]
            gain = 1.8 if ".conv." in key else 1.0
            v = rs.normal(0, 1, shape) * np.sqrt(gain / fan_in)
        else:
            v = rs.normal(0, 1, shape)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v if v.dtype == np.int64 else v.astype(np.float32)))
    return sd


def build_input(bs: int, h: int, w: int, seed: int, ch: int = 3) -> np.ndarray:
    """An image-like float32 [bs, ch, h, w]: multiples of 1/255 in [0, 1], as ``detector_input`` makes them."""
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 256, (bs, ch, h, w)).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def build_tensor(shape, seed: int, negative: bool = False) -> np.ndarray:
    """float32 N(0, 1); negative: strictly negative values (-|N| - 0.01), where a zero padding would win a max."""
    v = np.random.RandomState(seed).normal(0, 1, shape).astype(np.float32)
    return (-np.abs(v) - np.float32(0.01)).astype(np.float32) if negative else v


# the leaf cases the reference's own modules are recorded on (tests/golden/make_golden_detector.py)
LEAVES = {
    "conv_k3_s1_5x7": dict(c1=12, c2=8, k=3, s=1, hw=(5, 7), bs=1, seed=21),
    "conv_k3_s2_7x9": dict(c1=12, c2=18, k=3, s=2, hw=(7, 9), bs=2, seed=22),
    "conv_k1_1x1": dict(c1=12, c2=8, k=1, s=1, hw=(1, 1), bs=1, seed=23),
    "conv_k3_long_chain": dict(c1=512, c2=8, k=3, s=1, hw=(5, 7), bs=1, seed=24),
    "conv_res_5x7": dict(c1=8, c2=8, k=3, s=1, hw=(5, 7), bs=1, seed=25, res=True),
    "focus_6x10": dict(c1=12, c2=8, k=3, s=1, hw=(6, 10), bs=2, seed=26, focus=True),
    "pool_14x20": dict(c1=4, hw=(14, 20), bs=2, seed=27, pool=True),
    "pool_negative_3x4": dict(c1=3, hw=(3, 4), bs=1, seed=28, pool=True, negative=True),
}


def leaf_inputs(name: str) -> dict:
    """x (for Focus the stored [bs, c1 / 4, h, w] image), w, b, res of a leaf case; w ~ N(0, 1 / fan_in), b ~ N(0, 1)."""
    c = LEAVES[name]
    rs = np.random.RandomState(c["seed"])
    h, w = c["hw"]
    if c.get("pool"):
        return dict(x=build_tensor((c["bs"], c["c1"], h, w), c["seed"], c.get("negative", False)))
    cx = c["c1"] // 4 if c.get("focus") else c["c1"]
    out = dict(x=rs.normal(0, 1, (c["bs"], cx, h, w)).astype(np.float32),
               w=(rs.normal(0, 1, (c["c2"], c["c1"], c["k"], c["k"])) / np.sqrt(c["c1"] * c["k"] ** 2)).astype(np.float32),
               b=rs.normal(0, 1, c["c2"]).astype(np.float32), res=None)
    if c.get("res"):
        out["res"] = rs.normal(0, 1, (c["bs"], c["c2"], h, w)).astype(np.float32)
    return out


def sha256(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_inputs(name: str):
    """(spec, unfused state dict, x) of a whole-network case."""
    narrow, bs, h, w, wseed, xseed = CASES[name]
    spec = spec_of(narrow)
    return spec, build_weights(spec, wseed), build_input(bs, h, w, xseed)


# ---- leaf truths (float64) ----

def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)) if not isinstance(a, torch.Tensor) else a.to(torch.float64)


def focus64(x):
    """Focus's slicing (common.py:175) on [bs, c, h, w]: (even row, even col), (odd, even), (even, odd), (odd, odd)."""
    return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


def upsample64(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def conv64(x, w, b, k, s, act=True, res=None, focus=False, variant=None):
    """(out, bound): the float64 value of ``act(b + conv(x, w)) [+ res]`` and the per-element bound of the float32
    evaluation (module docstring).  variant: one planted error (test_detector_host), None for the truth."""
    x, w, b = t64(x), t64(w), t64(b)
    if focus:
        x = focus64(x) if variant != "focus_order" else torch.cat(
            [x[..., ::2, ::2], x[..., ::2, 1::2], x[..., 1::2, ::2], x[..., 1::2, 1::2]], 1)
    ww = w.transpose(2, 3) if variant == "kykx" else w
    bb = torch.zeros_like(b) if variant == "no_bias" else b
    p = k // 2
    if variant == "pad_off":       # the window shifted by one: padding p + 1 in front, p - 1 behind
        xp = F.pad(x, (p + 1, p - 1, p + 1, p - 1))
        pre = F.conv2d(xp, ww, bb, stride=s)
    elif variant == "stride_phase":  # samples 1, 3, 5 ... in place of 0, 2, 4 ...
        xp = F.pad(x, (p, p + 1, p, p + 1))[..., 1:, 1:]
        pre = F.conv2d(xp, ww, bb, stride=s)[..., :(x.shape[2] + 2 * p - k) // s + 1, :(x.shape[3] + 2 * p - k) // s + 1]
    else:
        pre = F.conv2d(x, ww, bb, stride=s, padding=p)
    K = w.shape[1] * k * k
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=s, padding=p)
    E = (K + 2) * U * S
    if variant == "res_before_act" and res is not None:
        return silu64(pre + t64(res)), None
    y = silu64(pre) if act else pre
    bound = 1.1 * E + 5 * U * y.abs() if act else E
    if res is not None and variant != "no_res":
        y = t64(res) + y
        bound = bound + U * y.abs()
    return y, bound


def pool64(x, pad_value=-np.inf):
    """SPP's three pools of [bs, c, h, w] -> [bs, 3c, h, w] (5, then 9, then 13), in the input's dtype: exact."""
    x = torch.as_tensor(x)
    out = []
    for k in (5, 9, 13):
        xp = F.pad(x, (k // 2,) * 4, value=pad_value)
        out.append(F.max_pool2d(xp, k, 1, 0))
    return torch.cat(out, 1)


def fold64(w, g, beta, mean, var, eps):
    """((w', bound), (b', bound)) of the BatchNorm folding in float64."""
    w, g, beta, mean, var = (t64(v) for v in (w, g, beta, mean, var))
    scale = g / torch.sqrt(var + eps)
    wf = w * scale.reshape(-1, 1, 1, 1)
    t = g * mean / torch.sqrt(var + eps)
    bf = beta - t
    return (wf, 4 * U * wf.abs()), (bf, 4 * U * t.abs() + U * bf.abs())


# ---- the whole network (float64) ----

def network64(spec, state_dict, x, variant=None):
    """(heads, layers): the nl heads and every layer's output of the network in float64, its own walk of the spec:
    BatchNorm folded in float64 from the unfused tensors.  variant: "concat_swapped" / "upsample_shift" plant that
    error in every Concat / Upsample (test_detector_host)."""
    def get(key):
        return t64(state_dict["model." + key])

    def conv(key, v, k=1, s=1, act=True, plain=False):
        if plain:
            w, b = get(key + ".weight"), get(key + ".bias")
        else:
            (w, _), (b, _) = fold64(get(key + ".conv.weight"), get(key + ".bn.weight"), get(key + ".bn.bias"),
                                    get(key + ".bn.running_mean"), get(key + ".bn.running_var"), spec.bn_eps)
        y = F.conv2d(v, w, b, stride=s, padding=k // 2)
        return silu64(y) if act else y

    x = t64(x)
    ys, heads = [], None
    for i, L in enumerate(spec.layers):
        ins = [x if j < 0 else ys[j] for j in L["f"]]
        t, v = L["type"], ins[0]
        if t == "Focus":
            y = conv("%d.conv" % i, focus64(v), L["k"], L["s"])
        elif t == "Conv":
            y = conv("%d" % i, v, L["k"], L["s"])
        elif t == "C3":
            m = conv("%d.cv1" % i, v)
            for j in range(L["n"]):
                z = conv("%d.m.%d.cv2" % (i, j), conv("%d.m.%d.cv1" % (i, j), m), 3)
                m = m + z if L["shortcut"] else z
            y = conv("%d.cv3" % i, torch.cat((m, conv("%d.cv2" % i, v)), 1))
        elif t == "SPP":
            v = conv("%d.cv1" % i, v)
            y = conv("%d.cv2" % i, torch.cat((v, pool64(v)), 1))
        elif t == "Upsample":
            y = upsample64(v)
            if variant == "upsample_shift":
                y = torch.roll(y, 1, 3)
        elif t == "Concat":
            y = torch.cat(ins[::-1] if variant == "concat_swapped" else ins, 1)
        else:
            heads = [conv("%d.m.%d" % (i, l), h, act=False, plain=True) for l, h in enumerate(ins)]
            y = None
        ys.append(y)
    return heads, ys


def rel_l2(got, want) -> float:
    got, want = t64(got), t64(want)
    return float(torch.linalg.norm((got - want).reshape(-1)) / torch.linalg.norm(want.reshape(-1)))


def worst(got, want) -> float:
    return float((t64(got) - t64(want)).abs().max())


# ---- a duck-typed stand-in for the reference's live Model (DetectorSpec.from_module) ----

def _cls(name):
    return type(name, (), {})


class _Conv2d:
    def __init__(self, c1, c2, k=1, s=1):
        self.in_channels, self.out_channels, self.kernel_size, self.stride = c1, c2, (k, k), (s, s)
        self.padding, self.groups = (k // 2, k // 2), 1


def stand_in_model(spec, state_dict=None, fused=False, **planted):
    """An object tree with the reference's class names and attributes (``.model`` a list of modules with ``.i``,
    ``.f``, ``Conv.conv`` / ``.bn`` / ``.act`` ...), built from the spec -- what ``from_module`` walks.  planted:
    ``groups=2`` / ``act="Hardswish"`` / ``block="TransformerBlock"`` on the first matching module, for the refusals."""
    SiLU, BN, MaxPool = _cls(planted.get("act", "SiLU")), _cls("BatchNorm2d"), _cls("MaxPool2d")
    names = {n: _cls(n) for n in ("Conv", "Focus", "C3", "SPP", "Upsample", "Concat", "Detect", "Bottleneck")}

    def Conv(c1, c2, k=1, s=1):
        m = names["Conv"]()
        m.conv, m.act = _Conv2d(c1, c2, k, s), SiLU()
        m.conv.groups = planted.pop("groups", 1)
        if not fused:
            m.bn = BN()
            m.bn.eps = spec.bn_eps
        return m

    mods = []
    for i, L in enumerate(spec.layers):
        t = L["type"]
        m = names[t]()
        if t == "Focus":
            m.conv = Conv(4 * L["c1"], L["c2"], L["k"], L["s"])
        elif t == "Conv":
            m = Conv(L["c1"], L["c2"], L["k"], L["s"])
        elif t == "C3":
            m.cv1, m.cv2, m.cv3 = Conv(L["c1"], L["c_"]), Conv(L["c1"], L["c_"]), Conv(2 * L["c_"], L["c2"])
            m.m = []
            for _ in range(L["n"]):
                b = _cls(planted.pop("block", "Bottleneck"))()
                b.cv1, b.cv2, b.add = Conv(L["c_"], L["c_"]), Conv(L["c_"], L["c_"], 3), L["shortcut"]
                m.m.append(b)
        elif t == "SPP":
            m.cv1, m.cv2 = Conv(L["c1"], L["c_"]), Conv(4 * L["c_"], L["c2"])
            m.m = []
            for k in (5, 9, 13):
                p = MaxPool()
                p.kernel_size = k
                m.m.append(p)
        elif t == "Upsample":
            m.scale_factor, m.mode = 2.0, "nearest"
        elif t == "Concat":
            m.d = 1
        else:
            m.nc, m.na, m.nl = spec.nc, spec.na, spec.nl
            m.anchor_grid = torch.from_numpy(spec.anchor_grid.copy()).view(spec.nl, 1, spec.na, 1, 1, 2)
            m.stride = torch.tensor(spec.stride)
            m.m = [_Conv2d(c, spec.na * spec.no) for c in L["ch"]]
        m.i = i
        m.f = L["from"]
        mods.append(m)
    model = _cls("Model")()
    model.model = mods
    model.state_dict = lambda: state_dict
    return model
