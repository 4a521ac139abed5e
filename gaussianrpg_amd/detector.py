"""The detector's network on the device: the inference forward of the reference's YOLOv5 between ``detector_input``
and ``detections_from_heads`` (models/yolo.py:119-159 over models/common.py: ``Focus``, ``Conv``, ``Bottleneck``,
``C3``, ``SPP``, ``nn.Upsample``, ``Concat`` and ``Detect``'s 1x1 convs), as ONE native call per frame: FP32
(csrc/detector.hip) or, with ``dtype=torch.float16``, fp16 activations
and weights with float32 accumulation and float32 heads (csrc/detector_f16.hip).

    spec = DetectorSpec.from_yaml("yolov5s.yaml")            # or DetectorSpec.from_module(attempt_load(...))
    net = DetectorNet(spec, state_dict)                      # fused or unfused tensors, the reference's keys
    net = DetectorNet(spec, state_dict, dtype=torch.float16) # takes detector_input(..., dtype=torch.float16)
    heads = net(detector_input(frame["rgb8"], plan))         # the nl conv outputs [bs, na*(5+nc), ny, nx]
    det, count = net.detections(x, plan=plan)

``DetectorSpec`` is host only: the layer list ``parse_model`` (yolo.py:234-290) derives from the yaml.  ``DetectorNet``
folds BatchNorm on the host as ``fuse_conv_and_bn`` does (utils/torch_utils.py:263-300), repacks every weight once on
the device, and per input shape builds a *plan*: one activation arena and the launch list.  Everything the reference
does around a convolution is part of a convolution's launch record: SiLU, the Bottleneck shortcut, Focus's slicing,
``Concat`` / ``torch.cat`` (producers write into a channel slice of the consumer's buffer) and ``nn.Upsample`` (a
second, 2 x 2 replicated store of the producer).  Only SPP's three max-pools are a launch of their own, one for all.

Not here: bf16 execution, loading a pickled ``.pt``, augmented inference, training.
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .perception import DetectGeometry, LetterboxPlan, MAX_NMS, detections_from_heads

# grpg_detector_layer (include/grpg_rasterizer.h)
KIND_CONV, KIND_POOL = 0, 1
ACT_NONE, ACT_SILU = 0, 1
IN_PLAIN, IN_FOCUS = 0, 1
TILE_128, TILE_64 = 0, 1
RECORD_FIELDS = ("kind", "in", "in_c0", "in_ct", "out", "out_c0", "out_ct", "res", "res_c0", "res_ct", "up", "up_c0",
                 "up_ct", "packed", "bs", "c_in", "c_out", "h_in", "w_in", "h_out", "w_out", "k", "stride", "act",
                 "in_mode", "tile")
RECORD_FIELDS_F16 = RECORD_FIELDS + ("out_f32",)   # grpg_detector_layer_f16
SPP_KERNELS = (5, 9, 13)
CUS = 256   # MI355X: the tile policy wants at least one 128 x 128 tile per compute unit

_SUPPORTED = ("Focus", "Conv", "C3", "SPP", "Upsample", "Concat", "Detect")


def make_divisible(x, divisor):
    """utils/general.py: ``math.ceil(x / divisor) * divisor``."""
    return math.ceil(x / divisor) * divisor


def _module_name(m) -> str:
    if isinstance(m, str):
        return m.replace("nn.", "")
    return getattr(m, "__name__", type(m).__name__)


class DetectorSpec:
    """The network on the host: no device, no weights.

      layers       one dict per layer of the yaml, ``{"type", "from", "f", ...}``: ``from`` as the yaml has it, ``f`` the
                   absolute indices of the layers read (-1: the network's input); Focus / Conv carry c1, c2, k, s;
                   C3 c1, c2, n, shortcut, c_ (hidden); SPP c1, c2, c_; Concat and Detect their input channels ``ch``
      save         the reference's save list (sorted indices of layers read by a later, non-adjacent layer)
      stride       [nl] of the Detect levels, from the layers' strides
      anchor_grid  [nl, na, 2] in pixels (``Detect.anchor_grid``)
      nc, na, nl   classes, anchors per level, levels
      bn_eps       the BatchNorm eps an unfused state dict is folded with (the reference's ``initialize_weights``
                   sets 1e-3; ``from_module`` reads it from the model where it still has BatchNorm)"""

    def __init__(self, layers, anchor_grid, stride, nc, save, ch_in=3, bn_eps=1e-3):
        self.layers = layers
        self.anchor_grid = np.asarray(anchor_grid, dtype=np.float32)
        self.stride = [float(s) for s in stride]
        self.nc, self.ch_in, self.bn_eps = int(nc), int(ch_in), float(bn_eps)
        self.nl, self.na = int(self.anchor_grid.shape[0]), int(self.anchor_grid.shape[1])
        self.no = self.nc + 5
        self.save = sorted(save)
        if layers[-1]["type"] != "Detect" or any(L["type"] == "Detect" for L in layers[:-1]):
            raise ValueError("DetectorSpec: the last layer, and only the last, must be Detect")

    # ---- the two doors ----
    @classmethod
    def from_yaml(cls, cfg: Union[dict, str], ch: int = 3, nc: Optional[int] = None) -> "DetectorSpec":
        """``parse_model(cfg, [ch])`` for the supported modules; ``cfg`` is the yaml's dict or its path."""
        if not isinstance(cfg, dict):
            import yaml
            with open(cfg) as f:
                cfg = yaml.safe_load(f)
        anchors, gd, gw = cfg["anchors"], cfg["depth_multiple"], cfg["width_multiple"]
        nc = int(cfg["nc"] if nc is None else nc)
        if not isinstance(anchors, (list, tuple)):
            raise ValueError("DetectorSpec: anchors given as a count (autoanchor) are not supported")
        na = len(anchors[0]) // 2
        no = na * (nc + 5)
        layers, save, chs, scale = [], [], [], []   # scale: input pixels per pixel of the layer's output
        for i, (f, n, m, args) in enumerate(list(cfg["backbone"]) + list(cfg["head"])):
            name = _module_name(m)
            if name not in _SUPPORTED:
                raise ValueError("DetectorSpec: layer %d: module %s is not supported" % (i, name))
            args = [nc if a == "nc" else anchors if a == "anchors" else None if a == "None" else a for a in args]
            fl = [f] if isinstance(f, int) else list(f)
            fa = [(i - 1 if x == -1 else x % i if i else -1) for x in fl]   # absolute; layer 0 reads the input
            if i == 0:
                fa = [-1]
            c_of = lambda j: ch if j < 0 else chs[j]
            s_of = lambda j: 1 if j < 0 else scale[j]
            n = max(round(n * gd), 1) if n > 1 else n
            L = {"type": name, "from": f if isinstance(f, int) else list(f), "f": fa}
            if name in ("Focus", "Conv", "C3", "SPP"):
                c1, c2 = c_of(fa[0]), args[0]
                if c2 != no:
                    c2 = make_divisible(c2 * gw, 8)
                L.update(c1=c1, c2=c2)
                sc = s_of(fa[0])
                if name in ("Focus", "Conv"):
                    k = args[1] if len(args) > 1 else 1
                    s = args[2] if len(args) > 2 else 1
                    if len(args) > 3 and args[3] not in (None, k // 2):
                        raise ValueError("DetectorSpec: layer %d: %s padding %r is not k // 2" % (i, name, args[3]))
                    if len(args) > 4 and args[4] != 1:
                        raise ValueError("DetectorSpec: layer %d: %s with groups %r is not supported" % (i, name, args[4]))
                    if len(args) > 5 and args[5] is not True:
                        raise ValueError("DetectorSpec: layer %d: %s with a non-SiLU activation is not supported" % (i, name))
                    if k not in (1, 3) or s not in (1, 2):
                        raise ValueError("DetectorSpec: layer %d: %s with kernel %r, stride %r is not supported (kernel "
                                         "1 or 3, stride 1 or 2)" % (i, name, k, s))
                    if n != 1:
                        raise ValueError("DetectorSpec: layer %d: %s repeated %d times is not supported" % (i, name, n))
                    L.update(k=k, s=s)
                    sc = sc * s * (2 if name == "Focus" else 1)
                elif name == "C3":
                    shortcut = args[1] if len(args) > 1 else True
                    if len(args) > 2 and args[2] != 1:
                        raise ValueError("DetectorSpec: layer %d: C3 with groups %r is not supported" % (i, args[2]))
                    e = args[3] if len(args) > 3 else 0.5
                    L.update(n=n, shortcut=bool(shortcut), c_=int(c2 * e))
                else:
                    ks = tuple(args[1]) if len(args) > 1 else SPP_KERNELS
                    if ks != SPP_KERNELS:
                        raise ValueError("DetectorSpec: layer %d: SPP with kernels %r is not supported (5, 9, 13)" % (i, ks))
                    L.update(c_=c1 // 2)
            elif name == "Upsample":
                if len(args) < 2 or args[0] is not None or args[1] != 2 or (len(args) > 2 and args[2] != "nearest"):
                    raise ValueError("DetectorSpec: layer %d: only nn.Upsample(None, 2, 'nearest') is supported" % i)
                c2, sc = c_of(fa[0]), s_of(fa[0]) / 2
            elif name == "Concat":
                if args and args[0] != 1:
                    raise ValueError("DetectorSpec: layer %d: Concat over dimension %r is not supported" % (i, args[0]))
                L["ch"] = [c_of(j) for j in fa]
                c2, sc = sum(L["ch"]), s_of(fa[0])
            else:   # Detect
                L["ch"] = [c_of(j) for j in fa]
                c2, sc = no, 0
            save.extend(x for x, raw in zip(fa, fl) if raw != -1)
            layers.append(L)
            chs.append(c2)
            scale.append(sc)
        det = layers[-1]
        if det["type"] != "Detect" or len(anchors) != len(det["f"]):
            raise ValueError("DetectorSpec: the last layer must be Detect with one anchor row per input")
        stride = [scale[j] for j in det["f"]]
        ag = np.asarray(anchors, dtype=np.float32).reshape(len(anchors), -1, 2)
        return cls(layers, ag, stride, nc, sorted(set(save)), ch_in=ch)

    @classmethod
    def from_module(cls, model) -> "DetectorSpec":
        """From a live reference ``Model`` (what ``attempt_load`` returns), fused or not -- or anything shaped like it:
        goes by class name, ``.f`` and ``.i``, as ``DetectGeometry.from_module`` does."""
        seq = getattr(model, "model", model)
        mods = list(seq)
        layers, save, chs, scale = [], [], [], []
        eps = None

        def conv_of(i, name, m):   # a reference Conv: .conv (nn.Conv2d), maybe .bn, .act
            nonlocal eps
            c = m.conv
            k, s, p = _pair(c.kernel_size), _pair(c.stride), _pair(c.padding)
            if type(m).__name__ != "Conv":
                raise ValueError("DetectorSpec: layer %d: %s holds a %s where a Conv is expected" % (i, name, type(m).__name__))
            if int(c.groups) != 1:
                raise ValueError("DetectorSpec: layer %d: %s with groups %d (DWConv) is not supported" % (i, name, c.groups))
            if k[0] != k[1] or k[0] not in (1, 3) or s[0] != s[1] or s[0] not in (1, 2) or p != (k[0] // 2, k[0] // 2):
                raise ValueError("DetectorSpec: layer %d: %s with kernel %r, stride %r, padding %r is not supported" %
                                 (i, name, k, s, p))
            if type(m.act).__name__ != "SiLU":
                raise ValueError("DetectorSpec: layer %d: %s with activation %s is not supported (SiLU only)" %
                                 (i, name, type(m.act).__name__))
            if eps is None and getattr(m, "bn", None) is not None:
                eps = float(m.bn.eps)
            return int(c.in_channels), int(c.out_channels), k[0], s[0]

        for idx, m in enumerate(mods):
            i, f = int(getattr(m, "i", idx)), m.f
            name = type(m).__name__
            if name not in _SUPPORTED:
                raise ValueError("DetectorSpec: layer %d: module %s is not supported" % (i, name))
            fl = [f] if isinstance(f, int) else list(f)
            fa = [-1] if i == 0 else [(i - 1 if x == -1 else x % i) for x in fl]
            s_of = lambda j: 1 if j < 0 else scale[j]
            L = {"type": name, "from": f if isinstance(f, int) else list(f), "f": fa}
            if name == "Focus":
                c1, c2, k, s = conv_of(i, "Focus", m.conv)
                L.update(c1=c1 // 4, c2=c2, k=k, s=s)
                sc = s_of(fa[0]) * 2 * s
            elif name == "Conv":
                c1, c2, k, s = conv_of(i, "Conv", m)
                L.update(c1=c1, c2=c2, k=k, s=s)
                sc = s_of(fa[0]) * s
            elif name == "C3":
                c1, c_, _, _ = conv_of(i, "C3.cv1", m.cv1)
                conv_of(i, "C3.cv2", m.cv2)
                _, c2, _, _ = conv_of(i, "C3.cv3", m.cv3)
                blocks = list(m.m)
                for b in blocks:
                    if type(b).__name__ != "Bottleneck":
                        raise ValueError("DetectorSpec: layer %d: C3 holds a %s (C3TR?), which is not supported" %
                                         (i, type(b).__name__))
                    conv_of(i, "Bottleneck.cv1", b.cv1)
                    conv_of(i, "Bottleneck.cv2", b.cv2)
                L.update(c1=c1, c2=c2, n=len(blocks), shortcut=bool(blocks[0].add) if blocks else False, c_=c_)
                sc = s_of(fa[0])
            elif name == "SPP":
                c1, c_, _, _ = conv_of(i, "SPP.cv1", m.cv1)
                _, c2, _, _ = conv_of(i, "SPP.cv2", m.cv2)
                ks = tuple(int(_pair(p.kernel_size)[0]) for p in m.m)
                if ks != SPP_KERNELS:
                    raise ValueError("DetectorSpec: layer %d: SPP with kernels %r is not supported (5, 9, 13)" % (i, ks))
                L.update(c1=c1, c2=c2, c_=c_)
                sc = s_of(fa[0])
            elif name == "Upsample":
                if float(_pair(m.scale_factor)[0]) != 2.0 or m.mode != "nearest":
                    raise ValueError("DetectorSpec: layer %d: only nn.Upsample(None, 2, 'nearest') is supported" % i)
                c2, sc = chs[fa[0]], s_of(fa[0]) / 2
            elif name == "Concat":
                if int(getattr(m, "d", 1)) != 1:
                    raise ValueError("DetectorSpec: layer %d: Concat over dimension %r is not supported" % (i, m.d))
                L["ch"] = [chs[j] for j in fa]
                c2, sc = sum(L["ch"]), s_of(fa[0])
            else:
                L["ch"] = [int(c.in_channels) for c in m.m]
                det, c2, sc = m, int(m.m[0].out_channels), 0
            c2 = L.get("c2", c2)
            save.extend(x for x, raw in zip(fa, fl) if raw != -1)
            layers.append(L)
            chs.append(c2)
            scale.append(sc)
        geom = DetectGeometry.from_module(det)
        return cls(layers, geom.anchor_grid, [float(s) for s in geom.stride], geom.nc, sorted(set(save)),
                   ch_in=layers[0]["c1"], bn_eps=1e-3 if eps is None else eps)

    # ---- what follows from the layers ----
    def convs(self) -> List[dict]:
        """Every convolution in state-dict order: ``{"key", "c1", "c2", "k", "s", "act", "bias"}``; ``key`` is the
        prefix of its tensors (``<key>.conv.weight`` ... for a Conv, ``<key>.weight`` / ``<key>.bias`` for Detect's)."""
        out = []

        def add(key, c1, c2, k=1, s=1):
            out.append(dict(key=key, c1=c1, c2=c2, k=k, s=s, act=True, plain=False))

        for i, L in enumerate(self.layers):
            t = L["type"]
            if t == "Focus":
                add("%d.conv" % i, 4 * L["c1"], L["c2"], L["k"], L["s"])
            elif t == "Conv":
                add("%d" % i, L["c1"], L["c2"], L["k"], L["s"])
            elif t == "C3":
                add("%d.cv1" % i, L["c1"], L["c_"])
                add("%d.cv2" % i, L["c1"], L["c_"])
                add("%d.cv3" % i, 2 * L["c_"], L["c2"])
                for j in range(L["n"]):
                    add("%d.m.%d.cv1" % (i, j), L["c_"], L["c_"])
                    add("%d.m.%d.cv2" % (i, j), L["c_"], L["c_"], 3)
            elif t == "SPP":
                add("%d.cv1" % i, L["c1"], L["c_"])
                add("%d.cv2" % i, 4 * L["c_"], L["c2"])
            elif t == "Detect":
                for l, c in enumerate(L["ch"]):
                    out.append(dict(key="%d.m.%d" % (i, l), c1=c, c2=self.na * self.no, k=1, s=1, act=False, plain=True))
        return out

    def state_dict_shapes(self, fused: bool, prefix: str = "model.") -> List[Tuple[str, Tuple[int, ...]]]:
        """(key, shape) of every tensor of the reference's ``state_dict()``, in its order."""
        out = []
        det = len(self.layers) - 1
        for c in self.convs():
            if c["plain"]:
                continue
            k = prefix + c["key"]
            out.append((k + ".conv.weight", (c["c2"], c["c1"], c["k"], c["k"])))
            if fused:
                out.append((k + ".conv.bias", (c["c2"],)))
            else:
                out += [(k + ".bn.weight", (c["c2"],)), (k + ".bn.bias", (c["c2"],)), (k + ".bn.running_mean", (c["c2"],)),
                        (k + ".bn.running_var", (c["c2"],)), (k + ".bn.num_batches_tracked", ())]
        out.append((prefix + "%d.anchors" % det, (self.nl, self.na, 2)))
        out.append((prefix + "%d.anchor_grid" % det, (self.nl, 1, self.na, 1, 1, 2)))
        for c in self.convs():
            if c["plain"]:
                out += [(prefix + c["key"] + ".weight", (c["c2"], c["c1"], 1, 1)), (prefix + c["key"] + ".bias", (c["c2"],))]
        return out

    def parameters(self) -> int:
        """The trainable parameter count of the unfused model."""
        return sum(int(np.prod(s)) for k, s in self.state_dict_shapes(False)
                   if not k.endswith(("running_mean", "running_var", "num_batches_tracked", "anchors", "anchor_grid")))

    @property
    def max_stride(self) -> int:
        return int(max(self.stride))

    def geometry(self) -> DetectGeometry:
        return DetectGeometry(self.anchor_grid, self.stride, self.nc)

    def as_dict(self) -> dict:
        return {"layers": self.layers, "anchor_grid": self.anchor_grid.tolist(), "stride": self.stride, "nc": self.nc,
                "save": self.save, "ch_in": self.ch_in, "bn_eps": self.bn_eps}

    def __eq__(self, other):
        return isinstance(other, DetectorSpec) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return "DetectorSpec(%d layers, %d convs, nc=%d, stride=%s)" % (len(self.layers), len(self.convs()), self.nc,
                                                                        self.stride)


def _pair(v):
    return (v, v) if not isinstance(v, (tuple, list)) else tuple(v)


def fold_conv_bn(weight, bn_weight, bn_bias, mean, var, eps, conv_bias=None):
    """``fuse_conv_and_bn`` (utils/torch_utils.py:263-300) in the tensors' own dtype: ``diag(g / sqrt(eps + var))``
    times the weight, and ``bn_bias - g * mean / sqrt(var + eps)`` (plus the scaled conv bias, if any).  The reference's
    ``torch.mm`` with a diagonal matrix adds exact zeros to each product, so the elementwise form has its bits."""
    scale = bn_weight / torch.sqrt(eps + var)
    w = weight * scale.reshape(-1, 1, 1, 1)
    b = bn_bias - bn_weight * mean / torch.sqrt(var + eps)
    if conv_bias is not None:
        b = scale * conv_bias + b
    return w, b


def fused_parameters(spec: DetectorSpec, state_dict: Dict[str, torch.Tensor], dtype=torch.float32) -> List[Tuple]:
    """[(weight, bias)] in ``spec.convs()`` order on the host in ``dtype``, from fused (``conv.weight`` + ``conv.bias``)
    or unfused (``conv.weight`` + ``bn.*``) tensors under ``model.<i>...`` or ``<i>...`` keys."""
    def get(key, required=True):
        for k in ("model." + key, key):
            if k in state_dict:
                return torch.as_tensor(state_dict[k]).detach().to("cpu", dtype)
        if required:
            raise KeyError("DetectorNet: the state dict has neither 'model.%s' nor '%s'" % (key, key))
        return None

    out = []
    for c in spec.convs():
        key = c["key"]
        if c["plain"]:
            w, b = get(key + ".weight"), get(key + ".bias")
        else:
            w = get(key + ".conv.weight")
            b = get(key + ".conv.bias", required=False)
            g = get(key + ".bn.weight", required=False)
            if g is not None:
                w, b = fold_conv_bn(w, g, get(key + ".bn.bias"), get(key + ".bn.running_mean"),
                                    get(key + ".bn.running_var"), spec.bn_eps, b)
            elif b is None:
                raise KeyError("DetectorNet: '%s' has neither conv.bias (fused) nor bn.* (unfused) tensors" % key)
        want = (c["c2"], c["c1"], c["k"], c["k"])
        if tuple(w.shape) != want or tuple(b.shape) != (c["c2"],):
            raise ValueError("DetectorNet: '%s' has weight %s and bias %s, the spec needs %s and [%d]" %
                             (key, list(w.shape), list(b.shape), list(want), c["c2"]))
        out.append((w.contiguous(), b.contiguous()))
    return out


# ---- launch records ----

def out_size(n: int, k: int, s: int) -> int:
    return (n + 2 * (k // 2) - k) // s + 1


def choose_tile(c_out: int, n_pixels: int) -> int:
    """The tile policy: 128 x 128 outputs per workgroup where the layer has at least 96 output channels (a narrower
    layer would leave over a quarter of the tile's rows empty) AND fills every compute unit with such tiles; 64 x 64
    otherwise -- the narrow early layers and the stride-32 level (2400 pixels x 512 channels at 1920 x 1280 is 76 large
    tiles for 256 compute units, 304 small ones).  The result does not depend on the choice."""
    if c_out >= 96 and -(-c_out // 128) * -(-n_pixels // 128) >= CUS:
        return TILE_128
    return TILE_64


def conv_record(in_ptr, in_c0, in_ct, h_in, w_in, out_ptr, out_c0, out_ct, packed_ptr, bs, c_in, c_out, k, stride, act,
                res=None, up=None, focus=False, tile=None) -> List[int]:
    """One GRPG_DET_CONV row.  res / up: (ptr, c0, ct) or None.  h_in, w_in: the STORED input's."""
    lh, lw = (h_in // 2, w_in // 2) if focus else (h_in, w_in)
    h_out, w_out = out_size(lh, k, stride), out_size(lw, k, stride)
    rp, rc0, rct = res if res is not None else (0, 0, 0)
    up_, uc0, uct = up if up is not None else (0, 0, 0)
    if tile is None:
        tile = choose_tile(c_out, bs * h_out * w_out)
    return [KIND_CONV, in_ptr, in_c0, in_ct, out_ptr, out_c0, out_ct, rp, rc0, rct, up_, uc0, uct, packed_ptr, bs, c_in,
            c_out, h_in, w_in, h_out, w_out, k, stride, ACT_SILU if act else ACT_NONE, IN_FOCUS if focus else IN_PLAIN,
            tile]


def pool_record(in_ptr, in_c0, in_ct, out_ptr, out_c0, out_ct, bs, c, h, w) -> List[int]:
    """One GRPG_DET_POOL row: SPP's 5 / 9 / 13 pools of [in_c0, in_c0 + c) into [out_c0, out_c0 + 3 c)."""
    return [KIND_POOL, in_ptr, in_c0, in_ct, out_ptr, out_c0, out_ct, 0, 0, 0, 0, 0, 0, 0, bs, c, 3 * c, h, w, h, w,
            0, 0, 0, 0, 0]


def conv_record_f16(*args, out_f32=False, **kw) -> List[int]:
    """One GRPG_DET_CONV row of the fp16 network: ``conv_record``'s arguments; out_f32: ``out`` is float32 (Detect's
    heads; no res, no up)."""
    return conv_record(*args, **kw) + [int(bool(out_f32))]


def pool_record_f16(*args) -> List[int]:
    """One GRPG_DET_POOL row of the fp16 network: ``pool_record``'s arguments."""
    return pool_record(*args) + [0]


def _C():
    from .rasterizer import _C as ext
    return ext


def pack_weights(weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [c_out, c_in, k, k] (+ [c_out] bias) on the device -> the buffer the convolution streams: one launch."""
    if bias is None:
        bias = torch.zeros(weight.shape[0], dtype=weight.dtype, device=weight.device)
    return _C().detector_pack_weights(weight.contiguous(), bias.contiguous())


def run_records(records: Union[torch.Tensor, Sequence[Sequence[int]]], like: torch.Tensor) -> None:
    """Enqueue rows of ``conv_record`` / ``pool_record`` in ONE native call on the current stream; no host wait."""
    if not isinstance(records, torch.Tensor):
        records = torch.tensor([list(map(int, r)) for r in records], dtype=torch.int64)
    _C().detector_run(records, like)


def pack_weights_f16(weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The SAME float32 [c_out, c_in, k, k] (+ [c_out] bias) on the device -> the fp16 network's buffer, uint8:
    [bias: M_pad float32][M_pad][K_pad] fp16 with c_out padded to 128, K to 32 and zeros in the padding; the weight is
    rounded once, to nearest even, in the launch."""
    if bias is None:
        bias = torch.zeros(weight.shape[0], dtype=weight.dtype, device=weight.device)
    return _C().detector_pack_weights_f16(weight.contiguous(), bias.contiguous())


def run_records_f16(records: Union[torch.Tensor, Sequence[Sequence[int]]], like: torch.Tensor) -> None:
    """``run_records`` for rows of ``conv_record_f16`` / ``pool_record_f16``."""
    if not isinstance(records, torch.Tensor):
        records = torch.tensor([list(map(int, r)) for r in records], dtype=torch.int64)
    _C().detector_run_f16(records, like)


class DetectorPlan:
    """What ``DetectorNet.plan`` builds for one (bs, h, w, device): the arena, the records, the heads (views of the
    arena) and, for the tests, the symbolic launch list ``steps`` the records were made from."""

    def __init__(self, bs, h, w, device):
        self.bs, self.h, self.w, self.device = bs, h, w, device
        self.buffers: Dict[str, Tuple[int, int, int]] = {}   # name -> (channels, h, w)
        self.steps: List[dict] = []
        self.arena = self.records = None
        self.heads: List[torch.Tensor] = []
        self.offsets: Dict[str, int] = {}                    # name -> first byte in the arena
        self.arena_bytes = 0
        self.input_rows: List[int] = []

    @property
    def launches(self) -> int:
        return len(self.steps)


class DetectorNet:
    """The network with its weights.  ``net(x)`` -> the nl heads, in one native call, with no host wait and -- after
    the first call for a shape -- no allocation: the heads are views of that shape's arena and are overwritten by the
    next call with the same shape (clone what must outlive it).

    state_dict: the reference's keys (``model.<i>...`` or ``<i>...``), fused or unfused (see ``fused_parameters``).
    dtype: torch.float32 (the default) or torch.float16.  The half network folds BatchNorm in float32 exactly as the
    float32 one, rounds every weight once to fp16 (the bias stays float32), takes a float16 ``x``, rounds every
    activation once per layer and returns float32 heads."""

    def __init__(self, spec: DetectorSpec, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.float32):
        if dtype not in (torch.float32, torch.float16):
            raise TypeError("DetectorNet: dtype must be torch.float32 or torch.float16 (got %s)" % (dtype,))
        self.dtype = dtype
        self.spec = spec
        self.params = fused_parameters(spec, state_dict)
        self.geometry = spec.geometry()
        self.stride = torch.tensor(spec.stride)
        self._packed: Dict[torch.device, List[torch.Tensor]] = {}
        self._plans: Dict[tuple, DetectorPlan] = {}

    @classmethod
    def from_module(cls, model, dtype: torch.dtype = torch.float32) -> "DetectorNet":
        return cls(DetectorSpec.from_module(model), model.state_dict(), dtype)

    # ---- planning ----
    def layout(self, bs: int, h: int, w: int, tile: Optional[int] = None) -> DetectorPlan:
        """The symbolic plan: buffers and steps, no device.  Each step is a dict with ``kind``, ``conv`` (index into
        ``spec.convs()``), ``src`` / ``dst`` / ``res`` / ``up`` as (buffer, c0, c) and the sizes."""
        spec = self.spec
        if h % spec.max_stride or w % spec.max_stride or h < 1 or w < 1:
            raise ValueError("DetectorNet: height and width must be positive multiples of the largest stride %d "
                             "(got %d x %d); the reference fails at Concat there" % (spec.max_stride, h, w))
        if bs < 1:
            raise ValueError("DetectorNet: bs must be positive")
        P = DetectorPlan(bs, h, w, None)
        n_layers = len(spec.layers)
        # shapes
        ch, size = [], []
        for i, L in enumerate(spec.layers):
            f0 = L["f"][0]
            c1, (h1, w1) = (spec.ch_in, (h, w)) if f0 < 0 else (ch[f0], size[f0])
            t = L["type"]
            if t == "Focus":
                ch.append(L["c2"]); size.append((out_size(h1 // 2, L["k"], L["s"]), out_size(w1 // 2, L["k"], L["s"])))
            elif t == "Conv":
                ch.append(L["c2"]); size.append((out_size(h1, L["k"], L["s"]), out_size(w1, L["k"], L["s"])))
            elif t in ("C3", "SPP"):
                ch.append(L["c2"]); size.append((h1, w1))
            elif t == "Upsample":
                ch.append(c1); size.append((2 * h1, 2 * w1))
            elif t == "Concat":
                if any(size[j] != size[f0] for j in L["f"]):
                    raise ValueError("DetectorNet: layer %d: Concat of planes %s" % (i, [size[j] for j in L["f"]]))
                ch.append(sum(ch[j] for j in L["f"])); size.append((h1, w1))
            else:
                ch.append(0); size.append((0, 0))
        # placement: Concat's inputs are written where the Concat's consumer reads them
        place: Dict[int, Tuple[str, int]] = {}
        up_target: Dict[int, Tuple[str, int, int]] = {}
        consumers: Dict[int, List[int]] = {}
        for i, L in enumerate(spec.layers):
            for j in L["f"]:
                consumers.setdefault(j, []).append(i)
        for i, L in enumerate(spec.layers):
            if L["type"] != "Concat":
                continue
            name = "cat%d" % i
            P.buffers[name] = (ch[i], size[i][0], size[i][1])
            off = 0
            for j in L["f"]:
                tj = spec.layers[j]["type"] if j >= 0 else "input"
                if tj in ("Concat", "input"):
                    raise ValueError("DetectorNet: layer %d: a Concat of %s is not supported" % (i, tj))
                if tj == "Upsample":
                    p = spec.layers[j]["f"][0]
                    if p in up_target or spec.layers[p]["type"] in ("Upsample", "Concat") or consumers[j] != [i]:
                        raise ValueError("DetectorNet: layer %d: an Upsample must follow a convolution and feed one "
                                         "Concat only" % j)
                    up_target[p] = (name, off, ch[i])
                else:
                    if j in place:
                        raise ValueError("DetectorNet: layer %d feeds two Concats, which is not supported" % j)
                    place[j] = (name, off)
                off += ch[j]
            place[i] = (name, 0)
        for i, L in enumerate(spec.layers):
            if L["type"] == "Upsample":
                if any(spec.layers[c]["type"] != "Concat" for c in consumers.get(i, [])) or i not in consumers:
                    raise ValueError("DetectorNet: layer %d: an Upsample must feed a Concat" % i)
            elif L["type"] != "Detect" and i not in place:
                P.buffers["L%d" % i] = (ch[i], size[i][0], size[i][1])
                place[i] = ("L%d" % i, 0)

        def view(j):   # (buffer, c0, c) of layer j's output; -1: the input
            if j < 0:
                return ("input", 0, spec.ch_in)
            return (place[j][0], place[j][1], ch[j])

        conv_index = {c["key"]: n for n, c in enumerate(spec.convs())}

        def conv(key, src, dst, hw_in, k=1, s=1, act=True, res=None, up=None, focus=False):
            lh, lw = (hw_in[0] // 2, hw_in[1] // 2) if focus else hw_in
            ho, wo = out_size(lh, k, s), out_size(lw, k, s)
            c_in = src[2] * (4 if focus else 1)
            P.steps.append(dict(kind="conv", conv=conv_index[key], key=key, src=src, dst=dst, res=res, up=up, k=k, s=s,
                                act=act, focus=focus, hw_in=hw_in, hw_out=(ho, wo), c_in=c_in, c_out=dst[2],
                                tile=choose_tile(dst[2], bs * ho * wo) if tile is None else tile))

        def temp(name, c, hw):
            P.buffers[name] = (c, hw[0], hw[1])
            return (name, 0, c)

        for i, L in enumerate(spec.layers):
            t = L["type"]
            if t in ("Upsample", "Concat"):
                continue
            f0 = L["f"][0]
            hw_in = (h, w) if f0 < 0 else size[f0]
            if t == "Detect":
                for l, j in enumerate(L["f"]):
                    dst = temp("head%d" % l, spec.na * spec.no, size[j])
                    conv("%d.m.%d" % (i, l), view(j), dst, size[j], act=False)
                continue
            src, dst = view(f0), view(i)
            up = None
            if i in up_target:
                b, off, _ = up_target[i]
                up = (b, off, ch[i])
            if t == "Focus":
                conv("%d.conv" % i, src, dst, hw_in, L["k"], L["s"], up=up, focus=True)
            elif t == "Conv":
                conv("%d" % i, src, dst, hw_in, L["k"], L["s"], up=up)
            elif t == "C3":
                c_, n = L["c_"], L["n"]
                cat = temp("c3cat%d" % i, 2 * c_, hw_in)[0]
                cur = (cat, 0, c_) if n == 0 else temp("c3t%d.x" % i, c_, hw_in)
                conv("%d.cv1" % i, src, cur, hw_in)
                conv("%d.cv2" % i, src, (cat, c_, c_), hw_in)
                for j in range(n):
                    hid = temp("c3t%d.%d.h" % (i, j), c_, hw_in)
                    nxt = (cat, 0, c_) if j == n - 1 else temp("c3t%d.%d.y" % (i, j), c_, hw_in)
                    conv("%d.m.%d.cv1" % (i, j), cur, hid, hw_in)
                    conv("%d.m.%d.cv2" % (i, j), hid, nxt, hw_in, 3, res=cur if L["shortcut"] else None)
                    cur = nxt
                conv("%d.cv3" % i, (cat, 0, 2 * c_), dst, hw_in, up=up)
            else:   # SPP
                c_ = L["c_"]
                cat = temp("sppcat%d" % i, 4 * c_, hw_in)[0]
                conv("%d.cv1" % i, src, (cat, 0, c_), hw_in)
                P.steps.append(dict(kind="pool", src=(cat, 0, c_), dst=(cat, c_, 3 * c_), res=None, up=None, hw_in=hw_in,
                                    hw_out=hw_in))
                conv("%d.cv2" % i, (cat, 0, 4 * c_), dst, hw_in, up=up)
        return P

    def packed(self, device) -> List[torch.Tensor]:
        device = _device(device)
        if device not in self._packed:
            pack = pack_weights_f16 if self.dtype == torch.float16 else pack_weights
            self._packed[device] = [pack(w.to(device), b.to(device)) for w, b in self.params]
        return self._packed[device]

    def arena_layout(self, P: DetectorPlan) -> Tuple[Dict[str, int], int]:
        """({buffer: first byte}, bytes) of the arena of a ``layout()``: every buffer 256-byte aligned, ``self.dtype``
        elements -- except, in the half network, the float32 head buffers.  Host only."""
        offsets, total = {}, 0
        for name, (c, bh, bw) in P.buffers.items():
            size = 4 if self.dtype == torch.float32 or name.startswith("head") else 2
            offsets[name] = total
            total += -(-(P.bs * c * bh * bw * size) // 256) * 256
        return offsets, total

    def records_of(self, P: DetectorPlan, offsets: Dict[str, int], base: int, packed: Sequence[int]) -> List[List[int]]:
        """The launch records of a ``layout()`` whose buffers start ``offsets`` bytes behind ``base``; packed: the
        address of every convolution's packed weights.  Rows of ``RECORD_FIELDS`` (float32) or ``RECORD_FIELDS_F16``
        (half: ``out_f32`` on the rows that write a head).  The input's address is left 0.  Host only."""
        bs, half = P.bs, self.dtype == torch.float16
        ptr = lambda name: 0 if name == "input" else base + offsets[name]
        ct = lambda name: self.spec.ch_in if name == "input" else P.buffers[name][0]
        rows = []
        for n, s in enumerate(P.steps):
            (sb, sc0, sc), (db, dc0, dc) = s["src"], s["dst"]
            if s["kind"] == "pool":
                rows.append((pool_record_f16 if half else pool_record)(
                    ptr(sb), sc0, ct(sb), ptr(db), dc0, ct(db), bs, sc, s["hw_in"][0], s["hw_in"][1]))
                continue
            res = None if s["res"] is None else (ptr(s["res"][0]), s["res"][1], ct(s["res"][0]))
            up = None if s["up"] is None else (ptr(s["up"][0]), s["up"][1], ct(s["up"][0]))
            kw = dict(out_f32=db.startswith("head")) if half else {}
            rows.append((conv_record_f16 if half else conv_record)(
                ptr(sb), sc0, ct(sb), s["hw_in"][0], s["hw_in"][1], ptr(db), dc0, ct(db), packed[s["conv"]],
                bs, s["c_in"], s["c_out"], s["k"], s["s"], s["act"], res=res, up=up, focus=s["focus"], tile=s["tile"],
                **kw))
        return rows

    def plan(self, bs: int, h: int, w: int, device="cuda", tile: Optional[int] = None) -> DetectorPlan:
        """The plan for inputs [bs, ch, h, w] on ``device``: built and allocated once, then cached.  tile: force one
        tile shape on every layer (TILE_128 / TILE_64; the tests) instead of the policy's choice."""
        device = _device(device)
        key = (int(bs), int(h), int(w), device, tile)
        if key in self._plans:
            return self._plans[key]
        P = self.layout(int(bs), int(h), int(w), tile)
        P.device = device
        packed = self.packed(device)
        half = self.dtype == torch.float16
        P.offsets, P.arena_bytes = self.arena_layout(P)
        if half:
            P.arena = torch.empty(P.arena_bytes, dtype=torch.uint8, device=device)
        else:
            P.arena = torch.empty(P.arena_bytes // 4, dtype=torch.float32, device=device)
        rows = self.records_of(P, P.offsets, P.arena.data_ptr(), [t.data_ptr() for t in packed])
        P.input_rows = [n for n, s in enumerate(P.steps) if s["src"][0] == "input"]
        P.records = torch.tensor(rows, dtype=torch.int64)
        for l in range(self.spec.nl):
            c, hh, ww = P.buffers["head%d" % l]
            o = P.offsets["head%d" % l]
            if half:
                P.heads.append(P.arena[o:o + 4 * bs * c * hh * ww].view(torch.float32).view(bs, c, hh, ww))
            else:
                P.heads.append(P.arena[o // 4:o // 4 + bs * c * hh * ww].view(bs, c, hh, ww))
        self._plans[key] = P
        return P

    # ---- calls ----
    def _check(self, x):
        if not isinstance(x, torch.Tensor):
            raise TypeError("DetectorNet: x must be a tensor (got %s)" % type(x).__name__)
        if self.dtype == torch.float16 and x.dtype != torch.float16:
            raise TypeError("DetectorNet: x must be float16 (got %s) for a dtype=torch.float16 network: no hidden cast; "
                            "detector_input(..., dtype=torch.float16) makes it" % (x.dtype,))
        if self.dtype == torch.float32 and x.dtype != torch.float32:
            raise TypeError("DetectorNet: x must be float32 (got %s); the network is the FP32 model the reference loads, "
                            "a half-precision run is a different contract" % (x.dtype,))
        if x.dim() != 4 or x.shape[1] != self.spec.ch_in:
            raise ValueError("DetectorNet: x must be [bs, %d, h, w] (got %s)" % (self.spec.ch_in, list(x.shape)))
        if x.shape[2] % self.spec.max_stride or x.shape[3] % self.spec.max_stride:
            raise ValueError("DetectorNet: height and width must be multiples of the largest stride %d (got %d x %d); the "
                             "reference fails at Concat there" % (self.spec.max_stride, x.shape[2], x.shape[3]))
        if not x.is_contiguous():
            raise ValueError("DetectorNet: x must be contiguous NCHW (a copy would hide its cost)")
        if not x.is_cuda:
            raise ValueError("DetectorNet: x is on %s; it must live on a ROCm/HIP device (torch device 'cuda'): this "
                             "network has no CPU path" % x.device)

    def __call__(self, x: torch.Tensor, tile: Optional[int] = None) -> List[torch.Tensor]:
        self._check(x)
        P = self.plan(x.shape[0], x.shape[2], x.shape[3], x.device, tile)
        for n in P.input_rows:
            P.records[n, 1] = x.data_ptr()
        (_C().detector_run_f16 if self.dtype == torch.float16 else _C().detector_run)(P.records, P.arena)
        return P.heads

    def detections(self, x: torch.Tensor, conf_thres: float = 0.25, iou_thres: float = 0.45,
                   classes: Optional[Sequence[int]] = None, agnostic: bool = False, max_det: int = 300, *,
                   max_nms: int = MAX_NMS, plan: Optional[LetterboxPlan] = None, out=None):
        """``detections_from_heads(net(x), net.geometry, ...)``: the frame's ``(det, count)`` on the device."""
        return detections_from_heads(self(x), self.geometry, conf_thres, iou_thres, classes, agnostic, max_det,
                                     max_nms=max_nms, plan=plan, out=out)


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device
