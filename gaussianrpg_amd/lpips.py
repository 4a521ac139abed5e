"""LPIPS on the device: the reference's third quality number (``metrics.py:81``, ``lpips(render, gt, net_type='alex')``
over ``lib/utils/lpipsPyTorch/modules/{lpips,networks,utils}.py``) with the AlexNet or the VGG16 backbone, as ONE native
call per batch of pairs (csrc/lpips.hip).

    features = torchvision.models.alexnet(weights=...).features.state_dict()     # the user's to provide
    lin = torch.load("alex.pth")                                                 # the LPIPS v0.1 weight file
    criterion = LPIPS("alex", features, lin)
    value = criterion(render, gt)                  # [1, 1, 1, 1], the reference's contract
    per_pair = criterion.distances(x, y)           # [B]
    psnr_ssim_lpips = image_metrics(render, gt, criterion)   # device [3], no host wait

The backbone comes from ``torchvision`` in the reference; here it is two tables (``LAYERS``) and the caller's state
dict, so neither torchvision nor a download is needed.  Inputs are used as given: ``metrics.py`` passes [0, 1] images
into a z-score made for [-1, 1], and so does this.  No CPU path, no SqueezeNet, no half precision.

As a training term (csrc/lpips_bwd.hip): ``criterion.loss(x, y)`` is [B] with a gradient to ``x``
-- and to ``x`` only -- through one native backward call; ``lpips_loss(x, y, criterion, reduction)`` reduces it.  Every
other entry point stays a detached metric.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

NETS = {"alex": 0, "vgg": 1}          # GRPG_LPIPS_ALEX, GRPG_LPIPS_VGG16
TILE_128, TILE_64 = 0, 1              # GRPG_LPIPS_TILE_*
MEAN = (-.030, -.088, -.188)          # BaseNet's buffers (networks.py:41-44)
STD = (.458, .448, .450)
EPS = 1e-10                           # normalize_activation (utils.py:6)
MIN_SIZE = {"alex": 31, "vgg": 16}


def distance_px(c: int) -> int:
    """Pixels per workgroup of the distance kernel (csrc/lpips.hip): one partial sum each."""
    return 32 if c <= 192 else 16 if c <= 384 else 8


def _vgg16_layers():
    out, c = [], 3
    for stage, (width, depth) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))):
        for _ in range(depth):
            out += [("conv", c, width, 3, 1, 1), ("relu",)]
            c = width
        out.append(("pool", 2, 2))
    return tuple(out)


# torchvision's ``features`` stacks, module by module: ("conv", c_in, c_out, k, stride, pad), ("relu",), ("pool", k, stride)
LAYERS = {
    "alex": (("conv", 3, 64, 11, 4, 2), ("relu",), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2), ("relu",), ("pool", 3, 2),
             ("conv", 192, 384, 3, 1, 1), ("relu",), ("conv", 384, 256, 3, 1, 1), ("relu",), ("conv", 256, 256, 3, 1, 1),
             ("relu",), ("pool", 3, 2)),
    "vgg": _vgg16_layers(),
}
# the taps, counted from 1 as BaseNet.forward counts (networks.py:57-63, 82, 93): each is a ReLU's output
TARGETS = {"alex": (2, 5, 8, 10, 12), "vgg": (4, 9, 16, 23, 30)}
CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}


def _net(net_type: str) -> str:
    if net_type == "squeeze":
        raise ValueError("gaussianrpg_amd.lpips: net_type 'squeeze' is not supported (Fire modules and ceil-mode pools); "
                         "choose 'alex' or 'vgg'")
    if net_type not in NETS:
        raise ValueError("gaussianrpg_amd.lpips: choose net_type from ['alex', 'vgg'] (got %r)" % (net_type,))
    return net_type


def conv_indices(net_type: str) -> List[int]:
    """The positions of the convolutions in ``features``: the numbers in the state dict's keys."""
    return [i for i, L in enumerate(LAYERS[_net(net_type)]) if L[0] == "conv"]


def out_size(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def _align256(v: int) -> int:
    return -(-v // 256) * 256


def shape_plan(net_type: str, pairs: int, h: int, w: int) -> dict:
    """What one call does, on the host: ``steps`` (one dict per launch up to the fifth tap: kind "conv" / "pool", the
    sizes, ``tap`` on a convolution whose ReLU output is a tap), ``taps`` [(C, H, W)], and the workspace arithmetic of
    csrc/lpips.hip: ``act_bytes`` (ONE of the two ping-pong activations), ``map_offsets`` / ``slot_offsets`` (bytes) and
    ``workspace_bytes``; ``launches`` of the forward and ``backward_launches`` of ``LPIPS.loss``'s backward (one per
    convolution, pool and tap).  Raises ValueError for a size the native call refuses."""
    net_type = _net(net_type)
    least = MIN_SIZE[net_type]
    if pairs < 1 or pairs > 65535:
        raise ValueError("gaussianrpg_amd.lpips: pairs must be in 1 .. 65535 (got %d)" % pairs)
    if h < least or w < least:
        raise ValueError("gaussianrpg_amd.lpips: a %d x %d image is too small for net_type %r: at least %d x %d (the "
                         "reference fails in a pool there)" % (h, w, net_type, least, least))
    steps, taps = [], []
    c, ch, cw = 3, h, w
    last = TARGETS[net_type][-1]
    for i, L in enumerate(LAYERS[net_type][:last], 1):
        if L[0] == "conv":
            _, c_in, c_out, k, s, p = L
            ho, wo = out_size(ch, k, s, p), out_size(cw, k, s, p)
            steps.append(dict(kind="conv", index=i - 1, c_in=c_in, c_out=c_out, k=k, stride=s, pad=p, hw_in=(ch, cw),
                              hw_out=(ho, wo), tap=None))
            c = c_out
        elif L[0] == "pool":
            _, k, s = L
            ho, wo = out_size(ch, k, s, 0), out_size(cw, k, s, 0)
            steps.append(dict(kind="pool", index=i - 1, c_in=c, c_out=c, k=k, stride=s, pad=0, hw_in=(ch, cw),
                              hw_out=(ho, wo), tap=None))
        else:
            if i in TARGETS[net_type]:
                steps[-1]["tap"] = len(taps)
                taps.append((c, ch, cw))
            continue
        if ho < 1 or wo < 1:
            raise ValueError("gaussianrpg_amd.lpips: a %d x %d image is too small for net_type %r" % (h, w, net_type))
        if 2 * pairs * ho * wo >= 2 ** 31 - 256:
            raise ValueError("gaussianrpg_amd.lpips: %d pairs of %d x %d give a layer of 2^31 pixels or more" % (pairs, h, w))
        ch, cw = ho, wo
    most = max(2 * pairs * s["c_out"] * s["hw_out"][0] * s["hw_out"][1] for s in steps)
    act = _align256(4 * most)
    off = 2 * act
    map_offsets, slot_offsets = [], []
    for _, th, tw in taps:
        map_offsets.append(off)
        off += _align256(4 * pairs * th * tw)
    for tc, th, tw in taps:
        slot_offsets.append(off)
        off += _align256(4 * pairs * -(-(th * tw) // distance_px(tc)))
    convs, pools = sum(s["kind"] == "conv" for s in steps), sum(s["kind"] == "pool" for s in steps)
    return dict(net_type=net_type, pairs=pairs, h=h, w=w, steps=steps, taps=taps, act_bytes=act, map_offsets=map_offsets,
                slot_offsets=slot_offsets, workspace_bytes=off,
                launches=dict(conv=convs, pool=pools, distance=len(taps), finish=1, total=convs + pools + len(taps) + 1),
                backward_launches=dict(conv=convs, pool=pools, distance=len(taps), total=convs + pools + len(taps)))


# ---- the two state dicts ----

def _host_f32(t, name) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError("gaussianrpg_amd.lpips: %s must be a torch.Tensor (got %s)" % (name, type(t).__name__))
    if not t.dtype.is_floating_point:
        raise TypeError("gaussianrpg_amd.lpips: %s must be a floating-point tensor (got %s)" % (name, t.dtype))
    return t.detach().to("cpu", torch.float32).contiguous()


def feature_parameters(net_type: str, features: Dict[str, torch.Tensor]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """[(weight, bias)] of the convolutions up to the fifth tap, float32 on the host, from the state dict of
    torchvision's ``alexnet().features`` / ``vgg16().features`` (keys ``0.weight`` ...) or of the whole model (keys
    ``features.0.weight`` ...)."""
    net_type = _net(net_type)
    out = []
    for i in conv_indices(net_type):
        _, c_in, c_out, k, _, _ = LAYERS[net_type][i]
        got = []
        for leaf, want in (("weight", (c_out, c_in, k, k)), ("bias", (c_out,))):
            for key in ("%d.%s" % (i, leaf), "features.%d.%s" % (i, leaf)):
                if key in features:
                    break
            else:
                raise KeyError("gaussianrpg_amd.lpips: the features state dict has neither '%d.%s' nor 'features.%d.%s'"
                               % (i, leaf, i, leaf))
            t = _host_f32(features[key], key)
            if tuple(t.shape) != want:
                raise ValueError("gaussianrpg_amd.lpips: '%s' has shape %s, net_type %r needs %s"
                                 % (key, list(t.shape), net_type, list(want)))
            got.append(t)
        out.append(tuple(got))
    return out


def lin_parameters(net_type: str, lin: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
    """The five [C_l] weight vectors of ``LinLayers``, float32 on the host, from the official weight file's keys
    (``lin0.model.1.weight`` ...) or the renamed ones ``get_state_dict`` produces (``0.1.weight`` ...); each tensor is
    [1, C_l, 1, 1]."""
    net_type = _net(net_type)
    out = []
    for l, c in enumerate(CHANNELS[net_type]):
        for key in ("lin%d.model.1.weight" % l, "%d.1.weight" % l):
            if key in lin:
                break
        else:
            raise KeyError("gaussianrpg_amd.lpips: the lin state dict has neither 'lin%d.model.1.weight' nor '%d.1.weight'"
                           % (l, l))
        t = _host_f32(lin[key], key)
        if tuple(t.shape) != (1, c, 1, 1):
            raise ValueError("gaussianrpg_amd.lpips: '%s' has shape %s, tap %d of net_type %r has %d channels: [1, %d, 1, 1]"
                             % (key, list(t.shape), l, net_type, c, c))
        out.append(t.reshape(c).contiguous())
    return out


# ---- the native leaves ----

def _C():
    from .rasterizer import _C as ext
    return ext


def pack_weights(weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [c_out, c_in, k, k] (+ [c_out] bias) on the device, k in {3, 5, 11} -> the buffer the convolution
    streams: one launch."""
    if bias is None:
        bias = torch.zeros(weight.shape[0], dtype=weight.dtype, device=weight.device)
    return _C().lpips_pack_weights(weight.contiguous(), bias.contiguous())


def conv2d_relu(x: torch.Tensor, packed: torch.Tensor, c_out: int, k: int, stride: int = 1, pad: int = 0,
                zscore: bool = False, tile: int = TILE_64) -> torch.Tensor:
    """ONE launch of the convolution kernel: relu(bias + conv(x)), with BaseNet's z-score in the gather if asked."""
    return _C().lpips_conv2d(x, packed, int(c_out), int(k), int(stride), int(pad), list(MEAN + STD) if zscore else [],
                             int(tile))


def max_pool(x: torch.Tensor, k: int) -> torch.Tensor:
    """``F.max_pool2d(x, k, 2)`` for k in {2, 3}: one launch."""
    return _C().lpips_max_pool(x, int(k))


def pack_weights_bwd(weight: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """float32 [c_out, c_in, k, k] on the device -> the layout the backward-data kernel streams: k in {3, 5} at stride
    1, or k 11 at stride 4 with c_in <= 4; one launch, once per model."""
    return _C().lpips_bwd_pack_weights(weight.contiguous(), int(stride))


def conv2d_backward_data(grad_out: torch.Tensor, packed_bwd: torch.Tensor, c_in: int, hw_in: Tuple[int, int], k: int,
                         stride: int = 1, pad: int = 0, act: Optional[torch.Tensor] = None,
                         tap: Optional[torch.Tensor] = None, std: bool = False, tile: int = TILE_64) -> torch.Tensor:
    """ONE launch of the backward-data kernel: the gradient of a convolution's input from its pre-activation's;
    ``act`` (the ReLU output the gradient lands on) switches the select ``act > 0 ? g + tap : 0`` on, ``std`` the
    division by BaseNet's std (the image's gradient)."""
    return _C().lpips_conv2d_backward_data(grad_out, packed_bwd, act, tap, int(c_in), int(hw_in[0]), int(hw_in[1]), int(k),
                                           int(stride), int(pad), list(STD) if std else [], int(tile))


def max_pool_backward(act: torch.Tensor, grad_out: torch.Tensor, k: int, tap: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``MaxPool2d(k, 2)`` backward onto its input ``act`` (a ReLU output): ``act > 0 ? gathered + tap : 0``; one launch."""
    return _C().lpips_max_pool_backward(act, grad_out, tap, int(k))


def tap_distance_backward(feat: torch.Tensor, lin: torch.Tensor, grad_pairs: torch.Tensor) -> torch.Tensor:
    """One tap's gradient to the x half of ``feat`` [2 * pairs, C, H, W]: [pairs, C, H, W], 0 where x is not positive."""
    return _C().lpips_distance_backward(feat, lin, grad_pairs)


def tap_distance(feat: torch.Tensor, lin: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """One tap: feat [2 * pairs, C, H, W] (x's features first, then y's), lin [C] -> (the tap's term per pair [pairs],
    the per-pixel map s [pairs, H, W])."""
    return _C().lpips_distance(feat, lin)


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class LPIPS(nn.Module):
    """The criterion.  ``criterion(x, y)`` is the reference's ``LPIPS.forward``: [1, 1, 1, 1], for a batch the sum over
    it (lpips.py:36).  One native call, no host wait and -- after a shape's first call -- no allocation inside
    ``distances`` / ``tap_terms``: their results are views of that shape's buffers and are overwritten by the next call
    with the same shape (clone what must outlive it).

    features: state dict of torchvision's ``alexnet().features`` / ``vgg16().features`` (or of the whole model).
    lin: the LPIPS v0.1 weight file's state dict, original or renamed keys.  Both are the user's to provide.
    device: where the weights are packed in ``__init__``; default: the current ROCm device if there is one (without
    one the module can still be built -- and fails at the first call, there being no CPU path)."""

    def __init__(self, net_type: str = "alex", features: Optional[Dict[str, torch.Tensor]] = None,
                 lin: Optional[Dict[str, torch.Tensor]] = None, device=None):
        super().__init__()
        self.net_type = _net(net_type)
        if features is None or lin is None:
            raise ValueError("gaussianrpg_amd.lpips: LPIPS needs the backbone's `features` state dict and the `lin` "
                             "state dict; the package ships no weights and downloads none")
        self.params = feature_parameters(self.net_type, features)
        self.lin = lin_parameters(self.net_type, lin)
        self._packed: Dict[torch.device, tuple] = {}
        self._packed_bwd: Dict[torch.device, list] = {}
        self._buffers_of: Dict[tuple, tuple] = {}
        self._train_of: Dict[tuple, list] = {}
        if device is not None or torch.cuda.is_available():
            self.packed(device if device is not None else "cuda")

    def packed(self, device) -> tuple:
        """([packed convolution], [lin vector]) on ``device``: repacked once per device."""
        device = _device(device)
        if device not in self._packed:
            self._packed[device] = ([pack_weights(w.to(device), b.to(device)) for w, b in self.params],
                                    [v.to(device) for v in self.lin])
        return self._packed[device]

    def packed_bwd(self, device) -> list:
        """[the backward layout of every convolution's weights] on ``device``: repacked once per device."""
        device = _device(device)
        if device not in self._packed_bwd:
            strides = [LAYERS[self.net_type][i][4] for i in conv_indices(self.net_type)]
            self._packed_bwd[device] = [pack_weights_bwd(w.to(device), s) for (w, _), s in zip(self.params, strides)]
        return self._packed_bwd[device]

    def _check(self, x, y):
        for t, n in ((x, "x"), (y, "y")):
            if not isinstance(t, torch.Tensor):
                raise TypeError("gaussianrpg_amd.lpips: %s must be a torch.Tensor (got %s)" % (n, type(t).__name__))
            if t.dtype != torch.float32:
                raise TypeError("gaussianrpg_amd.lpips: %s must be float32 (got %s): no hidden cast" % (n, t.dtype))
        if x.shape != y.shape:
            raise ValueError("gaussianrpg_amd.lpips: x and y must have the same shape (got %s and %s)"
                             % (list(x.shape), list(y.shape)))
        if x.dim() not in (3, 4) or x.shape[-3] != 3 or x.numel() == 0:
            raise ValueError("gaussianrpg_amd.lpips: images must be [3, H, W] or [B, 3, H, W] (got %s)" % (list(x.shape),))
        plan = shape_plan(self.net_type, 1 if x.dim() == 3 else int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1]))
        for t, n in ((x, "x"), (y, "y")):
            if not t.is_contiguous():
                raise ValueError("gaussianrpg_amd.lpips: %s must be contiguous (a copy would hide its cost)" % n)
            if not t.is_cuda:
                raise ValueError("gaussianrpg_amd.lpips: %s is on %s; it must live on a ROCm/HIP device (torch device "
                                 "'cuda'): LPIPS has no CPU path" % (n, t.device))
        if x.device != y.device:
            raise ValueError("gaussianrpg_amd.lpips: x on %s, y on %s" % (x.device, y.device))
        return plan

    def _run(self, x, y):
        plan = self._check(x, y)
        key = (plan["pairs"], plan["h"], plan["w"], x.device)
        if key not in self._buffers_of:
            self._buffers_of[key] = (torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=x.device),
                                     torch.empty(plan["pairs"], dtype=torch.float32, device=x.device),
                                     torch.empty(plan["pairs"], 5, dtype=torch.float32, device=x.device))
        ws, out, taps = self._buffers_of[key]
        packed, lin = self.packed(x.device)
        shape = (plan["pairs"], 3, plan["h"], plan["w"])
        with torch.no_grad():
            _C().lpips_forward(NETS[self.net_type], packed, lin, x.detach().view(shape), y.detach().view(shape), ws, out, taps)
        return plan, ws, out, taps

    def distances(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """[B]: the value of every pair.  Detached: no gradient is provided."""
        return self._run(x, y)[2]

    def tap_terms(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """[B, 5]: every pair's five tap terms; a pair's value is their sum in tap order."""
        return self._run(x, y)[3]

    def tap_maps(self, x: torch.Tensor, y: torch.Tensor) -> List[torch.Tensor]:
        """The five per-pixel maps s [B, H_l, W_l] (copies), for the tests and tools/lpips_parity.py: the call's
        partial results, read out of its workspace."""
        plan, ws, _, _ = self._run(x, y)
        maps = []
        for (c, th, tw), off in zip(plan["taps"], plan["map_offsets"]):
            n = plan["pairs"] * th * tw
            maps.append(ws[off:off + 4 * n].view(torch.float32).view(plan["pairs"], th, tw).clone())
        return maps

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return self.distances(x, y).sum().reshape(1, 1, 1, 1)

    # ---- the training term ----

    def _run_train(self, x, y):
        """The forward that keeps its activations: (plan, key, state) with state = [workspace, out, taps, generation,
        grad_pairs buffer] of the shape; every call raises the generation, so a backward can tell that its activations
        are gone."""
        plan = self._check(x, y)
        key = (plan["pairs"], plan["h"], plan["w"], x.device)
        if key not in self._train_of:
            nbytes = _C().lpips_train_workspace_bytes(NETS[self.net_type], plan["pairs"], plan["h"], plan["w"])
            self._train_of[key] = [torch.empty(nbytes, dtype=torch.uint8, device=x.device),
                                   torch.empty(plan["pairs"], dtype=torch.float32, device=x.device),
                                   torch.empty(plan["pairs"], 5, dtype=torch.float32, device=x.device), 0,
                                   torch.empty(plan["pairs"], dtype=torch.float32, device=x.device)]
            self.packed_bwd(x.device)
        state = self._train_of[key]
        packed, lin = self.packed(x.device)
        shape = (plan["pairs"], 3, plan["h"], plan["w"])
        state[3] += 1
        with torch.no_grad():
            _C().lpips_forward_train(NETS[self.net_type], packed, lin, x.detach().view(shape), y.detach().view(shape),
                                     state[0], state[1], state[2])
        return plan, key, state

    def loss(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """[B]: ``distances(x, y)`` bit for bit, as a fresh tensor with a gradient to ``x`` (one native backward call;
        no host wait, and after a shape's first forward + backward no allocation but the returned tensors).  The
        gradient goes to ``x`` only: a ``y`` that requires grad is refused.  The activations live in the shape's
        workspace until the next ``loss`` / ``train_activations`` call of that shape: call backward before it."""
        if isinstance(y, torch.Tensor) and y.requires_grad:
            raise ValueError("gaussianrpg_amd.lpips: y requires grad, but the gradient goes to x only; pass y.detach()")
        return _LpipsLoss.apply(x, y, self)

    def train_activations(self, x: torch.Tensor, y: torch.Tensor) -> List[torch.Tensor]:
        """The kept post-ReLU activations of the x images [B, C_i, H_i, W_i] (copies), one per convolution, for the
        tests and tools/lpips_bwd_parity.py: what the backward's selects and pool winners are decided by."""
        plan, _, state = self._run_train(x, y)
        acts = []
        for i, s in enumerate(s for s in plan["steps"] if s["kind"] == "conv"):
            off = _C().lpips_train_activation_offset(NETS[self.net_type], plan["pairs"], plan["h"], plan["w"], i)
            n = plan["pairs"] * s["c_out"] * s["hw_out"][0] * s["hw_out"][1]
            acts.append(state[0][off:off + 4 * n].view(torch.float32).view(plan["pairs"], s["c_out"], *s["hw_out"]).clone())
        return acts


class _LpipsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, crit):
        plan, key, state = crit._run_train(x, y)
        ctx.crit, ctx.key, ctx.generation, ctx.x_shape = crit, key, state[3], x.shape
        ctx.save_for_backward(state[1])            # torch's own guard against a second backward through the graph
        ctx.set_materialize_grads(False)
        return state[1].clone()

    @staticmethod
    def backward(ctx, grad):
        ctx.saved_tensors                          # raises once the graph's buffers are freed
        if grad is None or not ctx.needs_input_grad[0]:
            return None, None, None
        crit, key = ctx.crit, ctx.key
        state = crit._train_of[key]
        if state[3] != ctx.generation:
            raise RuntimeError("gaussianrpg_amd.lpips: the activations of this loss were overwritten by a later loss / "
                               "train_activations call of the same shape; call backward before it")
        if grad.dtype != torch.float32 or not grad.is_cuda:
            raise TypeError("gaussianrpg_amd.lpips: the incoming gradient must be a float32 device tensor")
        pairs, h, w, device = key
        grad_x = torch.empty((pairs, 3, h, w), dtype=torch.float32, device=device)
        if not grad.is_contiguous():               # e.g. sum()'s expanded scalar: into the shape's own buffer
            grad = state[4].copy_(grad)
        _C().lpips_backward(NETS[crit.net_type], crit.packed_bwd(device), crit.packed(device)[1], state[0], grad, grad_x)
        return grad_x.view(ctx.x_shape), None, None


def lpips_loss(x: torch.Tensor, y: torch.Tensor, criterion: LPIPS, reduction: str = "mean") -> torch.Tensor:
    """The training term: ``criterion.loss(x, y)`` reduced over the pairs ('mean', 'sum') or as it is ('none')."""
    if not isinstance(criterion, LPIPS):
        raise TypeError("gaussianrpg_amd.lpips: criterion must be a gaussianrpg_amd.lpips.LPIPS (got %s); build it once "
                        "from the two state dicts" % type(criterion).__name__)
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("gaussianrpg_amd.lpips: reduction must be 'mean', 'sum' or 'none' (got %r)" % (reduction,))
    d = criterion.loss(x, y)
    return d.mean() if reduction == "mean" else d.sum() if reduction == "sum" else d


def lpips(x: torch.Tensor, y: torch.Tensor, criterion: LPIPS) -> torch.Tensor:
    """The functional form.  The reference's ``lpips(x, y, net_type)`` builds (and downloads) a criterion per call; here
    the caller builds it once and passes it."""
    if not isinstance(criterion, LPIPS):
        raise TypeError("gaussianrpg_amd.lpips: criterion must be a gaussianrpg_amd.lpips.LPIPS (got %s); build it once "
                        "from the two state dicts" % type(criterion).__name__)
    return criterion(x, y)


def image_metrics(render: torch.Tensor, gt: torch.Tensor, criterion: LPIPS) -> torch.Tensor:
    """``metrics.py:79-81`` in one call: a device [3] tensor (PSNR, SSIM, LPIPS) of one [3, H, W] view, with no host
    wait; equal bit for bit to ``loss.psnr``, ``loss.ssim`` and ``criterion.distances``."""
    from . import loss
    if not isinstance(criterion, LPIPS):
        raise TypeError("gaussianrpg_amd.lpips: criterion must be a gaussianrpg_amd.lpips.LPIPS")
    if not isinstance(render, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise TypeError("gaussianrpg_amd.lpips: render and gt must be torch.Tensors")
    if render.dim() != 3:
        raise ValueError("gaussianrpg_amd.lpips: image_metrics takes one [3, H, W] view (got %s)" % (list(render.shape),))
    d = criterion.distances(render, gt)
    return torch.stack((loss.psnr(render, gt), loss.ssim(render, gt).detach(), d[0]))
