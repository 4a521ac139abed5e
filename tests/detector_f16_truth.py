"""Builders, truths and error bounds of the detector's network in fp16 (gaussianrpg_amd/detector.py with
``dtype=torch.float16``, csrc/detector_f16.hip), for tests/test_detector_f16_host.py, tests/test_gpu_detector_f16.py and
tests/golden/make_golden_detector_f16.py.  Everything float64 comes from tests/detector_truth.py (``T``).

The contract of a convolution that feeds another layer: float32 bias + float32 accumulation of the exact fp16 x fp16
products; SiLU in float32; the residual (an fp16 value) added in float32 after the activation; ONE rounding to fp16, to
nearest even.  Detect's convolutions store the float32 value unrounded.

Inputs.  ``rep16`` makes x, w and res fp16-representable (``v.half()``) and free of fp16 subnormals (0 < |v| < 2^-14
becomes 0): how the f16 matrix instruction treats subnormal operands is not pinned, so the tests keep them out.  The bias
stays float32.  On such inputs the weight's rounding and the input's are no part of the error: the float64 truth
``T.conv64`` runs on the very values the kernel reads.

Error bound (u = 2^-24, T.U; first order in u, as in T's docstring)
--------------------------------------------------------------------
before the activation.  An 11-bit by 11-bit product is exact in float32, so the only roundings are the accumulator's.
The kernel adds one 16-deep instruction per 16 k onto the accumulator, which started at the bias: a product passes
through at most ceil(K / 16) roundings between instructions plus at most 16 inside its own instruction, however the
hardware orders those -- at most K + 18 for every K >= 1 (K = 1: 1 + 16 = 17).  With S = |b| + sum_k |w_k x_k|:
|err_pre| <= E' = (K + 18) u S, which is T.conv64's E = (K + 2) u S plus 16 u S.

SiLU and residual: as T derives them -- |err_y| <= 1.1 E' + 5u |y| with an activation, E' without; the residual adds
u |r + y|.  Together ``bound'`` = T.conv64's bound + (1.1 or 1) * 16 u S.

the output rounding.  One rounding to nearest of a value within bound' of y: at most half an fp16 ulp of the rounded
value, 2^-11 |y| to first order for a normal result, and 2^-25 -- half the spacing 2^-24 of the fp16 subnormals -- for
a result below 2^-14:  bound_f16 = bound' + 2^-11 |y| + 2^-25.
A float32 output (``out_f32``, Detect's heads) is not rounded: bound_f16 = bound'.

pool, Focus gather, upsample, every concat placement: data movement on fp16 values, exact -- compared bit for bit.
"""
import numpy as np
import torch
import torch.nn.functional as F

import detector_truth as T

TINY = 2.0 ** -14          # the smallest normal fp16
U16 = 2.0 ** -11           # the unit roundoff of fp16


def rep16(v):
    """float32 array -> the nearest fp16 value as float32, fp16 subnormals set to 0.  None stays None."""
    if v is None:
        return None
    t = torch.as_tensor(np.asarray(v, dtype=np.float32)).half().float()
    t = torch.where((t != 0) & (t.abs() < TINY), torch.zeros_like(t), t)
    return t.numpy()


def leaf_case(seed, bs, c_in, c_out, k, hw, focus=False):
    """(x, w, b, rs) as test_gpu_detector._case builds them, x and w passed through ``rep16``; b stays float32."""
    rs = np.random.RandomState(seed)
    cx = c_in // 4 if focus else c_in
    x = rs.normal(0, 1, (bs, cx, hw[0], hw[1])).astype(np.float32)
    w = (rs.normal(0, 1, (c_out, c_in, k, k)) / np.sqrt(c_in * k * k)).astype(np.float32)
    b = rs.normal(0, 1, c_out).astype(np.float32)
    return rep16(x), rep16(w), b, rs


def conv64_f16(x, w, b, k, s, act=True, res=None, focus=False, out_f32=False):
    """(out, bound_f16): ``T.conv64`` on fp16-representable x, w, res (asserted) and the bound of the module docstring."""
    for name, v in (("x", x), ("w", w), ("res", res)):
        assert v is None or np.array_equal(rep16(v), np.asarray(v, dtype=np.float32)), name + " is not what rep16 gives"
    y, bound = T.conv64(x, w, b, k, s, act, res, focus)
    xa = T.t64(x)
    if focus:
        xa = T.focus64(xa)
    S = F.conv2d(xa.abs(), T.t64(w).abs(), T.t64(b).abs(), stride=s, padding=k // 2)
    bound = bound + (1.1 if act else 1.0) * 16 * T.U * S
    if not out_f32:
        bound = bound + U16 * y.abs() + 2.0 ** -25
    return y, bound


def round16(v, variant=None):
    """float32 tensor -> fp16 to nearest even (``Tensor.half()``); variant "round_to_zero": the planted error."""
    h = v.half()
    if variant == "round_to_zero":
        up = h.float().abs() > v.abs()                           # rounded away from zero: step one fp16 back
        bits = h.view(torch.int16)
        h = torch.where(up, bits - 1, bits).view(torch.float16)  # sign-magnitude: -1 on the bits shrinks |h|
    return h


def conv_f16_restated(x, w, b, k, s, act=True, res=None, focus=False, out_f32=False, variant=None):
    """The contract of one convolution restated with CPU torch in float32: ``F.conv2d`` on fp16-valued float32 tensors
    with a float32 bias, SiLU in float32, + res, one rounding.  Returns float32 (out_f32) or float16.  variant: one
    planted contract error -- "res_before_act", "bias_f16", "round_to_zero"."""
    x, w, b = (torch.as_tensor(np.asarray(v, dtype=np.float32)) for v in (x, w, b))
    if focus:
        x = T.focus64(x)
    if variant == "bias_f16":
        b = b.half().float()
    y = F.conv2d(x, w, b, stride=s, padding=k // 2)
    r = None if res is None else torch.as_tensor(np.asarray(res, dtype=np.float32))
    if variant == "res_before_act" and r is not None:
        y, r = y + r, None
    if act:
        y = y * (1.0 / (1.0 + torch.exp(-y)))
    if r is not None:
        y = r + y
    return y if out_f32 else round16(y, variant)


def fused_f16(spec, state_dict):
    """[(weight, bias)] of the half network on the host: BatchNorm folded in float32 (``fused_parameters``), the weight
    rounded once to fp16 and given back as float32, the bias float32."""
    from gaussianrpg_amd.detector import fused_parameters
    return [(w.half().float(), b) for w, b in fused_parameters(spec, state_dict)]


def network_f16(spec, state_dict, x):
    """(heads, layers): the contract of the whole half network on the CPU.  x: fp16-valued.  Every convolution is a
    float32 ``F.conv2d`` on fp16-valued tensors, rounded ONCE per layer behind activation and residual; the heads stay
    float32.  The summation order is CPU torch's, not the kernel's: rounding ties may fall differently, so the GPU
    test records its distance from this and asserts none."""
    params = {c["key"]: p for c, p in zip(spec.convs(), fused_f16(spec, state_dict))}

    def conv(key, v, k=1, s=1, act=True, res=None, out_f32=False):
        w, b = params[key]
        y = F.conv2d(v.float(), w, b, stride=s, padding=k // 2)
        if act:
            y = y * (1.0 / (1.0 + torch.exp(-y)))
        if res is not None:
            y = res.float() + y
        return y if out_f32 else y.half()

    with torch.no_grad():
        x = torch.as_tensor(x).half()
        ys, heads = [], None
        for i, L in enumerate(spec.layers):
            ins = [x if j < 0 else ys[j] for j in L["f"]]
            t, v = L["type"], ins[0]
            if t == "Focus":
                y = conv("%d.conv" % i, T.focus64(v), L["k"], L["s"])
            elif t == "Conv":
                y = conv("%d" % i, v, L["k"], L["s"])
            elif t == "C3":
                m = conv("%d.cv1" % i, v)
                for j in range(L["n"]):
                    hid = conv("%d.m.%d.cv1" % (i, j), m)
                    m = conv("%d.m.%d.cv2" % (i, j), hid, 3, res=m if L["shortcut"] else None)
                y = conv("%d.cv3" % i, torch.cat((m, conv("%d.cv2" % i, v)), 1))
            elif t == "SPP":
                v = conv("%d.cv1" % i, v)
                y = conv("%d.cv2" % i, torch.cat((v, T.pool64(v.float()).half()), 1))
            elif t == "Upsample":
                y = T.upsample64(v)
            elif t == "Concat":
                y = torch.cat(ins, 1)
            else:
                heads = [conv("%d.m.%d" % (i, l), h, act=False, out_f32=True) for l, h in enumerate(ins)]
                y = None
            ys.append(y)
    return heads, ys
