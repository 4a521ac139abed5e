"""CPU tests (-m "not gpu") of the detector's network (gaussianrpg_amd/detector.py, csrc/detector.hip): the spec against
the reference's recorded state dict, the two doors against each other, the refusals, the BatchNorm folding, the
PyTorch route against the reference's recorded heads, the derived bounds of tests/detector_truth.py against the
reference's recorded leaf values and against planted errors, the plan's launch list, and the C entry points'
argument checks.  The recorded values come from tests/golden/make_golden_detector.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import detector_truth as T
from gaussianrpg_amd import detector as D
from gaussianrpg_amd import harness as hz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
MARGIN = 4.0   # the project's bound on a distance from the float64 truth: 4 x the reference's own


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_detector.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(T.GOLDEN, "ref_detector.npz"))


@pytest.fixture(scope="module")
def narrow():
    spec, sd, x = T.case_inputs("narrow_2x64x96")
    heads, layers = T.network64(spec, sd, x)
    return dict(spec=spec, sd=sd, x=x, heads=heads, layers=layers)


# ---- the spec ----

@pytest.mark.parametrize("model", ["narrow", "yolov5s"])
@pytest.mark.parametrize("fused", [False, True])
def test_spec_gives_the_reference_state_dict(golden, model, fused):
    spec = T.spec_of(model == "narrow")
    want = [(k, tuple(s)) for k, s in golden[0]["keys"][model]["fused" if fused else "unfused"]]
    assert spec.state_dict_shapes(fused) == want


def test_spec_figures_of_yolov5s(golden):
    spec = T.spec_of(False)
    assert spec.save == [4, 6, 10, 14, 17, 20, 23] and spec.stride == [8.0, 16.0, 32.0]
    assert (spec.nc, spec.na, spec.nl, spec.max_stride) == (80, 3, 3, 32)
    assert spec.parameters() == 7276605                      # the unfused yolov5s of this release
    assert [L["n"] for L in spec.layers if L["type"] == "C3"] == [1, 3, 3, 1, 1, 1, 1, 1]   # max(round(n * 0.33), 1)
    assert spec.layers[0] == {"type": "Focus", "from": -1, "f": [-1], "c1": 3, "c2": 32, "k": 3, "s": 1}
    assert np.array_equal(spec.anchor_grid[2], np.float32([[116, 90], [156, 198], [373, 326]]))
    narrow = T.spec_of(True)
    assert [L["c2"] for L in narrow.layers[:4]] == [16, 32, 32, 64]   # make_divisible(c * 0.25, 8)
    g = spec.geometry()
    assert (g.nl, g.na, g.nc) == (3, 3, 80)


@pytest.mark.parametrize("narrow_model", [True, False])
@pytest.mark.parametrize("fused", [False, True])
def test_from_module_equals_from_yaml(narrow_model, fused):
    spec = T.spec_of(narrow_model)
    assert D.DetectorSpec.from_module(T.stand_in_model(spec, fused=fused)) == spec


@pytest.mark.parametrize("module,args", [("BottleneckCSP", [128]), ("C3TR", [128]), ("GhostConv", [128, 3, 2]),
                                         ("DWConv", [128, 3, 2]), ("SPPF", [128, 5]), ("Contract", [2])])
def test_unsupported_yaml_modules_raise(module, args):
    cfg = T.load_cfg(True)
    cfg["backbone"][2] = [-1, 1, module, args]
    with pytest.raises(ValueError, match=module):
        D.DetectorSpec.from_yaml(cfg)


@pytest.mark.parametrize("layer,what", [([-1, 1, "Conv", [128, 5, 2]], "kernel 5"), ([-1, 1, "Conv", [128, 3, 4]], "stride 4"),
                                        ([-1, 1, "Conv", [128, 3, 2, None, 2]], "groups"),
                                        ([-1, 1, "Conv", [128, 3, 2, None, 1, False]], "non-SiLU"),
                                        ([-1, 1, "SPP", [128, [3, 5, 7]]], "SPP with kernels")])
def test_unsupported_yaml_arguments_raise(layer, what):
    cfg = T.load_cfg(True)
    cfg["backbone"][1 if layer[2] == "Conv" else 8] = layer
    with pytest.raises(ValueError, match=what):
        D.DetectorSpec.from_yaml(cfg)


@pytest.mark.parametrize("planted,what", [(dict(groups=2), "groups 2"), (dict(act="Hardswish"), "Hardswish"),
                                          (dict(block="TransformerBlock"), "TransformerBlock")])
def test_unsupported_modules_raise(planted, what):
    with pytest.raises(ValueError, match=what):
        D.DetectorSpec.from_module(T.stand_in_model(T.spec_of(True), **planted))


def test_refused_inputs_need_no_device(narrow):
    net = D.DetectorNet(narrow["spec"], narrow["sd"])
    with pytest.raises(TypeError, match="float32"):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="largest stride 32"):
        net(torch.zeros(1, 3, 48, 32))
    with pytest.raises(ValueError, match="largest stride 32"):
        net.layout(1, 32, 40)
    with pytest.raises(ValueError, match="no CPU path"):
        net(torch.zeros(1, 3, 32, 32))
    sd = dict(narrow["sd"])
    del sd["model.3.bn.weight"]
    with pytest.raises(KeyError, match="3"):
        D.DetectorNet(narrow["spec"], sd)


# ---- folding and the PyTorch route ----

def test_bn_folding_within_its_bound(narrow):
    spec, sd = narrow["spec"], narrow["sd"]
    fused = D.fused_parameters(spec, sd)
    worst = 0.0
    for c, (w, b) in zip(spec.convs(), fused):
        if c["plain"]:
            assert torch.equal(w, sd["model." + c["key"] + ".weight"]) and torch.equal(b, sd["model." + c["key"] + ".bias"])
            continue
        k = "model." + c["key"]
        (w64, wb), (b64, bb) = T.fold64(sd[k + ".conv.weight"], sd[k + ".bn.weight"], sd[k + ".bn.bias"],
                                        sd[k + ".bn.running_mean"], sd[k + ".bn.running_var"], spec.bn_eps)
        assert not torch.equal(w, sd[k + ".conv.weight"])        # the statistics are randomised: folding matters
        rw, rb = ((w.double() - w64).abs() / wb.clamp_min(1e-300)).max(), ((b.double() - b64).abs() / bb.clamp_min(1e-300)).max()
        worst = max(worst, float(rw), float(rb))
        assert rw <= 1 and rb <= 1, (c["key"], float(rw), float(rb))
    print("BN folding: worst err / bound %.3f" % worst)
    assert worst > 0.01            # the bound is not vacuous


def test_fused_and_unfused_state_dicts_give_the_same_parameters(narrow):
    spec, sd = narrow["spec"], narrow["sd"]
    fused_sd = {}
    for c, (w, b) in zip(spec.convs(), D.fused_parameters(spec, sd)):
        pre = c["key"] + ("" if c["plain"] else ".conv")           # keys without the "model." prefix
        fused_sd[pre + ".weight"], fused_sd[pre + ".bias"] = w, b
    for (w0, b0), (w1, b1) in zip(D.fused_parameters(spec, sd), D.fused_parameters(spec, fused_sd)):
        assert torch.equal(w0, w1) and torch.equal(b0, b1)


@pytest.mark.parametrize("case", list(T.CASES))
def test_detector_torch_reproduces_the_reference_heads(golden, case):
    meta, arrays = golden
    spec, sd, x = T.case_inputs(case)
    row = meta["cases"][case]
    assert T.sha256(x) == row["sha256_input"] and T.sha256(*[v.numpy() for v in sd.values()]) == row["sha256_weights"]
    heads = hz.detector_torch(spec, sd)(torch.from_numpy(x))
    for l, h in enumerate(heads):
        ref = arrays["%s/head%d" % (case, l)]
        assert h.dtype == torch.float32 and list(h.shape) == row["head_shapes"][l]
        d = T.rel_l2(h, ref)
        print("%s head %d: distance from the reference %.2e, the reference's from the truth %.2e" % (case, l, d, row["heads"][l][0]))
        assert d <= row["heads"][l][0]


def test_detector_torch_in_float64_is_the_truth(narrow):
    heads = hz.detector_torch(narrow["spec"], narrow["sd"], dtype=torch.float64)(torch.from_numpy(narrow["x"]))
    for h, t in zip(heads, narrow["heads"]):
        assert h.dtype == torch.float64 and T.rel_l2(h, t) < 1e-14


def test_recorded_truth_distances_are_reproduced(golden, narrow):
    row, arrays = golden[0]["cases"]["narrow_2x64x96"], golden[1]
    for l, t in enumerate(narrow["heads"]):
        assert T.rel_l2(arrays["narrow_2x64x96/head%d" % l], t) == pytest.approx(row["heads"][l][0], rel=1e-6)


# ---- the bounds: they hold the reference's values and reject planted errors ----

def _leaf_truth(name, variant=None):
    c, a = T.LEAVES[name], T.leaf_inputs(name)
    if c.get("pool"):
        return T.pool64(torch.from_numpy(a["x"]), 0.0 if variant == "zero_pad" else -np.inf), None
    return T.conv64(a["x"], a["w"], a["b"], c["k"], c["s"], True, a["res"], c.get("focus", False), variant)


@pytest.mark.parametrize("name", list(T.LEAVES))
def test_reference_leaf_values_lie_inside_the_bounds(golden, name):
    meta, arrays = golden
    a = T.leaf_inputs(name)
    assert T.sha256(*[v for v in a.values() if v is not None]) == meta["leaves"][name]["sha256_input"]
    ref = torch.from_numpy(arrays["leaf/" + name])
    want, bound = _leaf_truth(name)
    if bound is None:
        assert torch.equal(ref, want)           # data movement: exact
        return
    ratio = float(((ref.double() - want).abs() / bound).max())
    print("%s: the reference's worst err / bound %.3f" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("name,variant", [("conv_k3_s1_5x7", "kykx"), ("conv_k3_s1_5x7", "pad_off"),
                                          ("conv_k3_s2_7x9", "stride_phase"), ("focus_6x10", "focus_order"),
                                          ("conv_res_5x7", "no_res"), ("conv_res_5x7", "res_before_act"),
                                          ("conv_k3_s1_5x7", "no_bias"), ("conv_k3_long_chain", "no_bias"),
                                          ("pool_negative_3x4", "zero_pad")])
def test_planted_leaf_errors_are_rejected(name, variant):
    want, bound = _leaf_truth(name)
    wrong, _ = _leaf_truth(name, variant)
    if bound is None:
        assert not torch.equal(wrong, want)
        assert float(want.max()) < 0 and float(wrong.max()) == 0.0     # the zero padding wins every clipped window
        return
    ratio = float(((wrong - want).abs() / bound).max())
    assert ratio > 100, (name, variant, ratio)     # a kernel with this error fails the leaf test by orders of magnitude


@pytest.mark.parametrize("variant", ["concat_swapped", "upsample_shift"])
def test_planted_network_errors_are_rejected(golden, narrow, variant):
    row = golden[0]["cases"]["narrow_2x64x96"]
    wrong, _ = T.network64(narrow["spec"], narrow["sd"], narrow["x"], variant)
    ratios = [T.rel_l2(w, t) / (MARGIN * row["heads"][l][0]) for l, (w, t) in enumerate(zip(wrong, narrow["heads"]))]
    assert max(ratios) > 100, ratios


# ---- the plan's launch list ----

@pytest.mark.parametrize("case,shape", [("narrow_2x64x96", (2, 64, 96)), ("narrow_32x32", (1, 32, 32)),
                                        ("yolov5s_64x64", (1, 1088, 1600))])
def test_every_slice_is_written_once_and_read_after(case, shape):
    spec, sd, _ = T.case_inputs(case)
    net = D.DetectorNet(spec, sd)
    P = net.layout(*shape)
    written = {name: np.zeros(c, bool) for name, (c, _, _) in P.buffers.items()}
    pools = 0
    for n, s in enumerate(P.steps):
        for role in ("src", "res"):
            if s[role] is None or s[role][0] == "input":
                continue
            b, c0, c = s[role]
            assert written[b][c0:c0 + c].all(), "step %d reads %s[%d:%d] before it is written" % (n, b, c0, c0 + c)
            assert P.buffers[b][1:] == (s["hw_in"] if role == "src" else s["hw_out"])
        for role in ("dst", "up"):
            if s[role] is None:
                continue
            b, c0, c = s[role]
            assert c0 >= 0 and c0 + c <= P.buffers[b][0]
            assert not written[b][c0:c0 + c].any(), "step %d writes %s[%d:%d] twice" % (n, b, c0, c0 + c)
            written[b][c0:c0 + c] = True
            ho, wo = s["hw_out"]
            assert P.buffers[b][1:] == ((2 * ho, 2 * wo) if role == "up" else (ho, wo))
        pools += s["kind"] == "pool"
        if s["kind"] == "conv":
            cv = spec.convs()[s["conv"]]
            assert (cv["c1"], cv["c2"], cv["k"], cv["s"], cv["act"]) == (s["c_in"], s["c_out"], s["k"], s["s"], s["act"])
    assert all(w.all() for w in written.values()), [b for b, w in written.items() if not w.all()]
    convs = [s["conv"] for s in P.steps if s["kind"] == "conv"]
    assert sorted(convs) == list(range(len(spec.convs()))) and pools == 1      # every convolution exactly once
    assert len(P.steps) == 63 and sum(s["up"] is not None for s in P.steps) == 2
    assert [P.buffers["head%d" % l] for l in range(3)] == [(spec.na * spec.no, shape[1] // st, shape[2] // st) for st in (8, 16, 32)]


def test_tile_policy():
    spec, sd, _ = T.case_inputs("yolov5s_64x64")
    net = D.DetectorNet(spec, sd)
    P = net.layout(1, 1280, 1920)
    tiles = {s["key"]: s["tile"] for s in P.steps if s["kind"] == "conv"}
    assert tiles["0.conv"] == D.TILE_64        # 32 output channels: a quarter of a large tile's rows
    assert tiles["3"] == D.TILE_128            # 128 channels x 38400 pixels
    assert tiles["9.cv3"] == D.TILE_64         # the stride-32 level: 2400 pixels x 512 channels
    assert D.choose_tile(512, 2400) == D.TILE_64 and D.choose_tile(128, 128 * 256) == D.TILE_128
    assert {s["tile"] for s in net.layout(1, 64, 64, tile=D.TILE_128).steps if s["kind"] == "conv"} == {D.TILE_128}


# ---- the C entry points ----

class Layer(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("in_", ctypes.c_void_p), ("in_c0", ctypes.c_int), ("in_ct", ctypes.c_int),
                ("out", ctypes.c_void_p), ("out_c0", ctypes.c_int), ("out_ct", ctypes.c_int),
                ("res", ctypes.c_void_p), ("res_c0", ctypes.c_int), ("res_ct", ctypes.c_int),
                ("up", ctypes.c_void_p), ("up_c0", ctypes.c_int), ("up_ct", ctypes.c_int),
                ("packed", ctypes.c_void_p), ("bs", ctypes.c_int), ("c_in", ctypes.c_int), ("c_out", ctypes.c_int),
                ("h_in", ctypes.c_int), ("w_in", ctypes.c_int), ("h_out", ctypes.c_int), ("w_out", ctypes.c_int),
                ("k", ctypes.c_int), ("stride", ctypes.c_int), ("act", ctypes.c_int), ("in_mode", ctypes.c_int),
                ("tile", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the HIP runtime the library links)
    lib = ctypes.CDLL(LIB)
    lib.grpg_conv2d_packed_bytes.restype = ctypes.c_size_t
    lib.grpg_detector_run.restype = ctypes.c_int
    lib.grpg_detector_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.grpg_conv2d_pack_weights.restype = ctypes.c_int
    lib.grpg_conv2d_pack_weights.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    lib.grpg_last_error.restype = ctypes.c_char_p
    return lib


def _conv_layer(**kw):
    # addresses that are never dereferenced: the checks run on the host and nothing is enqueued
    L = Layer(kind=0, in_=0x10000, in_c0=0, in_ct=4, out=0x200000, out_c0=0, out_ct=8, res=None, up=None,
              packed=0x400000, bs=1, c_in=4, c_out=8, h_in=6, w_in=10, h_out=6, w_out=10, k=3, stride=1, act=1,
              in_mode=0, tile=0)
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def test_packed_bytes_is_a_pure_size_query(lib):
    assert lib.grpg_conv2d_packed_bytes(8, 12, 3) == 4 * 128 * (112 + 1)      # c_out -> 128, K = 108 -> 112, + bias
    assert lib.grpg_conv2d_packed_bytes(255, 512, 1) == 4 * 256 * 513
    assert lib.grpg_conv2d_packed_bytes(8, 12, 5) == 0 and lib.grpg_conv2d_packed_bytes(0, 12, 3) == 0


@pytest.mark.parametrize("bad,text", [
    (dict(in_=None), b"NULL"), (dict(out=None), b"NULL"), (dict(packed=None), b"NULL"),
    (dict(in_=0x10002), b"aligned"), (dict(packed=0x400004), b"16-byte"), (dict(res=0x300001), b"aligned"),
    (dict(bs=0), b"positive"), (dict(c_out=0), b"positive"), (dict(h_in=0), b"positive"),
    (dict(k=5), b"k must be 1 or 3"), (dict(stride=3), b"stride must be 1 or 2"), (dict(act=2), b"activation"),
    (dict(in_mode=2), b"input mode"), (dict(tile=2), b"tile"), (dict(kind=2), b"unknown kind"),
    (dict(in_c0=1), b"leaves its tensor"), (dict(out_c0=-1), b"leaves its tensor"), (dict(out_ct=7), b"leaves its tensor"),
    (dict(res=0x300000, res_c0=1, res_ct=8), b"residual slice"), (dict(up=0x500000, up_c0=0, up_ct=4), b"upsampled slice"),
    (dict(h_out=5), b"h_out / w_out"), (dict(stride=2), b"h_out / w_out"),
    (dict(in_mode=1, w_in=9, h_out=3, w_out=4), b"Focus"), (dict(out=0x10000), b"cannot write a tensor it reads"),
    (dict(kind=1), b"3 \\* c_in"), (dict(kind=1, c_out=12, out_ct=12, out=0x10000, in_ct=12), b"must not overlap"),
])
def test_detector_run_refuses_before_it_enqueues(lib, bad, text):
    good = _conv_layer()
    layers = (Layer * 2)(good, _conv_layer(**bad))      # the bad layer is the second: nothing may have been enqueued
    rc = lib.grpg_detector_run(ctypes.byref(layers), 2, None)
    assert rc == -1, (rc, lib.grpg_last_error())
    import re
    assert re.search(text, lib.grpg_last_error()) and b"layer 1" in lib.grpg_last_error(), lib.grpg_last_error()


def test_entry_points_without_arguments_or_device(lib):
    assert lib.grpg_detector_run(None, 1, None) == -1
    layers = (Layer * 1)(_conv_layer())
    assert lib.grpg_detector_run(ctypes.byref(layers), 0, None) == -1
    assert lib.grpg_conv2d_pack_weights(None, None, 8, 4, 3, 0x400000, None) == -1
    assert lib.grpg_conv2d_pack_weights(0x10000, None, 8, 4, 5, 0x400000, None) == -1
    assert lib.grpg_conv2d_pack_weights(0x10000, None, 8, 4, 3, 0x400004, None) == -1
    if torch.cuda.is_available():
        return            # with a device the valid calls below would run on made-up addresses
    pool = _conv_layer(kind=1, c_out=12, out_ct=16, out_c0=4, out=0x10000, in_ct=16)    # SPP's cat: one tensor, two slices
    layers = (Layer * 2)(_conv_layer(), pool)
    assert lib.grpg_detector_run(ctypes.byref(layers), 2, None) == -2                   # GRPG_ERR_NO_DEVICE: no fallback
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_conv2d_pack_weights(0x10000, None, 8, 4, 3, 0x400000, None) == -2


def test_records_have_the_struct_s_fields():
    assert list(D.RECORD_FIELDS) == [n.rstrip("_") for n, _ in Layer._fields_]
    row = D.conv_record(64, 1, 4, 6, 10, 128, 2, 8, 256, 2, 12, 8, 3, 1, True, focus=True, res=(512, 0, 8), tile=D.TILE_64)
    d = dict(zip(D.RECORD_FIELDS, row))
    assert (d["h_out"], d["w_out"], d["in_mode"], d["act"], d["res"], d["up"], d["tile"]) == (3, 5, 1, 1, 512, 0, 1)
    d = dict(zip(D.RECORD_FIELDS, D.pool_record(64, 0, 16, 64, 4, 16, 2, 4, 14, 20)))
    assert (d["kind"], d["c_in"], d["c_out"], d["h_out"], d["w_out"]) == (1, 4, 12, 14, 20)
