"""CPU tests (-m "not gpu") of the detector's network in fp16 (gaussianrpg_amd/detector.py ``dtype=torch.float16``,
csrc/detector_f16.hip): the reference's recorded half distances (tests/golden/make_golden_detector_f16.py) against the
PyTorch half route and against the contract's CPU restatement (tests/detector_f16_truth.py), the leaf bound against
planted contract errors, the gather's index walk against the direct formula, lossless packing of fp16-valued weights,
the half plan and its records, the C entry points' argument checks and the refusals of ``DetectorNet(dtype=...)``."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import detector_f16_truth as H
import detector_truth as T
from gaussianrpg_amd import detector as D
from gaussianrpg_amd import harness as hz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
MARGIN = 4.0   # the project's bound on a distance from the float64 truth: 4 x the reference's own


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_detector_f16.json")) as f:
        return json.load(f)


_cases = {}


def _case(name):
    if name not in _cases:
        spec, sd, x = T.case_inputs(name)
        _cases[name] = (spec, sd, x, T.network64(spec, sd, x)[0])      # the truth: once per case
    return _cases[name]


# ---- the recorded distances ----

@pytest.mark.parametrize("case", list(T.CASES))
def test_half_torch_route_reproduces_the_recorded_distances(golden, case):
    """The same ops in the same dtype as the reference's half model: per head within 25 % (the stand-in's order of
    roundings inside a convolution and a concatenation is CPU torch's either way).  The reference fuses in float32 and
    then calls ``.half()``, so the stand-in gets the float32-FUSED tensors: given the unfused ones it would fold
    BatchNorm in half, other ops, and lands 35 % off on narrow_32x32's first head (4.59e-4 against 3.39e-4)."""
    spec, sd, x, heads64 = _case(case)
    row = golden["cases"][case]
    assert T.sha256(x) == row["sha256_input"] and T.sha256(*[v.numpy() for v in sd.values()]) == row["sha256_weights"]
    fused_sd = {}
    for c, (w, b) in zip(spec.convs(), D.fused_parameters(spec, sd)):
        pre = c["key"] + ("" if c["plain"] else ".conv")
        fused_sd[pre + ".weight"], fused_sd[pre + ".bias"] = w, b
    heads = hz.detector_torch(spec, fused_sd, dtype=torch.float16)(torch.from_numpy(x))
    for l, (h, t) in enumerate(zip(heads, heads64)):
        assert h.dtype == torch.float16 and list(h.shape) == row["head_shapes"][l]
        d = T.rel_l2(h.float(), t)
        print("%s head %d: half torch %.3e, the reference's half model %.3e" % (case, l, d, row["heads"][l][0]))
        assert d == pytest.approx(row["heads"][l][0], rel=0.25)


@pytest.mark.parametrize("case", list(T.CASES))
def test_contract_restatement_is_inside_the_bar(golden, case):
    spec, sd, x, heads64 = _case(case)
    row = golden["cases"][case]
    heads, _ = H.network_f16(spec, sd, x)
    for l, (h, t) in enumerate(zip(heads, heads64)):
        assert h.dtype == torch.float32 and list(h.shape) == row["head_shapes"][l]
        d = T.rel_l2(h, t)
        print("%s head %d: the contract %.3e, the reference's half model %.3e, ratio %.2f" %
              (case, l, d, row["heads"][l][0], d / row["heads"][l][0]))
        assert d <= MARGIN * row["heads"][l][0]


# ---- the leaf bound: it holds the restatement and rejects planted contract errors ----

# name: (bs, c_in, c_out, k, stride, (h, w), act, res, out_f32)
LEAVES = {
    "k3_res_5x7": (1, 8, 8, 3, 1, (5, 7), True, True, False),
    "k3_res_9x11_bs2": (2, 12, 18, 3, 1, (9, 11), True, True, False),
    "k1_linear_heads": (1, 32, 24, 1, 1, (6, 4), False, False, True),
    "k3_K4608_linear": (1, 512, 8, 3, 1, (5, 7), False, False, False),
}


def _leaf(name):
    bs, c_in, c_out, k, s, hw, act, res, out_f32 = LEAVES[name]
    x, w, b, rs = H.leaf_case(sum(map(ord, name)), bs, c_in, c_out, k, hw)
    r = H.rep16(rs.normal(0, 1, (bs, c_out, hw[0], hw[1])).astype(np.float32)) if res else None
    return (x, w, b, k, s, act, r, False, out_f32)


def _ratio(args, variant=None):
    want, bound = H.conv64_f16(*args)
    got = H.conv_f16_restated(*args, variant=variant)
    return float(((got.double() - want).abs() / bound).max())


@pytest.mark.parametrize("name", list(LEAVES))
def test_restated_leaf_lies_inside_the_bound(name):
    ratio = _ratio(_leaf(name))
    print("%s: worst err / bound %.3f" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("variant", ["res_before_act", "bias_f16", "round_to_zero"])
def test_planted_contract_errors_leave_the_bound(variant):
    ratios = {name: _ratio(_leaf(name), variant) for name in LEAVES}
    print(variant, {k: round(v, 2) for k, v in ratios.items()})
    assert max(ratios.values()) > 1.0, ratios


def test_rep16_values():
    v = H.rep16(np.float32([1.0, 2.0 ** -14, 2.0 ** -15, -2.0 ** -20, 0.1, 70000.0, 0.0]))
    assert v.tolist() == [1.0, 2.0 ** -14, 0.0, 0.0, float(np.float16(0.1)), float("inf"), 0.0]
    r = H.round16(torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -13, -(1.0 + 2.0 ** -11 + 2.0 ** -13), 1.0]), "round_to_zero")
    assert r.tolist() == [1.0, -1.0, 1.0]
    assert H.round16(torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -13])).item() == 1.0 + 2.0 ** -10


# ---- the gather's index walk ----

def test_gather_walk_equals_the_direct_formula(tmp_path):
    """csrc/detector_gather.h is plain integer code: compiled for the host and compared, element by element, with
    (ci, ky, kx) = divmod of k, the four padding comparisons and the plain / Focus offsets."""
    import subprocess
    exe = str(tmp_path / "gather_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "gaussianrpg_amd", "csrc"),
                    os.path.join(ROOT, "tests", "detector_gather_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok, ") and int(out.split()[1]) > 1_000_000, out


# ---- weights ----

def test_fp16_valued_weights_round_losslessly():
    spec, sd, _, _ = _case("narrow_32x32")
    fused = D.fused_parameters(spec, sd)
    half_sd = {}
    for c, (w, b) in zip(spec.convs(), fused):
        pre = c["key"] + ("" if c["plain"] else ".conv")
        half_sd[pre + ".weight"], half_sd[pre + ".bias"] = w.half().float(), b
    net = D.DetectorNet(spec, half_sd, dtype=torch.float16)
    assert net.dtype == torch.float16
    lossy = 0
    for (w0, b0), (w1, b1), (w2, b2) in zip(fused, net.params, H.fused_f16(spec, half_sd)):
        assert w1.dtype == torch.float32 and torch.equal(w1.half().float(), w1)       # what the repack rounds: no loss
        assert torch.equal(w1, w0.half().float()) and torch.equal(b1, b0) and torch.equal(w2, w1) and torch.equal(b2, b0)
        lossy += int(not torch.equal(w0, w1))
    assert lossy == len(fused)             # the float32 weights themselves were not fp16 values: the test is not vacuous


# ---- the plan ----

class Layer16(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("in_", ctypes.c_void_p), ("in_c0", ctypes.c_int), ("in_ct", ctypes.c_int),
                ("out", ctypes.c_void_p), ("out_c0", ctypes.c_int), ("out_ct", ctypes.c_int),
                ("res", ctypes.c_void_p), ("res_c0", ctypes.c_int), ("res_ct", ctypes.c_int),
                ("up", ctypes.c_void_p), ("up_c0", ctypes.c_int), ("up_ct", ctypes.c_int),
                ("packed", ctypes.c_void_p), ("bs", ctypes.c_int), ("c_in", ctypes.c_int), ("c_out", ctypes.c_int),
                ("h_in", ctypes.c_int), ("w_in", ctypes.c_int), ("h_out", ctypes.c_int), ("w_out", ctypes.c_int),
                ("k", ctypes.c_int), ("stride", ctypes.c_int), ("act", ctypes.c_int), ("in_mode", ctypes.c_int),
                ("tile", ctypes.c_int), ("out_f32", ctypes.c_int)]


def test_records_have_the_struct_s_fields():
    assert list(D.RECORD_FIELDS_F16) == [n.rstrip("_") for n, _ in Layer16._fields_]
    assert D.RECORD_FIELDS_F16[:-1] == D.RECORD_FIELDS and len(D.RECORD_FIELDS) == 26
    assert ctypes.sizeof(Layer16) == 136 and Layer16.out_f32.offset == 128 and Layer16.packed.offset == 72
    args = (64, 1, 4, 6, 10, 128, 2, 8, 256, 2, 12, 8, 3, 1, True)
    row = D.conv_record_f16(*args, focus=True, res=(512, 0, 8), tile=D.TILE_64)
    assert row[:-1] == D.conv_record(*args, focus=True, res=(512, 0, 8), tile=D.TILE_64) and row[-1] == 0
    assert D.conv_record_f16(*args, out_f32=True)[-1] == 1 and len(row) == 27
    assert D.pool_record_f16(64, 0, 16, 64, 4, 16, 2, 4, 14, 20) == D.pool_record(64, 0, 16, 64, 4, 16, 2, 4, 14, 20) + [0]


@pytest.mark.parametrize("case,shape", [("narrow_2x64x96", (2, 64, 96)), ("yolov5s_64x64", (1, 1088, 1600))])
def test_half_plan(case, shape):
    spec, sd, _, _ = _case(case)
    net32, net16 = D.DetectorNet(spec, sd), D.DetectorNet(spec, sd, dtype=torch.float16)
    P, Q = net32.layout(*shape), net16.layout(*shape)
    assert P.steps == Q.steps and P.buffers == Q.buffers and len(Q.steps) == 63          # layout() is dtype-free
    off32, bytes32 = net32.arena_layout(P)
    off16, bytes16 = net16.arena_layout(Q)
    al = lambda n: -(-n // 256) * 256
    want = 0
    for name, (c, h, w) in Q.buffers.items():
        assert off16[name] == want and off16[name] % 256 == 0
        want += al(shape[0] * c * h * w * (4 if name.startswith("head") else 2))
    assert bytes16 == want
    assert bytes32 == sum(al(shape[0] * c * h * w * 4) for c, h, w in P.buffers.values())
    heads = sum(al(shape[0] * c * h * w * 4) for n, (c, h, w) in Q.buffers.items() if n.startswith("head"))
    assert abs((bytes16 - heads) - (bytes32 - heads) / 2) <= 128 * len(Q.buffers)         # half, up to the alignment
    print("%s %s: arena %.1f MiB in float32, %.1f MiB in fp16" % (case, shape, bytes32 / 2 ** 20, bytes16 / 2 ** 20))
    # every slice written once and read after (the steps are test_detector_host's; here: the head rows)
    written = {name: np.zeros(c, bool) for name, (c, _, _) in Q.buffers.items()}
    for n, s in enumerate(Q.steps):
        for role in ("src", "res"):
            if s[role] is not None and s[role][0] != "input":
                b, c0, c = s[role]
                assert written[b][c0:c0 + c].all(), "step %d reads %s[%d:%d] before it is written" % (n, b, c0, c0 + c)
        for role in ("dst", "up"):
            if s[role] is not None:
                b, c0, c = s[role]
                assert not written[b][c0:c0 + c].any(), "step %d writes %s[%d:%d] twice" % (n, b, c0, c0 + c)
                written[b][c0:c0 + c] = True
    assert all(w.all() for w in written.values())
    head_rows = [n for n, s in enumerate(Q.steps) if s["dst"][0].startswith("head")]
    assert len(head_rows) == spec.nl
    for n in head_rows:      # what plan() marks out_f32: a float32 output takes no residual, no second store, no SiLU
        assert Q.steps[n]["res"] is None and Q.steps[n]["up"] is None and not Q.steps[n]["act"]
    assert not any(s["src"][0].startswith("head") or (s["res"] or ("",))[0].startswith("head") for s in Q.steps)
    # the records: out_f32 on exactly the head rows, addresses inside the arena at the buffers' byte offsets
    base = 0x7F0000000000
    rows = net16.records_of(Q, off16, base, [0x1000 * (1 + n) for n in range(len(spec.convs()))])
    f = {name: i for i, name in enumerate(D.RECORD_FIELDS_F16)}
    assert all(len(r) == 27 for r in rows) and [n for n, r in enumerate(rows) if r[f["out_f32"]]] == head_rows
    for r, s in zip(rows, Q.steps):
        assert r[f["out"]] == base + off16[s["dst"][0]] and r[f["out_ct"]] == Q.buffers[s["dst"][0]][0]
        assert r[f["in"]] == (0 if s["src"][0] == "input" else base + off16[s["src"][0]])
        assert base <= r[f["out"]] < base + bytes16
    rows32 = net32.records_of(P, off32, base, [0x1000 * (1 + n) for n in range(len(spec.convs()))])
    assert all(len(r) == 26 for r in rows32) and [r[:1] + r[14:] for r in rows32] == [r[:1] + r[14:26] for r in rows]


# ---- the C entry points ----

@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the HIP runtime the library links)
    lib = ctypes.CDLL(LIB)
    lib.grpg_conv2d_packed_bytes_f16.restype = ctypes.c_size_t
    lib.grpg_detector_run_f16.restype = ctypes.c_int
    lib.grpg_detector_run_f16.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.grpg_conv2d_pack_weights_f16.restype = ctypes.c_int
    lib.grpg_conv2d_pack_weights_f16.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_abi_version.restype = ctypes.c_int
    return lib


def _conv_layer(**kw):
    # addresses that are never dereferenced: the checks run on the host and nothing is enqueued
    L = Layer16(kind=0, in_=0x10000, in_c0=0, in_ct=4, out=0x200000, out_c0=0, out_ct=8, res=None, up=None,
                packed=0x400000, bs=1, c_in=4, c_out=8, h_in=6, w_in=10, h_out=6, w_out=10, k=3, stride=1, act=1,
                in_mode=0, tile=0, out_f32=0)
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def test_packed_bytes_f16_is_a_pure_size_query(lib):
    assert lib.grpg_abi_version() == 7
    assert lib.grpg_conv2d_packed_bytes_f16(8, 12, 3) == 4 * 128 + 2 * 128 * 128       # c_out -> 128, K = 108 -> 128
    assert lib.grpg_conv2d_packed_bytes_f16(255, 512, 1) == 4 * 256 + 2 * 256 * 512
    assert lib.grpg_conv2d_packed_bytes_f16(3, 5, 3) == 4 * 128 + 2 * 128 * 64         # K = 45 -> 64
    assert lib.grpg_conv2d_packed_bytes_f16(8, 12, 5) == 0 and lib.grpg_conv2d_packed_bytes_f16(0, 12, 3) == 0
    assert lib.grpg_conv2d_packed_bytes_f16(8, -1, 1) == 0


@pytest.mark.parametrize("bad,text", [
    (dict(in_=None), b"NULL"), (dict(out=None), b"NULL"), (dict(packed=None), b"NULL"),
    (dict(in_=0x10001), b"2-byte aligned"), (dict(out=0x200001), b"2-byte aligned"), (dict(res=0x300001), b"2-byte aligned"),
    (dict(up=0x500001, up_ct=8), b"2-byte aligned"), (dict(out=0x200002, out_f32=1, act=0), b"4-byte aligned"),
    (dict(packed=0x400008), b"16-byte"),
    (dict(bs=0), b"positive"), (dict(c_out=0), b"positive"), (dict(h_in=0), b"positive"),
    (dict(k=5), b"k must be 1 or 3"), (dict(stride=3), b"stride must be 1 or 2"), (dict(act=2), b"activation"),
    (dict(in_mode=2), b"input mode"), (dict(tile=2), b"tile"), (dict(kind=2), b"unknown kind"),
    (dict(out_f32=2), b"out_f32 must be 0 or 1"),
    (dict(out_f32=1, res=0x300000, res_ct=8), b"no residual"), (dict(out_f32=1, up=0x500000, up_ct=8), b"no residual"),
    (dict(in_c0=1), b"leaves its tensor"), (dict(out_c0=-1), b"leaves its tensor"), (dict(out_ct=7), b"leaves its tensor"),
    (dict(res=0x300000, res_c0=1, res_ct=8), b"residual slice"), (dict(up=0x500000, up_c0=0, up_ct=4), b"upsampled slice"),
    (dict(h_out=5), b"h_out / w_out"), (dict(stride=2), b"h_out / w_out"),
    (dict(in_mode=1, w_in=9, h_out=3, w_out=4), b"Focus"), (dict(out=0x10000), b"cannot write a tensor it reads"),
    # the overlap is in bytes: the input is 1 * 4 * 6 * 10 halves = 480 bytes
    (dict(out=0x10000 + 478), b"cannot write a tensor it reads"),
    (dict(kind=1), b"3 \\* c_in"), (dict(kind=1, c_out=12, out_ct=12, out=0x10000, in_ct=12), b"must not overlap"),
    (dict(kind=1, c_out=12, out_ct=12, out_f32=1), b"out_f32 must be 0"),
])
def test_detector_run_f16_refuses_before_it_enqueues(lib, bad, text):
    layers = (Layer16 * 2)(_conv_layer(), _conv_layer(**bad))      # the bad layer is the second: nothing was enqueued
    rc = lib.grpg_detector_run_f16(ctypes.byref(layers), 2, None)
    assert rc == -1, (rc, lib.grpg_last_error())
    assert re.search(text, lib.grpg_last_error()) and b"layer 1" in lib.grpg_last_error(), lib.grpg_last_error()


def test_f16_entry_points_without_arguments_or_device(lib):
    assert lib.grpg_detector_run_f16(None, 1, None) == -1
    layers = (Layer16 * 1)(_conv_layer())
    assert lib.grpg_detector_run_f16(ctypes.byref(layers), 0, None) == -1
    assert lib.grpg_conv2d_pack_weights_f16(None, None, 8, 4, 3, 0x400000, None) == -1
    assert lib.grpg_conv2d_pack_weights_f16(0x10000, None, 8, 4, 5, 0x400000, None) == -1
    assert lib.grpg_conv2d_pack_weights_f16(0x10000, None, 8, 4, 3, 0x400004, None) == -1
    assert lib.grpg_conv2d_pack_weights_f16(0x10002, None, 8, 4, 3, 0x400000, None) == -1
    if torch.cuda.is_available():
        return            # with a device the valid calls below would run on made-up addresses
    # the byte-exact neighbours are accepted: out right behind the 480 bytes of the input, a float32 head
    ok = (Layer16 * 3)(_conv_layer(), _conv_layer(out=0x10000 + 480), _conv_layer(out_f32=1, act=0))
    assert lib.grpg_detector_run_f16(ctypes.byref(ok), 3, None) == -2                   # GRPG_ERR_NO_DEVICE: no fallback
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_conv2d_pack_weights_f16(0x10000, None, 8, 4, 3, 0x400000, None) == -2


# ---- DetectorNet(dtype=...) ----

def test_dtype_refusals_need_no_device():
    spec, sd, _, _ = _case("narrow_32x32")
    with pytest.raises(TypeError, match="float32 or torch.float16"):
        D.DetectorNet(spec, sd, dtype=torch.bfloat16)
    net16 = D.DetectorNet(spec, sd, dtype=torch.float16)
    with pytest.raises(TypeError, match="float16"):
        net16(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="no CPU path"):
        net16(torch.zeros(1, 3, 32, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="largest stride 32"):
        net16(torch.zeros(1, 3, 48, 32, dtype=torch.float16))
    net32 = D.DetectorNet(spec, sd)
    assert net32.dtype == torch.float32
    with pytest.raises(TypeError, match="x must be float32 \\(got torch.float16\\); the network is the FP32 model"):
        net32(torch.zeros(1, 3, 32, 32, dtype=torch.float16))
    other = D.DetectorNet.from_module(T.stand_in_model(spec, sd), dtype=torch.float16)
    assert other.dtype == torch.float16 and other.spec == spec
