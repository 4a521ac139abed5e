"""GPU tests of the detector's network in fp16 (gaussianrpg_amd/detector.py ``dtype=torch.float16``,
csrc/detector_f16.hip).  Every comparison is against a truth computed on the CPU (tests/detector_truth.py,
tests/detector_f16_truth.py); no torch convolution runs on the device.

1. The convolution leaf against float64 within the derived per-element bound (detector_f16_truth's docstring): every
   geometry of test_gpu_detector's CONV_CASES plus K on, one over and below the 32-deep tile, on fp16-representable
   inputs without fp16 subnormals, always inside wider tensors whose other channels hold an fp16 sentinel that must
   survive bit for bit, with BOTH tile shapes, whose bits must be equal.
2. The pool leaf bit for bit, the packed layout, the binding's refusals.
3. The whole network: per head at most MARGIN x the reference's half model's own recorded distance from the float64
   truth (tests/golden/ref_detector_f16.json), determinism, the second call's launches / waits / allocations, the two
   doors, and a frame through ``harness.simulator_detections_from_frame`` without a cast launch.
"""
import json
import os

import numpy as np
import pytest
import torch

import detector_f16_truth as H
import detector_truth as T
from gaussianrpg_amd import detector as D
from test_gpu_detector import CONV_CASES

pytestmark = pytest.mark.gpu
MARGIN = 4.0
SENTINEL = 1234.5          # an fp16 value
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES_F16 = dict(CONV_CASES)
CASES_F16.update({
    "k1_K32": (1, 32, 18, 1, 1, (5, 7), True, False, False, False),            # K on the 32-deep tile
    "k1_K33": (1, 33, 18, 1, 1, (5, 7), True, False, False, False),            # one over: a second tile with one tap
    "k3_K27_cout8_3x3": (1, 3, 8, 3, 1, (3, 3), True, False, False, False),    # K below one tile, over one instruction
    "k1_K12_cout255_heads_6x4_bs2": (2, 12, 255, 1, 1, (6, 4), False, False, False, False),   # run with out_f32
})
OUT_F32 = ("k1_K12_cout255_heads_6x4_bs2",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _wide(dev, x, c0, extra, dtype=torch.float16):
    """x [bs, c, h, w] inside a [bs, c0 + c + extra, h, w] tensor of sentinels."""
    x = torch.as_tensor(x)
    t = torch.full((x.shape[0], c0 + x.shape[1] + extra, x.shape[2], x.shape[3]), SENTINEL, dtype=dtype)
    t[:, c0:c0 + x.shape[1]] = x.to(dtype)
    return t.to(dev)


def _untouched(t, c0, c):
    rest = torch.cat((t[:, :c0], t[:, c0 + c:]), 1)
    return bool((rest == torch.tensor(SENTINEL, dtype=t.dtype)).all())


def run_conv(dev, x, w, b, k, s, act, res=None, focus=False, up=False, tile=D.TILE_64, out_f32=False, offs=(2, 3, 1, 4)):
    """The kernel on x (stored layout, fp16 values) inside wider tensors; returns (out, up or None) on the host after
    checking every sentinel and that input and residual are unchanged."""
    bs, _, h, wd = x.shape
    c_out, c_in = w.shape[0], w.shape[1]
    ic0, oc0, rc0, uc0 = offs
    xin = _wide(dev, x, ic0, 2)
    lh, lw = (h // 2, wd // 2) if focus else (h, wd)
    ho, wo = D.out_size(lh, k, s), D.out_size(lw, k, s)
    out = torch.full((bs, oc0 + c_out + 1, ho, wo), SENTINEL, dtype=torch.float32 if out_f32 else torch.float16, device=dev)
    rt = None if res is None else _wide(dev, res, rc0, 1)
    ut = torch.full((bs, uc0 + c_out + 2, 2 * ho, 2 * wo), SENTINEL, dtype=torch.float16, device=dev) if up else None
    packed = D.pack_weights_f16(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev))
    rec = D.conv_record_f16(xin.data_ptr(), ic0, xin.shape[1], h, wd, out.data_ptr(), oc0, out.shape[1], packed.data_ptr(),
                            bs, c_in, c_out, k, s, act, res=None if rt is None else (rt.data_ptr(), rc0, rt.shape[1]),
                            up=None if ut is None else (ut.data_ptr(), uc0, ut.shape[1]), focus=focus, tile=tile,
                            out_f32=out_f32)
    D.run_records_f16([rec], xin)
    torch.cuda.synchronize()
    assert _untouched(out, oc0, c_out), "the output's other channels changed"
    assert torch.equal(xin.cpu(), _wide("cpu", x, ic0, 2)), "the input changed"
    if rt is not None:
        assert torch.equal(rt.cpu(), _wide("cpu", res, rc0, 1)), "the residual changed"
    got_up = None
    if ut is not None:
        assert _untouched(ut, uc0, c_out), "the upsampled tensor's other channels changed"
        got_up = ut[:, uc0:uc0 + c_out].cpu()
    return out[:, oc0:oc0 + c_out].cpu(), got_up


RATIOS = {}


@pytest.mark.parametrize("name", list(CASES_F16))
def test_conv_leaf(dev, name):
    bs, c_in, c_out, k, s, hw, act, res, focus, up = CASES_F16[name]
    out_f32 = name in OUT_F32
    x, w, b, rs = H.leaf_case(sum(map(ord, name)), bs, c_in, c_out, k, hw, focus=focus)
    lh, lw = (hw[0] // 2, hw[1] // 2) if focus else hw
    r = H.rep16(rs.normal(0, 1, (bs, c_out, D.out_size(lh, k, s), D.out_size(lw, k, s))).astype(np.float32)) if res else None
    want, bound = H.conv64_f16(x, w, b, k, s, act, r, focus, out_f32=out_f32)
    got = {}
    for tile in (D.TILE_128, D.TILE_64):
        out, upo = run_conv(dev, x, w, b, k, s, act, r, focus, up, tile, out_f32)
        assert out.shape == want.shape and out.dtype == (torch.float32 if out_f32 else torch.float16)
        ratio = float(((out.double() - want).abs() / bound).max())
        RATIOS["%s/tile%d" % (name, tile)] = ratio
        print("%s tile %s: worst err / bound %.3f" % (name, "128" if tile == D.TILE_128 else "64", ratio))
        assert ratio <= 1.0
        if up:
            assert torch.equal(upo, out.repeat_interleave(2, 2).repeat_interleave(2, 3))     # the stored values, 2 x 2
        got[tile] = out
    assert torch.equal(got[D.TILE_128], got[D.TILE_64])     # the same instructions per element in both shapes: same bits


def test_conv_leaf_twice_gives_the_same_bits(dev):
    x, w, b, _ = H.leaf_case(5, 2, 64, 40, 3, (9, 11))
    a, _ = run_conv(dev, x, w, b, 3, 1, True, tile=D.TILE_128)
    c, _ = run_conv(dev, x, w, b, 3, 1, True, tile=D.TILE_128)
    assert torch.equal(a, c)


def test_output_overflows_to_inf_as_half_does(dev):
    """1 x 1, one channel, linear: out = w * x + b exactly in float32, then the one rounding.  65265 -> 65280; 65519 is
    below the tie 65520 -> 65504, the largest fp16; 65521 -> inf, -65551 -> -inf: as ``Tensor.half()``."""
    x = np.float32([[[[255.0, 256.0, -256.0, 1.0], [256.0, 0.0, 0.0, 0.0]]]])
    w, b = np.float32([[[[256.0]]], [[[256.0]]]]), np.float32([-15.0, -17.0])
    out, _ = run_conv(dev, x, w, b, 1, 1, False)
    want = (torch.from_numpy(x) * 256.0 + torch.tensor([-15.0, -17.0]).view(1, 2, 1, 1)).half()
    assert want[0, 0, 0].tolist() == [65280.0, float("inf"), float("-inf"), 241.0] and want[0, 1, 1, 0].item() == 65504.0
    assert torch.equal(out, want)


def test_packed_weights_layout(dev):
    x, w, b, _ = H.leaf_case(6, 1, 5, 3, 3, (2, 2))
    w32 = (w * np.float32(1.0009765625)).astype(np.float32)             # no longer fp16 values: the repack rounds
    p = D.pack_weights_f16(torch.from_numpy(w32).to(dev), torch.from_numpy(b).to(dev)).cpu()
    assert p.dtype == torch.uint8 and p.numel() == 4 * 128 + 2 * 128 * 64          # bias block, c_out -> 128, K = 45 -> 64
    bias, body = p[:512].view(torch.float32), p[512:].view(torch.float16).view(128, 64)
    assert torch.equal(bias[:3], torch.from_numpy(b)) and not bias[3:].any()
    assert torch.equal(body[:3, :45], torch.from_numpy(w32).reshape(3, 45).half())   # [m][k], nearest even
    assert not torch.equal(body[:3, :45].float(), torch.from_numpy(w32).reshape(3, 45))
    assert not body[3:].any() and not body[:, 45:].any()


# ---- pool ----

@pytest.mark.parametrize("bs,c,hw,negative", [(1, 3, (1, 1), False), (1, 3, (3, 4), False), (2, 2, (13, 13), False),
                                              (2, 4, (14, 20), False), (1, 3, (3, 4), True), (1, 2, (33, 17), True),
                                              (1, 2, (16, 32), False)])
def test_pool_leaf(dev, bs, c, hw, negative):
    x = torch.from_numpy(T.build_tensor((bs, c, hw[0], hw[1]), 40 + hw[0] + hw[1] + negative, negative)).half()
    want = T.pool64(x.float()).half()             # max of fp16 values: exact in either dtype
    # SPP's layout: one tensor, the input slice in front of the three output slices, sentinels around
    cat = torch.full((bs, 1 + 4 * c + 2, hw[0], hw[1]), SENTINEL, dtype=torch.float16)
    cat[:, 1:1 + c] = x
    cat = cat.to(dev)
    D.run_records_f16([D.pool_record_f16(cat.data_ptr(), 1, cat.shape[1], cat.data_ptr(), 1 + c, cat.shape[1], bs, c, hw[0], hw[1])], cat)
    torch.cuda.synchronize()
    got = cat.cpu()
    assert torch.equal(got[:, 1:1 + c], x) and _untouched(got, 1, 4 * c)
    assert torch.equal(got[:, 1 + c:1 + 4 * c], want)
    if negative:
        assert float(got[:, 1 + c:1 + 4 * c].max()) < 0
    # and into a tensor of its own
    xin = _wide(dev, x, 2, 1)
    out = torch.full((bs, 3 * c + 3, hw[0], hw[1]), SENTINEL, dtype=torch.float16, device=dev)
    D.run_records_f16([D.pool_record_f16(xin.data_ptr(), 2, xin.shape[1], out.data_ptr(), 3, out.shape[1], bs, c, hw[0], hw[1])], xin)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 3:].cpu(), want) and _untouched(out, 3, 3 * c)


def test_binding_refuses_bad_records(dev):
    x = torch.zeros(1, 4, 4, 4, device=dev, dtype=torch.float16)
    rec = D.pool_record_f16(x.data_ptr(), 0, 4, x.data_ptr(), 1, 4, 1, 1, 4, 4)
    rec[5] = 2                                                     # out slice [2, 5) of 4 channels
    with pytest.raises(RuntimeError, match="leaves its tensor"):
        D.run_records_f16([rec], x)
    with pytest.raises(RuntimeError, match="records must be"):
        D.run_records_f16(torch.zeros(1, 26, dtype=torch.int64), x)
    with pytest.raises(RuntimeError, match="records must be"):
        D.run_records(torch.zeros(1, 27, dtype=torch.int64), x)
    with pytest.raises(RuntimeError, match="float32"):
        D.pack_weights_f16(torch.zeros(8, 4, 3, 3, device=dev, dtype=torch.float16))


# ---- the whole network ----

@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_detector_f16.json")) as f:
        return json.load(f)


_nets = {}
PARITY = {}


def _net(case):
    if case not in _nets:
        spec, sd, x = T.case_inputs(case)
        heads64, _ = T.network64(spec, sd, x)        # the truth: once per case
        _nets[case] = (D.DetectorNet(spec, sd, dtype=torch.float16), spec, sd, x, heads64)
    return _nets[case]


@pytest.mark.parametrize("case", list(T.CASES))
def test_network_heads(dev, golden, case):
    net, spec, sd, x, heads64 = _net(case)
    row = golden["cases"][case]
    xh = torch.from_numpy(x).half()
    heads = net(xh.to(dev))
    torch.cuda.synchronize()
    restated, _ = H.network_f16(spec, sd, xh)
    assert len(heads) == spec.nl
    PARITY[case] = []
    for l, (h, t) in enumerate(zip(heads, heads64)):
        assert h.dtype == torch.float32 and list(h.shape) == row["head_shapes"][l] and h.is_contiguous()
        d, dr = T.rel_l2(h.cpu(), t), T.rel_l2(h.cpu(), restated[l])
        PARITY[case].append(dict(rel_l2=d, reference_rel_l2=row["heads"][l][0], ratio=d / row["heads"][l][0],
                                 rel_l2_from_cpu_restatement=dr))
        print("%s head %d: rel L2 %.3e, the reference's half model %.3e, ratio %.2f; from the CPU restatement %.3e" %
              (case, l, d, row["heads"][l][0], d / row["heads"][l][0], dr))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "detector_f16_parity.json"), "w") as f:
        json.dump({"margin": MARGIN, "device": torch.cuda.get_device_name(dev), "cases": PARITY}, f, indent=1)
        f.write("\n")
    for p in PARITY[case]:
        assert p["ratio"] <= MARGIN


def test_network_both_tile_shapes_and_twice(dev):
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).half().to(dev)
    first = [h.clone() for h in net(xd)]
    again = [h.clone() for h in net(xd)]
    big = [h.clone() for h in net(xd, tile=D.TILE_128)]
    small = [h.clone() for h in net(xd, tile=D.TILE_64)]
    for a, b, c, d in zip(first, again, big, small):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_replan_and_back(dev):
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).half().to(dev)
    first = [h.clone() for h in net(xd)]
    other = net(torch.from_numpy(T.build_input(1, 96, 32, 9)).half().to(dev))
    assert [tuple(h.shape) for h in other] == [(1, 24, 12, 4), (1, 24, 6, 2), (1, 24, 3, 1)]
    assert net.plan(2, 64, 96, dev) is net.plan(2, 64, 96, dev) and len(net._plans) >= 2
    P = net.plan(2, 64, 96, dev)
    assert P.arena.dtype == torch.uint8 and P.arena.numel() == P.arena_bytes == net.arena_layout(net.layout(2, 64, 96))[1]
    for a, b in zip(first, net(xd)):
        assert torch.equal(a, b)


def test_detections_equal_detections_from_heads(dev):
    from gaussianrpg_amd.perception import detections_from_heads
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).half().to(dev)
    det, count = net.detections(xd, conf_thres=0.05, max_det=50)
    det2, count2 = detections_from_heads(net(xd), net.geometry, conf_thres=0.05, max_det=50)
    assert torch.equal(det, det2) and torch.equal(count, count2)
    assert int(count.sum()) > 0 and net.stride.tolist() == [8.0, 16.0, 32.0]


def test_second_call_launches_only(dev):
    from torch.profiler import ProfilerActivity, profile
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).half().to(dev)
    net(xd)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        net(xd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before      # no allocation
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        net(xd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    assert [n for n in names if "memcpy" in n.lower() or "memset" in n.lower()] == []
    assert len(names) == 63 and sum("spp_f16_kernel" in n for n in names) == 1
    assert sum("conv_f16_kernel" in n for n in names) == 62


def test_from_module_gives_the_same_bits(dev):
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).half().to(dev)
    want = [h.clone() for h in net(xd)]
    other = D.DetectorNet.from_module(T.stand_in_model(spec, sd), dtype=torch.float16)
    for a, b in zip(want, other(xd)):
        assert torch.equal(a, b)
    with pytest.raises(TypeError, match="float16"):
        net(xd.float())
    with pytest.raises(ValueError, match="largest stride"):
        net(xd[:, :, :48].contiguous())


def test_frame_to_detections_without_a_cast(dev):
    """A 64 x 96 frame through ``simulator_detections_from_frame`` with the half net: ``detector_input`` makes the half
    input in its one launch, and no launch of the profile is a cast or a copy."""
    from torch.profiler import ProfilerActivity, profile
    from gaussianrpg_amd import harness as hz
    from gaussianrpg_amd.perception import LetterboxPlan
    net, spec, sd, _, _ = _net("narrow_2x64x96")
    frame = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (64, 96, 3)).astype(np.uint8)).to(dev)
    plan = LetterboxPlan(64, 96, (64, 96), stride=32, device=dev)
    assert plan.out_shape == (64, 96)
    seen = []

    class Spy:                      # the net as the harness sees it: .dtype, .geometry and the call
        dtype, geometry = net.dtype, net.geometry

        def __call__(self, x):
            seen.append((x.dtype, tuple(x.shape), x.is_contiguous()))
            return net(x)

    want = hz.simulator_detections_from_frame(frame, Spy(), plan, conf_thres=0.05)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        got = hz.simulator_detections_from_frame(frame, Spy(), plan, conf_thres=0.05)
        torch.cuda.synchronize()
    assert seen == [(torch.float16, (1, 3, 64, 96), True)] * 2
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    print(sorted(set(n for n in names if "conv_f16_kernel" not in n)))
    assert sum("conv_f16_kernel" in n for n in names) == 62 and sum("spp_f16_kernel" in n for n in names) == 1
    assert sum("letterbox" in n for n in names) == 1
    # no cast and no copy between the letterbox launch and the network: torch's are elementwise / copy kernels
    assert [n for n in names if "conv_kernel" in n or "elementwise" in n or "copy_kernel" in n or "DtoD" in n] == [], names
    assert len(got) == len(want) == 1 and torch.equal(got[0], want[0])
