"""GPU tests of the detector's network (gaussianrpg_amd/detector.py, csrc/detector.hip).  Every comparison is against a
truth computed on the CPU (tests/detector_truth.py); no torch convolution runs on the device.

1. The convolution leaf against float64 within the derived per-element bound (detector_truth's docstring), at the
   smallest shapes at which each mechanism can go wrong, always inside wider tensors whose other channels hold a
   sentinel that must survive bit for bit, and with BOTH tile shapes: the chain of an output element is the same in
   both (blocks of 32 k, the block sums added in order onto the bias), so their bits must be equal.
2. The pool leaf bit for bit.
3. The whole network: per head at most MARGIN x the reference's own recorded distance from the float64 truth
   (tests/golden/ref_detector.json), determinism, the second call's launches / waits / allocations, the two doors.
"""
import json
import os

import numpy as np
import pytest
import torch

import detector_truth as T
from gaussianrpg_amd import detector as D

pytestmark = pytest.mark.gpu
MARGIN = 4.0
SENTINEL = 12345.678


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _wide(dev, x, c0, extra):
    """x [bs, c, h, w] inside a [bs, c0 + c + extra, h, w] tensor of sentinels."""
    x = torch.as_tensor(x)
    t = torch.full((x.shape[0], c0 + x.shape[1] + extra, x.shape[2], x.shape[3]), SENTINEL, dtype=torch.float32)
    t[:, c0:c0 + x.shape[1]] = x
    return t.to(dev)


def _untouched(t, c0, c):
    rest = torch.cat((t[:, :c0], t[:, c0 + c:]), 1)
    return bool((rest == torch.tensor(SENTINEL, dtype=torch.float32)).all())


def run_conv(dev, x, w, b, k, s, act, res=None, focus=False, up=False, tile=D.TILE_64, offs=(2, 3, 1, 4)):
    """The kernel on x (stored layout) inside wider tensors; returns (out, up or None), both on the host, after checking
    every sentinel."""
    bs, _, h, wd = x.shape
    c_out, c_in = w.shape[0], w.shape[1]
    ic0, oc0, rc0, uc0 = offs
    xin = _wide(dev, x, ic0, 2)
    lh, lw = (h // 2, wd // 2) if focus else (h, wd)
    ho, wo = D.out_size(lh, k, s), D.out_size(lw, k, s)
    out = torch.full((bs, oc0 + c_out + 1, ho, wo), SENTINEL, dtype=torch.float32, device=dev)
    rt = None if res is None else _wide(dev, res, rc0, 1)
    ut = torch.full((bs, uc0 + c_out + 2, 2 * ho, 2 * wo), SENTINEL, dtype=torch.float32, device=dev) if up else None
    packed = D.pack_weights(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev))
    rec = D.conv_record(xin.data_ptr(), ic0, xin.shape[1], h, wd, out.data_ptr(), oc0, out.shape[1], packed.data_ptr(),
                        bs, c_in, c_out, k, s, act, res=None if rt is None else (rt.data_ptr(), rc0, rt.shape[1]),
                        up=None if ut is None else (ut.data_ptr(), uc0, ut.shape[1]), focus=focus, tile=tile)
    D.run_records([rec], xin)
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


def _case(seed, bs, c_in, c_out, k, hw, res=False, focus=False):
    rs = np.random.RandomState(seed)
    cx = c_in // 4 if focus else c_in
    x = rs.normal(0, 1, (bs, cx, hw[0], hw[1])).astype(np.float32)
    w = (rs.normal(0, 1, (c_out, c_in, k, k)) / np.sqrt(c_in * k * k)).astype(np.float32)
    b = rs.normal(0, 1, c_out).astype(np.float32)
    return x, w, b, rs


RATIOS = {}

# name: (bs, c_in, c_out, k, stride, (h, w), act, res, focus, up)
CONV_CASES = {
    "k1_K12_cout8_5x7": (1, 12, 8, 1, 1, (5, 7), True, False, False, False),
    "k3_K108_cout18_5x7_bs2_res": (2, 12, 18, 3, 1, (5, 7), True, True, False, False),        # a pixel tile over two images
    "k3_K4608_cout255_5x7_linear": (1, 512, 255, 3, 1, (5, 7), False, False, False, False),   # the long chain, 2 M blocks
    "k3_K108_cout8_1x1": (1, 12, 8, 3, 1, (1, 1), True, False, False, False),
    "k1_K12_cout255_1x1_bs2_linear_res": (2, 12, 255, 1, 1, (1, 1), False, True, False, False),
    "k3_s2_7x9_odd": (1, 12, 18, 3, 2, (7, 9), True, False, False, False),
    "k3_s2_8x8_bs2": (2, 12, 8, 3, 2, (8, 8), True, True, False, False),
    "k1_s2_7x9": (1, 12, 18, 1, 2, (7, 9), False, False, False, False),
    "focus_6x10_bs2": (2, 12, 8, 3, 1, (6, 10), True, False, True, False),
    "focus_s2_10x6": (1, 12, 18, 3, 2, (10, 6), True, False, True, False),
    "up_3x5_bs2": (2, 12, 18, 1, 1, (3, 5), True, False, False, True),
    "up_k3_res_3x5": (1, 8, 8, 3, 1, (3, 5), True, True, False, True),
    "k3_K108_cout18_20x13_bs2": (2, 12, 18, 3, 1, (20, 13), True, True, False, False),        # 520 pixels: 9 / 5 N blocks
    "k1_K130_cout130_9x15": (1, 130, 130, 1, 1, (9, 15), True, False, False, False),          # K tail 2, M tail 2, N 135
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_leaf(dev, name):
    bs, c_in, c_out, k, s, hw, act, res, focus, up = CONV_CASES[name]
    x, w, b, rs = _case(sum(map(ord, name)), bs, c_in, c_out, k, hw, focus=focus)
    lh, lw = (hw[0] // 2, hw[1] // 2) if focus else hw
    r = rs.normal(0, 1, (bs, c_out, D.out_size(lh, k, s), D.out_size(lw, k, s))).astype(np.float32) if res else None
    want, bound = T.conv64(x, w, b, k, s, act, r, focus)
    got = {}
    for tile in (D.TILE_128, D.TILE_64):
        out, upo = run_conv(dev, x, w, b, k, s, act, r, focus, up, tile)
        assert out.shape == want.shape
        ratio = float(((out.double() - want).abs() / bound).max())
        RATIOS["%s/tile%d" % (name, tile)] = ratio
        print("%s tile %s: worst err / bound %.3f" % (name, "128" if tile == D.TILE_128 else "64", ratio))
        assert ratio <= 1.0
        if up:
            assert torch.equal(upo, out.repeat_interleave(2, 2).repeat_interleave(2, 3))     # the stored values, 2 x 2
        got[tile] = out
    assert torch.equal(got[D.TILE_128], got[D.TILE_64])     # same order in both shapes: same bits


def test_conv_leaf_twice_gives_the_same_bits(dev):
    x, w, b, _ = _case(5, 2, 64, 40, 3, (9, 11))
    a, _ = run_conv(dev, x, w, b, 3, 1, True, tile=D.TILE_128)
    c, _ = run_conv(dev, x, w, b, 3, 1, True, tile=D.TILE_128)
    assert torch.equal(a, c)


def test_packed_weights_layout(dev):
    x, w, b, _ = _case(6, 1, 5, 3, 3, (2, 2))
    p = D.pack_weights(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)).cpu().view(-1, 128)
    assert p.shape[0] == 1 + 48                                   # bias row, K = 45 -> 48
    assert torch.equal(p[0, :3], torch.from_numpy(b)) and not p[0, 3:].any()
    assert torch.equal(p[1:46, :3], torch.from_numpy(w).reshape(3, 45).t()) and not p[46:].any() and not p[:, 3:].any()


# ---- pool ----

@pytest.mark.parametrize("bs,c,hw,negative", [(1, 3, (1, 1), False), (1, 3, (3, 4), False), (2, 2, (13, 13), False),
                                              (2, 4, (14, 20), False), (1, 3, (3, 4), True), (1, 2, (33, 17), True),
                                              (1, 2, (16, 32), False)])
def test_pool_leaf(dev, bs, c, hw, negative):
    x = T.build_tensor((bs, c, hw[0], hw[1]), 40 + hw[0] + hw[1] + negative, negative)
    want = T.pool64(torch.from_numpy(x))
    # SPP's layout: one tensor, the input slice in front of the three output slices, sentinels around
    cat = torch.full((bs, 1 + 4 * c + 2, hw[0], hw[1]), SENTINEL, dtype=torch.float32)
    cat[:, 1:1 + c] = torch.from_numpy(x)
    cat = cat.to(dev)
    D.run_records([D.pool_record(cat.data_ptr(), 1, cat.shape[1], cat.data_ptr(), 1 + c, cat.shape[1], bs, c, hw[0], hw[1])], cat)
    torch.cuda.synchronize()
    got = cat.cpu()
    assert torch.equal(got[:, 1:1 + c], torch.from_numpy(x)) and _untouched(got, 1, 4 * c)
    assert torch.equal(got[:, 1 + c:1 + 4 * c], want)
    if negative:
        assert float(got[:, 1 + c:1 + 4 * c].max()) < 0
    # and into a tensor of its own
    xin = _wide(dev, x, 2, 1)
    out = torch.full((bs, 3 * c + 3, hw[0], hw[1]), SENTINEL, dtype=torch.float32, device=dev)
    D.run_records([D.pool_record(xin.data_ptr(), 2, xin.shape[1], out.data_ptr(), 3, out.shape[1], bs, c, hw[0], hw[1])], xin)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 3:].cpu(), want) and _untouched(out, 3, 3 * c)


def test_binding_refuses_bad_records(dev):
    x = torch.zeros(1, 4, 4, 4, device=dev)
    rec = D.pool_record(x.data_ptr(), 0, 4, x.data_ptr(), 1, 4, 1, 1, 4, 4)
    rec[5] = 2                                                     # out slice [2, 5) of 4 channels
    with pytest.raises(RuntimeError, match="leaves its tensor"):
        D.run_records([rec], x)
    with pytest.raises(RuntimeError, match="records must be"):
        D.run_records(torch.zeros(1, 25, dtype=torch.int64), x)


# ---- the whole network ----

@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_detector.json")) as f:
        return json.load(f)


_nets = {}


def _net(case):
    if case not in _nets:
        spec, sd, x = T.case_inputs(case)
        heads64, _ = T.network64(spec, sd, x)        # the truth: once per case
        _nets[case] = (D.DetectorNet(spec, sd), spec, sd, x, heads64)
    return _nets[case]


@pytest.mark.parametrize("case", list(T.CASES))
def test_network_heads(dev, golden, case):
    net, spec, sd, x, heads64 = _net(case)
    row = golden["cases"][case]
    heads = net(torch.from_numpy(x).to(dev))
    torch.cuda.synchronize()
    assert len(heads) == spec.nl
    for l, (h, t) in enumerate(zip(heads, heads64)):
        assert h.dtype == torch.float32 and list(h.shape) == row["head_shapes"][l] and h.is_contiguous()
        d = T.rel_l2(h.cpu(), t)
        RATIOS["%s/head%d" % (case, l)] = d / row["heads"][l][0]
        print("%s head %d: rel L2 %.3e, the reference's %.3e, ratio %.2f" % (case, l, d, row["heads"][l][0], d / row["heads"][l][0]))
    for l in range(spec.nl):
        assert RATIOS["%s/head%d" % (case, l)] <= MARGIN


def test_network_both_tile_shapes_and_twice(dev):
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).to(dev)
    first = [h.clone() for h in net(xd)]
    again = [h.clone() for h in net(xd)]
    big = [h.clone() for h in net(xd, tile=D.TILE_128)]
    small = [h.clone() for h in net(xd, tile=D.TILE_64)]
    for a, b, c, d in zip(first, again, big, small):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_replan_and_back(dev):
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).to(dev)
    first = [h.clone() for h in net(xd)]
    other = net(torch.from_numpy(T.build_input(1, 96, 32, 9)).to(dev))
    assert [tuple(h.shape) for h in other] == [(1, 24, 12, 4), (1, 24, 6, 2), (1, 24, 3, 1)]
    assert net.plan(2, 64, 96, dev) is net.plan(2, 64, 96, dev) and len(net._plans) >= 2
    for a, b in zip(first, net(xd)):
        assert torch.equal(a, b)


def test_detections_equal_detections_from_heads(dev):
    from gaussianrpg_amd.perception import detections_from_heads
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).to(dev)
    det, count = net.detections(xd, conf_thres=0.05, max_det=50)
    det2, count2 = detections_from_heads(net(xd), net.geometry, conf_thres=0.05, max_det=50)
    assert torch.equal(det, det2) and torch.equal(count, count2)
    assert int(count.sum()) > 0 and net.stride.tolist() == [8.0, 16.0, 32.0]


def test_second_call_launches_only(dev):
    from torch.profiler import ProfilerActivity, profile
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).to(dev)
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
    assert len(names) == 63 and sum("spp_kernel" in n for n in names) == 1 and sum("conv_kernel" in n for n in names) == 62


def test_from_module_gives_the_same_bits(dev):
    net, spec, sd, x, _ = _net("narrow_2x64x96")
    xd = torch.from_numpy(x).to(dev)
    want = [h.clone() for h in net(xd)]
    other = D.DetectorNet.from_module(T.stand_in_model(spec, sd))
    for a, b in zip(want, other(xd)):
        assert torch.equal(a, b)
    with pytest.raises(TypeError, match="float32"):
        net(xd.half())
    with pytest.raises(ValueError, match="largest stride"):
        net(xd[:, :, :48].contiguous())
