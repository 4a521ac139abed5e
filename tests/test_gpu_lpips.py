"""GPU tests of LPIPS (gaussianrpg_amd/lpips.py, csrc/lpips.hip).  Every comparison is against a truth computed on the
CPU (tests/lpips_truth.py); no torch convolution runs on the device.

1. The convolution leaf (with the z-score gather, the ReLU, k in {3, 5, 11}) against float64 within the derived
   per-element bound, with BOTH tile shapes, whose bits must be equal; the pool leaf bit for bit against F.max_pool2d;
   the distance leaf against float64 within its derived bounds, with all-zero feature vectors.
2. The whole nets: the two acceptance bounds of lpips_truth's docstring on every fixture case -- measured against the
   reference's own recorded distance from the float64 truth (tests/golden/ref_lpips.json), never against this code --
   the reference's contract of ``forward``, batching, the second call's launches / waits / allocations,
   ``image_metrics`` and the refusals.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_truth as T
from gaussianrpg_amd import loss
from gaussianrpg_amd import lpips as LP

pytestmark = pytest.mark.gpu
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_lpips.json")) as f:
        return json.load(f)


# ---- convolution ----

# name: (bs, c_in, c_out, k, stride, pad, (h, w), zscore)
CONV_CASES = {
    "k11_s4_p2_z_31x31_bs2": (2, 3, 64, 11, 4, 2, (31, 31), True),
    "k11_s4_p2_z_35x47_bs2": (2, 3, 64, 11, 4, 2, (35, 47), True),
    "k5_p2_64to192_3x5_bs2": (2, 64, 192, 5, 1, 2, (3, 5), False),           # 192: one full and one partial M tile
    "k5_p2_64to192_7x10_bs4": (4, 64, 192, 5, 1, 2, (7, 10), False),         # 280 pixels: 5 / 3 N blocks
    "k3_192to384_1x1_bs2": (2, 192, 384, 3, 1, 1, (1, 1), False),
    "k3_192to384_1x2_bs2": (2, 192, 384, 3, 1, 1, (1, 2), False),
    "k3_192to384_3x4_bs2": (2, 192, 384, 3, 1, 1, (3, 4), False),
    "k3_384to256_1x1_bs2": (2, 384, 256, 3, 1, 1, (1, 1), False),
    "k3_384to256_1x2_bs2": (2, 384, 256, 3, 1, 1, (1, 2), False),
    "k3_384to256_3x4_bs2": (2, 384, 256, 3, 1, 1, (3, 4), False),
    "k3_K4608_512to8_3x4_bs2": (2, 512, 8, 3, 1, 1, (3, 4), False),          # the long chain
}


def conv_inputs(name):
    bs, c_in, c_out, k, s, p, hw, z = CONV_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    if z:
        x = (rs.randint(0, 256, (bs, c_in, hw[0], hw[1])).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    else:
        x = rs.normal(0, 1, (bs, c_in, hw[0], hw[1])).astype(np.float32)
    w = (rs.normal(0, 1, (c_out, c_in, k, k)) * np.sqrt(2.0 / (c_in * k * k))).astype(np.float32)
    b = rs.normal(0, 0.1, c_out).astype(np.float32)
    return x, w, b


def run_conv(dev, name, tile):
    bs, c_in, c_out, k, s, p, hw, z = CONV_CASES[name]
    x, w, b = conv_inputs(name)
    packed = LP.pack_weights(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev))
    xd = torch.from_numpy(x).to(dev)
    out = LP.conv2d_relu(xd, packed, c_out, k, s, p, zscore=z, tile=tile)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), torch.from_numpy(x)), "the input changed"
    return out.cpu()


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_leaf(dev, name):
    bs, c_in, c_out, k, s, p, hw, z = CONV_CASES[name]
    x, w, b = conv_inputs(name)
    want, bound = T.conv_relu64(x, w, b, k, s, p, z)
    got = {}
    for tile in (LP.TILE_128, LP.TILE_64):
        out = run_conv(dev, name, tile)
        assert out.shape == want.shape and out.dtype == torch.float32
        ratio = float(((out.double() - want).abs() / bound).max())
        RATIOS["%s/tile%d" % (name, tile)] = ratio
        print("%s tile %s: worst err / bound %.3f, alive %.2f" % (name, "128" if tile == LP.TILE_128 else "64", ratio,
                                                                   float((out > 0).float().mean())))
        assert ratio <= 1.0
        assert float(out.min()) >= 0.0 and 0.1 < float((out > 0).float().mean()) < 0.9       # a ReLU, and not a dead one
        got[tile] = out
    assert torch.equal(got[LP.TILE_128], got[LP.TILE_64])       # same order in both shapes: same bits


def test_conv_leaf_twice_gives_the_same_bits(dev):
    for tile in (LP.TILE_128, LP.TILE_64):
        assert torch.equal(run_conv(dev, "k5_p2_64to192_7x10_bs4", tile), run_conv(dev, "k5_p2_64to192_7x10_bs4", tile))


def test_relu_propagates_nan(dev):
    x, w, b = conv_inputs("k3_192to384_3x4_bs2")
    x[1, 5, 2, 3] = np.nan
    packed = LP.pack_weights(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev))
    out = LP.conv2d_relu(torch.from_numpy(x).to(dev), packed, 384, 3, 1, 1).cpu()
    want = F.relu(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), padding=1))
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and bool(torch.isnan(out).any()) and not bool(torch.isnan(out[0]).any())


def test_packed_weights_layout(dev):
    rs = np.random.RandomState(6)
    w, b = rs.normal(0, 1, (3, 2, 5, 5)).astype(np.float32), rs.normal(0, 1, 3).astype(np.float32)
    p = LP.pack_weights(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)).cpu().view(-1, 128)
    assert p.shape[0] == 1 + 64                                   # bias row, K = 50 -> 64
    assert torch.equal(p[0, :3], torch.from_numpy(b)) and not p[0, 3:].any()
    assert torch.equal(p[1:51, :3], torch.from_numpy(w).reshape(3, 50).t()) and not p[51:].any() and not p[:, 3:].any()


# ---- pool ----

@pytest.mark.parametrize("k,hw,negative", [(3, (7, 7), False), (3, (8, 11), False), (3, (16, 22), False), (2, (3, 5), False),
                                           (2, (24, 40), False), (3, (8, 11), True), (2, (3, 5), True)])
def test_pool_leaf(dev, k, hw, negative):
    rs = np.random.RandomState(40 + hw[0] + hw[1] + k)
    x = rs.normal(0, 1, (2, 3, hw[0], hw[1])).astype(np.float32)
    if negative:
        x = -np.abs(x) - np.float32(0.01)
    ho, wo = (hw[0] - k) // 2 + 1, (hw[1] - k) // 2 + 1
    ignored = (2 * (ho - 1) + k < hw[0], 2 * (wo - 1) + k < hw[1])
    if ignored[0]:
        x[:, :, 2 * (ho - 1) + k:] = 1e9           # floor mode: rows and columns no window reaches (row 15, column 21
    if ignored[1]:
        x[:, :, :, 2 * (wo - 1) + k:] = 1e9        # of 16 x 22) must not show
    want = F.max_pool2d(torch.from_numpy(x), k, 2)
    got = LP.max_pool(torch.from_numpy(x).to(dev), k).cpu()
    assert list(got.shape) == [2, 3, ho, wo] and torch.equal(got, want)
    assert float(got.max()) < 1e8
    if hw == (16, 22):
        assert ignored == (True, True)
    if negative:
        assert float(got.max()) < 0


# ---- distance ----

def distance_inputs(c, hw, seed, pairs=2):
    rs = np.random.RandomState(seed)
    f = np.maximum(rs.normal(0, 1, (2 * pairs, c, hw[0], hw[1])), 0).astype(np.float32)      # a ReLU's output
    w = rs.uniform(0, 1, c).astype(np.float32)
    return f, w


@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (16, 22)])
@pytest.mark.parametrize("c", [64, 192, 384, 256, 512])
def test_distance_leaf(dev, c, hw):
    f, w = distance_inputs(c, hw, c + hw[0])
    s64, m64, e_s, e_m = T.distance64(f[:2], f[2:], w)
    mean, smap = LP.tap_distance(torch.from_numpy(f).to(dev), torch.from_numpy(w).to(dev))
    torch.cuda.synchronize()
    mean, smap = mean.cpu().double(), smap.cpu().double()
    assert list(smap.shape) == [2, hw[0], hw[1]] and list(mean.shape) == [2]
    r_map, r_mean = float(((smap - s64).abs() / e_s).max()), float(((mean - m64).abs() / e_m).max())
    RATIOS["distance/c%d_%dx%d" % (c, hw[0], hw[1])] = (r_map, r_mean)
    print("distance C %d at %dx%d: worst map err / bound %.3f, mean err / bound %.3f" % (c, hw[0], hw[1], r_map, r_mean))
    assert r_map <= 1.0 and r_mean <= 1.0 and float(m64.min()) > 0


def test_distance_of_all_zero_feature_vectors(dev):
    f, w = distance_inputs(64, (7, 7), 99)
    f[0, :, 0, 0] = 0            # pair 0: x only
    f[2, :, 0, 1] = 0            # pair 0: y only
    f[0, :, 0, 2] = 0            # pair 0: both
    f[2, :, 0, 2] = 0
    s64, m64, e_s, e_m = T.distance64(f[:2], f[2:], w)
    mean, smap = LP.tap_distance(torch.from_numpy(f).to(dev), torch.from_numpy(w).to(dev))
    mean, smap = mean.cpu().double(), smap.cpu().double()
    assert bool(torch.isfinite(smap).all()) and bool(torch.isfinite(mean).all())
    assert float(smap[0, 0, 2]) == 0.0 and float(smap[0, 0, 0]) > 0 and float(smap[0, 0, 1]) > 0
    assert bool(((smap - s64).abs() <= e_s).all()) and bool(((mean - m64).abs() <= e_m).all())


def test_distance_twice_gives_the_same_bits(dev):
    f, w = distance_inputs(192, (16, 22), 7)
    fd, wd = torch.from_numpy(f).to(dev), torch.from_numpy(w).to(dev)
    a, b = LP.tap_distance(fd, wd), LP.tap_distance(fd, wd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the whole nets ----

_crits, _runs = {}, {}


def crit_of(net):
    if net not in _crits:
        _crits[net] = LP.LPIPS(net, T.build_features(net), T.build_lin(net))
    return _crits[net]


def run_case(dev, case):
    """(maps, values, taps, truth, x, y) of a fixture case: the device once, the float64 truth once."""
    if case not in _runs:
        net, features, lin, x, y = T.case_inputs(case)
        crit = crit_of(net)
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        maps = [m.cpu() for m in crit.tap_maps(xd, yd)]
        values, taps = crit.distances(xd, yd).cpu().clone(), crit.tap_terms(xd, yd).cpu().clone()
        _runs[case] = (maps, values, taps, T.truth64(net, features, lin, x, y), xd, yd)
    return _runs[case]


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_acceptance_bounds_on_every_fixture_case(dev, golden, net):
    results = {}
    for case, row in T.CASES.items():
        if row[0] == net:
            maps, values, taps, truth, _, _ = run_case(dev, case)
            assert [list(m.shape) for m in maps] == [list(m.shape) for m in truth["maps"]]
            results[case] = (maps, values, truth)
    acc = T.acceptance(net, golden, results)
    RATIOS["net/" + net] = acc
    print(net, "map rel L2 over the reference's, per tap:", ["%.2f" % r for r in acc["map_ratio"]])
    for case, v in acc["value_ratio"].items():
        print(case, "value error over the reference's summed mean absolute map error, per pair:", ["%.2f" % r for r in v],
              "value", results[case][1].tolist(), "reference", golden["cases"][case]["reference"])
    assert all(r <= T.MARGIN for r in acc["map_ratio"])
    assert all(r <= T.MARGIN for v in acc["value_ratio"].values() for r in v)


@pytest.mark.parametrize("case", list(T.CASES))
def test_forward_is_the_references_contract(dev, golden, case):
    maps, values, taps, truth, xd, yd = run_case(dev, case)
    crit = crit_of(T.CASES[case][0])
    out = crit(xd, yd)
    assert list(out.shape) == [1, 1, 1, 1] and out.dtype == torch.float32 and not out.requires_grad
    assert torch.equal(out.reshape(()), crit.distances(xd, yd).sum())
    assert torch.equal(LP.lpips(xd, yd, crit), out)
    assert torch.equal(crit.distances(xd, yd).cpu(), values)                         # a second call: the same bits
    acc = taps[:, 0]
    for l in range(1, 5):
        acc = acc + taps[:, l]
    assert torch.equal(acc, values)                                                  # the five terms in tap order
    for l, m in enumerate(maps):                                                     # a term is its map's mean
        assert torch.allclose(m.double().mean((1, 2)), taps[:, l].double(), rtol=22 * T.U, atol=0)   # D of lpips_truth
    if xd.shape[0] == 1:
        assert torch.equal(crit(xd[0], yd[0]), out)                                  # [3, H, W] is [1, 3, H, W]


def test_pairs_in_one_call_equal_single_pair_calls(dev):
    maps, values, taps, _, xd, yd = run_case(dev, "alex_2x67x93")
    crit = crit_of("alex")
    for p in range(2):
        one = crit.tap_maps(xd[p:p + 1].contiguous(), yd[p:p + 1].contiguous())
        assert torch.equal(crit.distances(xd[p], yd[p]).cpu(), values[p:p + 1])
        assert torch.equal(crit.tap_terms(xd[p], yd[p]).cpu(), taps[p:p + 1])
        for a, b in zip(one, maps):
            assert torch.equal(a.cpu()[0], b[p])
    maps, values, taps, _, xd, yd = run_case(dev, "vgg_2x24x40")
    for p in range(2):
        assert torch.equal(crit_of("vgg").tap_terms(xd[p], yd[p]).cpu(), taps[p:p + 1])


@pytest.mark.parametrize("net,case,convs,pools", [("alex", "alex_2x67x93", 5, 2), ("vgg", "vgg_2x24x40", 13, 4)])
def test_second_call_launches_only(dev, net, case, convs, pools):
    from torch.profiler import ProfilerActivity, profile
    _, _, _, _, xd, yd = run_case(dev, case)
    crit = crit_of(net)
    crit.distances(xd, yd)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        crit.distances(xd, yd)
        crit.tap_terms(xd, yd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before      # no allocation
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        crit.distances(xd, yd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    assert [n for n in names if "memcpy" in n.lower() or "memset" in n.lower()] == []
    count = lambda word: sum(word in n for n in names)
    assert (count("lpips_conv_kernel"), count("lpips_pool_kernel"), count("lpips_distance_kernel"), count("lpips_finish_kernel")) \
        == (convs, pools, 5, 1)
    assert len(names) == convs + pools + 6 == LP.shape_plan(net, 2, xd.shape[2], xd.shape[3])["launches"]["total"]


def test_image_metrics_equals_the_three_calls(dev):
    _, _, _, _, xd, yd = run_case(dev, "alex_1x35x47")
    crit = crit_of("alex")
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = LP.image_metrics(xd[0], yd[0], crit)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(m.shape) == [3] and m.is_cuda and not m.requires_grad
    want = torch.stack((loss.psnr(xd[0], yd[0]), loss.ssim(xd[0], yd[0]), crit.distances(xd[0], yd[0])[0]))
    assert torch.equal(m, want)
    assert 5 < float(m[0]) < 40 and 0 < float(m[1]) < 1 and 0 < float(m[2]) < 1


def test_binding_refuses(dev):
    crit = crit_of("alex")
    x = torch.rand(1, 3, 40, 40, device=dev)
    with pytest.raises(ValueError, match="too small"):
        crit(x[:, :, :30].contiguous(), x[:, :, :30].contiguous())
    with pytest.raises(ValueError, match="too small"):
        crit_of("vgg")(x[:, :, :15].contiguous(), x[:, :, :15].contiguous())
    with pytest.raises(TypeError, match="float32"):
        crit(x.half(), x.half())
    with pytest.raises(ValueError, match="no CPU path"):
        crit(x.cpu(), x.cpu())
    with pytest.raises(ValueError, match="no CPU path"):
        crit(x, x.cpu())
    with pytest.raises(ValueError, match="same shape"):
        crit(x, x[:, :, :39].contiguous())
    ext = LP._C()
    packed, lin = crit.packed(dev)
    ws = torch.empty(ext.lpips_workspace_bytes(0, 1, 40, 40), dtype=torch.uint8, device=dev)
    out, taps = torch.empty(1, device=dev), torch.empty(1, 5, device=dev)
    with pytest.raises(RuntimeError, match="192 channels"):
        ext.lpips_forward(0, packed, [lin[0], lin[0], lin[2], lin[3], lin[4]], x, x, ws, out, taps)
    with pytest.raises(RuntimeError, match="at least 31 x 31"):
        ext.lpips_forward(0, packed, lin, x[:, :, :30].contiguous(), x[:, :, :30].contiguous(), ws, out, taps)
    with pytest.raises(RuntimeError, match="float32"):
        ext.lpips_forward(0, packed, lin, x.half(), x.half(), ws, out, taps)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.lpips_forward(0, packed, lin, x.cpu(), x.cpu(), ws, out, taps)
    with pytest.raises(RuntimeError, match="workspace"):
        ext.lpips_forward(0, packed, lin, x, x, ws[:1024], out, taps)
    with pytest.raises(RuntimeError, match="13 packed"):
        ext.lpips_forward(1, packed, lin, x, x, ws, out, taps)
    with pytest.raises(RuntimeError, match="k must be 3, 5 or 11"):
        LP.pack_weights(torch.zeros(4, 4, 1, 1, device=dev))
    with pytest.raises(RuntimeError, match="k 2 or 3"):
        LP.max_pool(x, 4)
    # identical images: every term is exactly 0
    assert float(crit(x, x)) == 0.0
