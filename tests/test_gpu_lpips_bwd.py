"""GPU tests of the LPIPS backward (gaussianrpg_amd/lpips.py ``LPIPS.loss``, csrc/lpips_bwd.hip).  Every comparison is
against a float64 truth computed on the CPU (tests/lpips_bwd_truth.py); no torch convolution runs on the device.

1. The three leaves against float64 within the bounds derived in lpips_bwd_truth's docstring: convolution
   backward-data (both tile shapes: the same bits; the strided first layer; the select with a NaN under a dead
   activation), the pool's gather (uncovered rows, equal maxima), the distance's derivative (all-zero vectors).
2. The whole nets on all six CASES: ``loss`` equals ``distances`` bit for bit, and the gradient lies within MARGIN x
   the reference's own recorded distance (tests/golden/ref_lpips_bwd.json) from the conditional truth at the HIP
   forward's own decisions; then determinism, batching, ``grad_pairs``, launches and allocations, and what stays
   detached.
"""
import json
import os

import numpy as np
import pytest
import torch

import lpips_bwd_truth as B
import lpips_truth as T
from gaussianrpg_amd import lpips as LP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_lpips_bwd.json")) as f:
        return json.load(f)


def worst_ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 (a deselected element) the value must be exactly the truth's"""
    got = got.double()
    dead = bound == 0
    assert torch.equal(got[dead], want[dead])
    err = (got - want).abs()[~dead] / bound[~dead]
    return float(err.max()) if err.numel() else 0.0


# ---- convolution backward-data ----

# name: (bs, c_out, c_in, k, stride, pad, (h_in, w_in), epilogue); "A to B" reads gradient channels -> produced channels
CONV_CASES = {
    "k11_s4_p2_64to3_31x31": (2, 64, 3, 11, 4, 2, (31, 31), "std"),
    "k11_s4_p2_64to3_34x38": (2, 64, 3, 11, 4, 2, (34, 38), "std"),        # row 33 and column 37 lie under no window
    "k5_192to64_3x3": (2, 192, 64, 5, 1, 2, (3, 3), "relu_tap"),
    "k5_192to64_7x7": (2, 192, 64, 5, 1, 2, (7, 7), "relu_tap"),
    "k3_384to192_1x5x7": (1, 384, 192, 3, 1, 1, (5, 7), "relu_tap"),       # M no multiple of 128, N = 35 below a tile
    "k3_512to512_2x2": (2, 512, 512, 3, 1, 1, (2, 2), "relu"),
    "k3_256to384_2x16x22": (2, 256, 384, 3, 1, 1, (16, 22), "relu_tap"),   # several tiles
    "k3_5to64_6x9": (2, 5, 64, 3, 1, 1, (6, 9), "plain"),                  # K = 45: no multiple of the block
    "k3_64to3_std_9x12": (2, 64, 3, 3, 1, 1, (9, 12), "std"),              # VGG16's first layer: the matrix path + 1 / std
}


def conv_inputs(name):
    bs, c_out, c_in, k, s, p, hw, epi = CONV_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    ho, wo = (hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1
    g = rs.normal(0, 1, (bs, c_out, ho, wo)).astype(np.float32)
    w = (rs.normal(0, 1, (c_out, c_in, k, k)) * np.sqrt(2.0 / (c_in * k * k))).astype(np.float32)
    act = np.maximum(rs.normal(0, 1, (bs, c_in, hw[0], hw[1])), 0).astype(np.float32)
    tap = rs.normal(0, 1, (bs, c_in, hw[0], hw[1])).astype(np.float32)
    return g, w, act, tap


def run_conv_bwd(dev, name, tile, g, w, act, tap):
    bs, c_out, c_in, k, s, p, hw, epi = CONV_CASES[name]
    packed = LP.pack_weights_bwd(torch.from_numpy(w).to(dev), s)
    out = LP.conv2d_backward_data(torch.from_numpy(g).to(dev), packed, c_in, hw, k, s, p,
                                  act=torch.from_numpy(act).to(dev) if epi.startswith("relu") else None,
                                  tap=torch.from_numpy(tap).to(dev) if epi == "relu_tap" else None, std=epi == "std", tile=tile)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_backward_leaf(dev, name):
    bs, c_out, c_in, k, s, p, hw, epi = CONV_CASES[name]
    g, w, act, tap = conv_inputs(name)
    want, bound = B.conv_bwd(g, w, k, s, p, hw, mask=act > 0 if epi.startswith("relu") else None,
                             tap=tap if epi == "relu_tap" else None, std=epi == "std")
    got = {}
    for tile in (LP.TILE_128, LP.TILE_64):
        out = run_conv_bwd(dev, name, tile, g, w, act, tap)
        assert list(out.shape) == [bs, c_in, hw[0], hw[1]] and out.dtype == torch.float32
        ratio = worst_ratio(out, want, bound)
        print("%s tile %s: worst err / bound %.3f" % (name, "128" if tile == LP.TILE_128 else "64", ratio))
        assert ratio <= 1.0
        got[tile] = out
    assert torch.equal(got[LP.TILE_128], got[LP.TILE_64])            # one summation order in both shapes
    assert float(want.abs().max()) > 0.1
    if name == "k11_s4_p2_64to3_34x38":
        assert not got[LP.TILE_64][:, :, 33].any() and not got[LP.TILE_64][:, :, :, 37].any()     # exactly 0
        assert bool(got[LP.TILE_64][:, :, :33, :37].abs().min() > 0)
    if name == "k11_s4_p2_64to3_31x31":
        assert bool(got[LP.TILE_64].abs().min() > 0)               # 31 = 4 * 6 + 11 - 4: every row lies under a window


def test_conv_backward_twice_gives_the_same_bits(dev):
    for name in ("k3_256to384_2x16x22", "k11_s4_p2_64to3_34x38"):
        args = conv_inputs(name)
        assert torch.equal(run_conv_bwd(dev, name, LP.TILE_128, *args), run_conv_bwd(dev, name, LP.TILE_128, *args))


@pytest.mark.parametrize("name", ["k5_192to64_7x7", "k3_384to192_1x5x7"])
def test_relu_select_stops_a_nan_under_a_dead_activation(dev, name):
    bs, c_out, c_in, k, s, p, hw, epi = CONV_CASES[name]
    g, w, act, tap = conv_inputs(name)
    act[0, 3, 2, 1] = 0.0
    tap[0, 3, 2, 1] = np.nan                   # a non-finite tap gradient under a dead activation
    act[0, 5, 1, 2] = 0.0
    g[0, 7, 1, 2] = np.inf                     # and a non-finite upstream gradient that reaches dead and live elements
    out = run_conv_bwd(dev, name, LP.TILE_64, g, w, act, tap)
    assert float(out[0, 3, 2, 1]) == 0.0 and float(out[0, 5, 1, 2]) == 0.0
    assert not bool(torch.isnan(out[torch.from_numpy(act) <= 0]).any()) and not out[torch.from_numpy(act) <= 0].any()
    assert bool((~torch.isfinite(out[0])).any())               # the live elements under the window do carry it
    if bs > 1:
        assert bool(torch.isfinite(out[1]).all())


def test_backward_packed_layouts(dev):
    rs = np.random.RandomState(8)
    w = rs.normal(0, 1, (3, 2, 5, 5)).astype(np.float32)
    p = LP.pack_weights_bwd(torch.from_numpy(w).to(dev), 1).cpu().view(-1, 128)
    assert p.shape[0] == 80                                        # K = 3 * 25 = 75 -> 80
    assert torch.equal(p[:75, :2], torch.from_numpy(w).permute(0, 2, 3, 1).reshape(75, 2)) and not p[75:].any() and not p[:, 2:].any()
    w = rs.normal(0, 1, (4, 3, 11, 11)).astype(np.float32)
    p = LP.pack_weights_bwd(torch.from_numpy(w).to(dev), 4).cpu().view(-1, 4)
    assert torch.equal(p[:, :3], torch.from_numpy(w).permute(0, 2, 3, 1).reshape(484, 3)) and not p[:, 3].any()
    with pytest.raises(RuntimeError, match="k 3 or 5 at stride 1"):
        LP.pack_weights_bwd(torch.zeros(4, 4, 3, 3, device=dev), 2)
    with pytest.raises(RuntimeError, match="k 3 or 5 at stride 1"):
        LP.pack_weights_bwd(torch.zeros(4, 8, 11, 11, device=dev), 4)


# ---- pool ----

def pool_inputs(k, hw, seed):
    rs = np.random.RandomState(seed)
    act = np.maximum(rs.normal(0, 1, (2, 3, hw[0], hw[1])), 0).astype(np.float32)
    ho, wo = (hw[0] - k) // 2 + 1, (hw[1] - k) // 2 + 1
    g = rs.normal(0, 1, (2, 3, ho, wo)).astype(np.float32)
    tap = rs.normal(0, 1, act.shape).astype(np.float32)
    return act, g, tap


@pytest.mark.parametrize("with_tap", [False, True])
@pytest.mark.parametrize("k,hw", [(3, (7, 7)), (3, (8, 11)), (3, (16, 22)), (2, (3, 5)), (2, (24, 40))])
def test_pool_backward_leaf(dev, k, hw, with_tap):
    act, g, tap = pool_inputs(k, hw, 50 + hw[0] + hw[1] + k)
    want, bound = B.pool_bwd(act, g, k, tap=tap if with_tap else None)
    got = LP.max_pool_backward(torch.from_numpy(act).to(dev), torch.from_numpy(g).to(dev), k,
                               tap=torch.from_numpy(tap).to(dev) if with_tap else None).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    ratio = worst_ratio(got, want, bound)
    print("pool k %d at %dx%d tap %s: worst err / bound %.3f" % (k, hw[0], hw[1], with_tap, ratio))
    assert ratio <= 1.0 and float(want.abs().max()) > 0.1
    assert not got[torch.from_numpy(act) <= 0].any()               # the select
    if (k, hw) == (2, (3, 5)) and not with_tap:
        assert not got[:, :, 2].any() and not got[:, :, :, 4].any()     # row 2 and column 4 lie under no window
    # every window's gradient arrives exactly once where its winner is alive
    if not with_tap:
        alive = torch.from_numpy(act).unfold(2, k, 2).unfold(3, k, 2).amax((-1, -2)) > 0
        assert torch.allclose(got.double().sum(), torch.from_numpy(g).double()[alive].sum(), rtol=1e-5, atol=1e-5)


def test_pool_backward_sends_equal_maxima_to_the_first(dev):
    act, g, tap = pool_inputs(3, (7, 7), 61)
    act[0, 0, 0:3, 0:3] = 0.25
    act[0, 0, 0, 1] = 5.0                      # window (0, 0): two equal positive maxima, (0, 1) before (2, 2)
    act[0, 0, 2, 2] = 5.0
    act[1, 2, 4:7, 4:7] = 7.0                  # window (2, 2): all nine equal
    got = LP.max_pool_backward(torch.from_numpy(act).to(dev), torch.from_numpy(g).to(dev), 3).cpu()
    want, bound = B.pool_bwd(act, g, 3)
    wrong, _ = B.pool_bwd(act, g, 3, variant="pool_last_max")
    assert worst_ratio(got, want, bound) <= 1.0
    assert float(got[0, 0, 0, 1]) == float(g[0, 0, 0, 0])          # (0, 1) lies in window (0, 0) only
    assert float(wrong[0, 0, 0, 1]) == 0.0 and not torch.equal(got.double(), wrong)
    # (4, 4) is the first 7 of every window that holds one; (6, 6) lies in window (2, 2) only and is its last
    assert float(got[1, 2, 6, 6]) == 0.0 and float(got[1, 2, 4, 4]) != 0.0


# ---- distance ----

def distance_inputs(c, hw, seed, pairs=2):
    rs = np.random.RandomState(seed)
    f = np.maximum(rs.normal(0, 1, (2 * pairs, c, hw[0], hw[1])), 0).astype(np.float32)      # a ReLU's output
    w = rs.uniform(0, 1, c).astype(np.float32)
    gp = np.asarray([0.7, -1.3], np.float32)[:pairs]
    return f, w, gp


def run_distance_bwd(dev, f, w, gp):
    out = LP.tap_distance_backward(torch.from_numpy(f).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(gp).to(dev))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (16, 22)])
@pytest.mark.parametrize("c", [64, 192, 384, 256, 512])
def test_distance_backward_leaf(dev, c, hw):
    f, w, gp = distance_inputs(c, hw, c + hw[0])
    want, bound = B.distance_bwd(f[:2], f[2:], w, gp)
    got = run_distance_bwd(dev, f, w, gp)
    assert list(got.shape) == [2, c, hw[0], hw[1]] and got.dtype == torch.float32
    ratio = worst_ratio(got, want, bound)
    print("distance backward C %d at %dx%d: worst err / bound %.3f" % (c, hw[0], hw[1], ratio))
    assert ratio <= 1.0 and float(want.abs().max()) > 0
    assert torch.equal(run_distance_bwd(dev, f, w, gp), got)       # the same bits twice


def test_distance_backward_of_all_zero_feature_vectors(dev):
    f, w, gp = distance_inputs(64, (7, 7), 99)
    f[0, :, 0, 0] = 0            # pair 0: x only
    f[2, :, 0, 1] = 0            # pair 0: y only
    f[0, :, 0, 2] = 0            # pair 0: both
    f[2, :, 0, 2] = 0
    want, bound = B.distance_bwd(f[:2], f[2:], w, gp)
    got = run_distance_bwd(dev, f, w, gp)
    assert bool(torch.isfinite(got).all())
    assert not got[0, :, 0, 0].any() and not got[0, :, 0, 2].any() and bool(got[0, :, 0, 1].any())
    assert worst_ratio(got, want, bound) <= 1.0


def test_distance_backward_is_linear_in_grad_pairs(dev):
    f, w, gp = distance_inputs(192, (7, 7), 17)
    one = run_distance_bwd(dev, f, w, gp)
    assert torch.equal(run_distance_bwd(dev, f, w, 2 * gp), 2 * one)                 # a power of two: the same bits
    want, bound = B.distance_bwd(f[:2], f[2:], w, 3 * gp)
    assert worst_ratio(run_distance_bwd(dev, f, w, 3 * gp), want, bound) <= 1.0
    zero = run_distance_bwd(dev, f, w, np.asarray([0.7, 0.0], np.float32))
    assert torch.equal(zero[0], one[0]) and not zero[1].any()


# ---- the whole nets ----

_crits, _runs = {}, {}


def crit_of(net):
    if net not in _crits:
        _crits[net] = LP.LPIPS(net, T.build_features(net), T.build_lin(net))
    return _crits[net]


def grad_of(crit, xd, yd, gp=None):
    xr = xd.clone().requires_grad_(True)
    val = crit.loss(xr, yd)
    g, = torch.autograd.grad(val, xr, torch.ones_like(val) if gp is None else gp)
    return val.detach(), g


def run_case(dev, case):
    """(values, gradient, conditional truth, x, y) of a fixture case: the device once, the float64 truth once."""
    if case not in _runs:
        net, features, lin, x, y = T.case_inputs(case)
        crit = crit_of(net)
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        acts = [a.cpu() for a in crit.train_activations(xd, yd)]
        val, g = grad_of(crit, xd, yd)
        masks, winners = B.decisions_of(net, acts)
        truth = B.grad64(net, features, lin, x, y, masks=masks, winners=winners)
        _runs[case] = (val.cpu(), g.cpu(), truth, xd, yd)
    return _runs[case]


@pytest.mark.parametrize("case", list(T.CASES))
def test_gradient_within_the_references_own_distance_from_the_truth(dev, golden, case):
    val, g, truth, xd, yd = run_case(dev, case)
    crit = crit_of(T.CASES[case][0])
    assert torch.equal(val, crit.distances(xd, yd).cpu())                            # bit for bit
    assert g.shape == xd.shape and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
    rel, worst = B.figures(g, truth)
    acc = B.acceptance(golden["cases"][case], g, truth)
    print("%s: rel L2 %.3e (reference %.3e, ratio %.2f), worst element %.3e (reference %.3e, ratio %.2f)"
          % (case, rel, golden["cases"][case]["rel_l2"], acc["rel_l2"], worst, golden["cases"][case]["worst"], acc["worst"]))
    assert acc["rel_l2"] <= B.MARGIN
    assert acc["worst"] <= B.MARGIN


def test_loss_is_a_fresh_tensor_and_the_functional_form_reduces_it(dev):
    _, g, _, xd, yd = run_case(dev, "alex_2x67x93")
    crit = crit_of("alex")
    xr = xd.clone().requires_grad_(True)
    a = crit.loss(xr, yd)
    kept = a.detach().clone()
    b = crit.loss(xr, -yd + 1)                                   # another call of the shape must not change `a`
    assert torch.equal(a.detach(), kept) and a.requires_grad and list(a.shape) == [2] and not torch.equal(a.detach(), b.detach())
    for red, ref in (("none", lambda v: v), ("sum", lambda v: v.sum()), ("mean", lambda v: v.mean())):
        assert torch.equal(LP.lpips_loss(xr, yd, crit, red).detach(), ref(crit.distances(xd, yd)))
    m = LP.lpips_loss(xr, yd, crit, "mean")
    gm, = torch.autograd.grad(m, xr)
    assert torch.equal(gm.cpu(), grad_of(crit, xd, yd, torch.full((2,), 0.5, device=dev))[1].cpu())
    with pytest.raises(ValueError, match="reduction"):
        LP.lpips_loss(xr, yd, crit, "max")


def test_two_identical_calls_give_identical_bits(dev):
    for case in ("alex_2x67x93", "vgg_2x24x40"):
        val, g, _, xd, yd = run_case(dev, case)
        val2, g2 = grad_of(crit_of(T.CASES[case][0]), xd, yd)
        assert torch.equal(val2.cpu(), val) and torch.equal(g2.cpu(), g)


def test_pairs_in_one_call_equal_single_pair_calls(dev):
    for case in ("alex_2x67x93", "vgg_2x24x40"):
        _, g, _, xd, yd = run_case(dev, case)
        for p in range(2):
            _, one = grad_of(crit_of(T.CASES[case][0]), xd[p:p + 1].contiguous(), yd[p:p + 1].contiguous())
            assert torch.equal(one.cpu()[0], g[p])


def test_non_uniform_grad_pairs_are_honoured(dev):
    _, g, _, xd, yd = run_case(dev, "alex_2x67x93")
    crit = crit_of("alex")
    _, got = grad_of(crit, xd, yd, torch.tensor([2.0, -0.5], device=dev))
    assert torch.equal(got.cpu()[0], 2 * g[0]) and torch.equal(got.cpu()[1], -0.5 * g[1])        # powers of two: exact
    _, got = grad_of(crit, xd, yd, torch.tensor([0.0, 1.0], device=dev))
    assert not got[0].any() and torch.equal(got.cpu()[1], g[1])


@pytest.mark.parametrize("net,case,convs,pools", [("alex", "alex_2x67x93", 5, 2), ("vgg", "vgg_2x24x40", 13, 4)])
def test_second_forward_and_backward_launch_only(dev, net, case, convs, pools):
    from torch.profiler import ProfilerActivity, profile
    _, _, _, xd, yd = run_case(dev, case)
    crit = crit_of(net)
    xr = xd.clone().requires_grad_(True)
    ones = torch.ones(2, device=dev)
    torch.autograd.grad(crit.loss(xr, yd), xr, ones)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        val = crit.loss(xr, yd)
        g, = torch.autograd.grad(val, xr, ones)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before + 2       # the two returned tensors
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        val = crit.loss(xr, yd)
        g, = torch.autograd.grad(val, xr, ones)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    assert [n for n in names if "memset" in n.lower()] == []
    count = lambda word: sum(word in n for n in names)
    assert (count("lpips_conv_kernel"), count("lpips_pool_kernel"), count("lpips_distance_kernel"), count("lpips_finish_kernel")) \
        == (convs, pools, 5, 1)
    assert (count("lpips_bwd_conv"), count("lpips_bwd_pool_kernel"), count("lpips_bwd_distance_kernel")) == (convs, pools, 5)
    assert count("lpips_bwd_conv_strided_kernel") == (1 if net == "alex" else 0)
    plan = LP.shape_plan(net, 2, xd.shape[2], xd.shape[3])
    assert count("lpips_bwd_") == convs + pools + 5 == plan["backward_launches"]["total"] == (12 if net == "alex" else 22)
    assert count("lpips_") == plan["launches"]["total"] + plan["backward_launches"]["total"]
    others = [n for n in names if "lpips_" not in n]                                  # the copy that makes `val` fresh
    assert len(others) <= 1 and all("copy" in n.lower() or "memcpy" in n.lower() for n in others), others


def test_second_backward_and_overwritten_activations_raise(dev):
    _, _, _, xd, yd = run_case(dev, "alex_1x35x47")
    crit = crit_of("alex")
    xr = xd.clone().requires_grad_(True)
    val = crit.loss(xr, yd)
    val.sum().backward()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        val.sum().backward()
    val = crit.loss(xr, yd)
    crit.loss(xr, yd)                                            # the shape's workspace now holds the later call
    with pytest.raises(RuntimeError, match="overwritten"):
        val.sum().backward()
    with pytest.raises(ValueError, match="x only"):
        crit.loss(xr, yd.clone().requires_grad_(True))


def test_train_activations_are_the_forwards_post_relu_outputs(dev):
    net, features, lin, x, y = T.case_inputs("vgg_1x16x16")
    crit = crit_of("vgg")
    acts = crit.train_activations(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    own = B.forward64(net, features, x)
    assert len(acts) == 13
    for a, w in zip(acts, own["acts"]):
        assert a.shape == w.shape and float(a.min()) >= 0 and torch.allclose(a.cpu().double(), w, rtol=1e-4, atol=1e-4)


def test_the_metric_entry_points_stay_detached(dev):
    _, _, _, xd, yd = run_case(dev, "alex_1x35x47")
    crit = crit_of("alex")
    xr = xd.clone().requires_grad_(True)
    for out in (crit.distances(xr, yd), crit.tap_terms(xr, yd), crit(xr, yd), LP.lpips(xr, yd, crit), crit.tap_maps(xr, yd)[0]):
        assert not out.requires_grad and out.grad_fn is None
    assert torch.equal(crit.distances(xr, yd), crit.loss(xr, yd).detach())
