"""CPU tests (-m "not gpu") of the LPIPS backward's truth and contract (tests/lpips_bwd_truth.py,
gaussianrpg_amd/lpips.py ``LPIPS.loss``, csrc/lpips_bwd.hip): the conditional float64 chain with float64's own decisions
against plain float64 autograd; the recorded reference figures (tests/golden/ref_lpips_bwd.json) against a plain CPU
restatement; the acceptance bounds against eight planted errors (five in the
chain, three at a leaf) -- a bound that lets one of them through would prove
nothing on the GPU; a float32 CPU evaluation of every leaf inside its derived bound; the refusals that need no device;
the header's declarations, the library's exports and the pure size queries."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_bwd_truth as B
import lpips_truth as T
from gaussianrpg_amd import build
from gaussianrpg_amd import lpips as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_lpips_bwd.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
    if not os.path.exists(path):
        build.build_native()
    lib = ctypes.CDLL(path)
    for name in ("grpg_lpips_workspace_bytes", "grpg_lpips_train_workspace_bytes", "grpg_lpips_train_activation_offset",
                 "grpg_lpips_conv_bwd_packed_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
    return lib


_truths = {}


def truth(case):
    """the unconditional truth: float64's own decisions"""
    if case not in _truths:
        net, features, lin, x, y = T.case_inputs(case)
        _truths[case] = B.grad64(net, features, lin, x, y)
    return _truths[case]


# ---- the truth ----

@pytest.mark.parametrize("case", list(T.CASES))
def test_the_chain_with_float64s_own_decisions_is_float64_autograd(case):
    net, features, lin, x, y = T.case_inputs(case)
    gp = np.linspace(0.5, 1.5, x.shape[0])
    auto = B.autograd64(net, features, lin, x, y, gp)
    rel, worst = B.figures(B.grad64(net, features, lin, x, y, gp), auto)
    print(case, "chain against autograd: rel L2 %.2e, worst %.2e" % (rel, worst))
    assert rel < 1e-12 and float(auto.abs().max()) > 1e-5


def test_hashes_of_the_fixture(golden):
    assert sorted(golden["cases"]) == sorted(T.CASES)
    for case, row in golden["cases"].items():
        net, _, _, x, y = T.case_inputs(case)
        assert row["sha256_input"] == T.sha256(x, y) and row["sha256_weights"] == T.weights_hash(net)
        assert 1e-7 < row["rel_l2"] < 1e-4 and 0 < row["worst"] < 1e-4 * row["truth_max"]


@pytest.mark.parametrize("case", list(T.CASES))
def test_the_recorded_figures_reproduce_from_a_restatement(golden, case):
    net, features, lin, x, y = T.case_inputs(case)
    grad, acts = B.restatement32(net, features, lin, x, y)
    masks, winners = B.decisions_of(net, acts)
    rel, worst = B.figures(grad, B.grad64(net, features, lin, x, y, masks=masks, winners=winners))
    row = golden["cases"][case]
    print(case, "restatement rel L2 %.3e (recorded %.3e), worst %.3e (recorded %.3e)" % (rel, row["rel_l2"], worst, row["worst"]))
    assert row["rel_l2"] / 2 <= rel <= row["rel_l2"] * 2
    assert row["worst"] / 2 <= worst <= row["worst"] * 2


def test_first_maximum_is_max_pool2ds_winner():
    rs = np.random.RandomState(3)
    for k, hw in ((3, (7, 9)), (2, (5, 6)), (3, (16, 22))):
        act = torch.from_numpy(np.round(np.maximum(rs.normal(0, 1, (2, 3) + hw), 0) * 2) / 2)      # many ties
        _, idx = F.max_pool2d(act, k, 2, return_indices=True)
        assert torch.equal(B.first_max_index(act, k), idx)
        assert not torch.equal(B.last_max_index(act, k), idx)


# ---- the acceptance bound against planted errors ----

@pytest.mark.parametrize("variant", list(B.VARIANTS))
def test_acceptance_rejects_a_planted_error_in_the_chain(golden, variant):
    shown = 0
    for case, row in T.CASES.items():
        if row[0] not in B.VARIANTS[variant] or case not in ("alex_1x35x47", "vgg_1x16x16"):
            continue
        net, features, lin, x, y = T.case_inputs(case)
        acc = B.acceptance(golden["cases"][case], B.grad64(net, features, lin, x, y, variant=variant), truth(case))
        print(variant, case, acc)
        assert not B.within(acc)
        shown += 1
    assert shown == 2                # one case per net
    good = B.acceptance(golden["cases"]["alex_1x31x31"], truth("alex_1x31x31").float(), truth("alex_1x31x31"))
    assert B.within(good)            # ... while the truth rounded to float32 passes


def test_pool_bound_rejects_the_last_of_two_equal_maxima():
    rs = np.random.RandomState(5)
    act = np.maximum(rs.normal(0, 1, (1, 2, 7, 7)), 0).astype(np.float32)
    act[0, 0, 0, 1] = act[0, 0, 2, 2] = 5.0
    g = rs.normal(0, 1, (1, 2, 3, 3)).astype(np.float32)
    want, bound = B.pool_bwd(act, g, 3)
    wrong, _ = B.pool_bwd(act, g, 3, variant="pool_last_max")
    assert bool(((wrong - want).abs() > bound).any())
    assert bool(((B.pool_bwd(act, g, 3, dtype=torch.float32)[0].double() - want).abs() <= bound).all())


def test_conv_bound_rejects_the_relu_as_a_product_under_a_nan():
    rs = np.random.RandomState(6)
    g = rs.normal(0, 1, (1, 8, 4, 4)).astype(np.float32)
    w = rs.normal(0, 0.2, (8, 4, 3, 3)).astype(np.float32)
    act = np.maximum(rs.normal(0, 1, (1, 4, 4, 4)), 0).astype(np.float32)
    act[0, 1, 2, 2] = 0.0
    tap = rs.normal(0, 1, act.shape).astype(np.float32)
    tap[0, 1, 2, 2] = np.nan
    want, bound = B.conv_bwd(g, w, 3, 1, 1, (4, 4), mask=act > 0, tap=tap)
    assert float(want[0, 1, 2, 2]) == 0.0 and bool(torch.isfinite(want).all())
    wrong, _ = B.conv_bwd(g, w, 3, 1, 1, (4, 4), mask=act > 0, tap=tap, variant="relu_product")
    assert not bool(((wrong - want).abs() <= bound).all())       # the NaN fails the comparison


def test_conv_bound_rejects_a_gradient_in_rows_under_no_window():
    rs = np.random.RandomState(7)
    g = rs.normal(0, 1, (1, 64, 7, 8)).astype(np.float32)          # AlexNet's first layer at 34 x 38
    w = (rs.normal(0, 1, (64, 3, 11, 11)) * np.sqrt(2.0 / 363)).astype(np.float32)
    want, bound = B.conv_bwd(g, w, 11, 4, 2, (34, 38), std=True)
    assert not want[:, :, 33].any() and not want[:, :, :, 37].any() and not bound[:, :, 33].any()
    wrong, _ = B.conv_bwd(g, w, 11, 4, 2, (34, 38), std=True, variant="stride_remainder")
    assert bool(((wrong - want).abs() > bound).any()) and torch.equal(wrong[:, :, :33, :37], want[:, :, :33, :37])


# ---- float32 evaluations of the leaves inside their bounds ----

@pytest.mark.parametrize("c_out,c_in,k,s,p,hw,std", [(64, 3, 11, 4, 2, (34, 38), True), (192, 64, 5, 1, 2, (7, 7), False),
                                                      (384, 192, 3, 1, 1, (5, 7), False), (5, 64, 3, 1, 1, (6, 9), False)])
def test_a_float32_convolution_backward_lies_inside_its_bound(c_out, c_in, k, s, p, hw, std):
    rs = np.random.RandomState(c_out + k)
    ho, wo = (hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1
    g = rs.normal(0, 1, (2, c_out, ho, wo)).astype(np.float32)
    w = (rs.normal(0, 1, (c_out, c_in, k, k)) * np.sqrt(2.0 / (c_in * k * k))).astype(np.float32)
    act = np.maximum(rs.normal(0, 1, (2, c_in) + hw), 0).astype(np.float32)
    tap = rs.normal(0, 1, act.shape).astype(np.float32)
    kw = dict(std=True) if std else dict(mask=act > 0, tap=tap)
    want, bound = B.conv_bwd(g, w, k, s, p, hw, **kw)
    got, _ = B.conv_bwd(g, w, k, s, p, hw, dtype=torch.float32, **kw)
    ratio = float(((got.double() - want).abs()[bound > 0] / bound[bound > 0]).max())
    print("float32 conv backward k %d: worst err / bound %.3f" % (k, ratio))
    assert ratio <= 1.0 and bool((got[bound == 0] == 0).all())
    if std:
        assert not want[:, :, 33].any() and not want[:, :, :, 37].any()      # under no window: exactly 0 in the truth too


@pytest.mark.parametrize("c,hw", [(64, (7, 7)), (384, (3, 3)), (512, (1, 1))])
def test_a_float32_distance_backward_lies_inside_its_bound(c, hw):
    rs = np.random.RandomState(c)
    f = np.maximum(rs.normal(0, 1, (4, c) + hw), 0).astype(np.float32)
    f[0, :, 0, 0] = 0
    w = rs.uniform(0, 1, c).astype(np.float32)
    gp = np.asarray([0.7, -1.3], np.float32)
    want, bound = B.distance_bwd(f[:2], f[2:], w, gp)
    got, _ = B.distance_bwd(f[:2], f[2:], w, gp, dtype=torch.float32)
    ratio = float(((got.double() - want).abs()[bound > 0] / bound[bound > 0]).max())
    print("float32 distance backward C %d: worst err / bound %.3f" % (c, ratio))
    assert ratio <= 1.0 and not want[0, :, 0, 0].any() and bool(torch.isfinite(want).all())
    # the formula is the derivative: float64 autograd of the forward's s, behind the ReLU's select
    fx = T.t64(f[:2]).clone().requires_grad_(True)
    keep = torch.ones(2, 1, hw[0], hw[1], dtype=torch.bool)
    keep[0, 0, 0, 0] = False                                       # autograd's sqrt'(0) is not finite there
    s = (T.t64(w).reshape(1, -1, 1, 1) * (T.normalize64(fx) - T.normalize64(T.t64(f[2:]))) ** 2).sum(1, keepdim=True)
    auto, = torch.autograd.grad((torch.where(keep, s, torch.zeros_like(s)).mean((1, 2, 3)) * T.t64(gp)).sum(), fx)
    auto = torch.where((fx > 0) & keep, auto, torch.zeros_like(auto))
    assert torch.allclose(auto, want, rtol=1e-9, atol=1e-15)


# ---- refusals that need no device ----

def test_refusals_without_a_device():
    crit = LP.LPIPS("alex", T.build_features("alex"), T.build_lin("alex"), device=None) if not torch.cuda.is_available() \
        else LP.LPIPS("alex", T.build_features("alex"), T.build_lin("alex"))
    x = torch.rand(1, 3, 40, 40)
    with pytest.raises(ValueError, match="x only"):
        crit.loss(x.clone().requires_grad_(True), x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="too small"):
        crit.loss(x[:, :, :30].contiguous().requires_grad_(True), x[:, :, :30].contiguous())
    with pytest.raises(ValueError, match="too small"):
        crit.train_activations(x[:, :, :, :30].contiguous(), x[:, :, :, :30].contiguous())
    with pytest.raises(ValueError, match="no CPU path"):
        crit.loss(x.clone().requires_grad_(True), x)
    with pytest.raises(TypeError, match="float32"):
        crit.loss(x.double().requires_grad_(True), x.double())
    with pytest.raises(ValueError, match="reduction"):
        LP.lpips_loss(x, x, crit, "max")
    with pytest.raises(TypeError, match="criterion"):
        LP.lpips_loss(x, x, None)


# ---- header, exports, size queries ----

NEW = ("grpg_lpips_train_workspace_bytes", "grpg_lpips_train_activation_offset", "grpg_lpips_forward_train",
       "grpg_lpips_conv_bwd_packed_bytes", "grpg_lpips_conv_bwd_pack_weights", "grpg_lpips_backward",
       "grpg_lpips_conv2d_backward_data", "grpg_lpips_max_pool_backward", "grpg_lpips_distance_backward")


def test_header_declares_and_library_exports_the_new_entry_points(lib):
    text = open(os.path.join(ROOT, "include", "grpg_rasterizer.h")).read()
    declared = set(re.findall(r"GRPG_API\s+[\w\s\*]+?\b(grpg_\w+)\s*\(", text))
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+GRPG_ABI_VERSION\s+7\b", text)


def test_size_queries_are_pure(lib):
    for case, (net, pairs, h, w, _) in T.CASES.items():
        n = LP.NETS[net]
        P = LP.shape_plan(net, pairs, h, w)
        total = lib.grpg_lpips_train_workspace_bytes(n, pairs, h, w)
        convs = [s for s in P["steps"] if s["kind"] == "conv"]
        kept = sum(4 * 2 * pairs * s["c_out"] * s["hw_out"][0] * s["hw_out"][1] for s in convs)
        assert total % 256 == 0 and total > kept                  # every convolution's output of both sides is kept
        offs = [lib.grpg_lpips_train_activation_offset(n, pairs, h, w, i) for i in range(len(convs))]
        assert all(o % 256 == 0 and o > 0 for o in offs) and offs == sorted(offs)
        ends = offs[1:] + [total]
        assert all(e - o >= 4 * 2 * pairs * s["c_out"] * s["hw_out"][0] * s["hw_out"][1] for o, e, s in zip(offs, ends, convs))
        assert lib.grpg_lpips_train_activation_offset(n, pairs, h, w, len(convs)) == 0
        assert P["backward_launches"]["total"] == (12 if net == "alex" else 22)
    for net, least in ((0, 31), (1, 16)):                          # refused exactly where the forward refuses
        for h, w in ((least - 1, 64), (64, least - 1), (0, 0)):
            assert lib.grpg_lpips_train_workspace_bytes(net, 1, h, w) == 0
    assert lib.grpg_lpips_train_workspace_bytes(0, 0, 64, 64) == 0 and lib.grpg_lpips_train_workspace_bytes(2, 1, 64, 64) == 0
    assert lib.grpg_lpips_train_workspace_bytes(1, 1, 32768, 32768) == 0
    # the backward layouts: [K_pad][M_pad] at stride 1, [C_out k k][4] for the strided layer; nothing else is covered
    assert lib.grpg_lpips_conv_bwd_packed_bytes(192, 64, 5, 1) == 4 * 128 * 4800
    assert lib.grpg_lpips_conv_bwd_packed_bytes(5, 192, 3, 1) == 4 * 256 * 48
    assert lib.grpg_lpips_conv_bwd_packed_bytes(64, 3, 11, 4) == 4 * 4 * 64 * 121
    for args in ((64, 3, 11, 1), (64, 8, 11, 4), (64, 64, 3, 2), (64, 64, 7, 1), (0, 3, 3, 1)):
        assert lib.grpg_lpips_conv_bwd_packed_bytes(*args) == 0


def test_null_pointers_are_errors(lib):
    lib.grpg_last_error.restype = ctypes.c_char_p
    assert lib.grpg_lpips_backward(0, None, None, None, None, None, 1, 64, 64, None) == -1
    assert b"NULL" in lib.grpg_last_error()
    assert lib.grpg_lpips_forward_train(0, None, None, None, None, 1, 64, 64, None, None, None, None) == -1
    assert lib.grpg_lpips_conv2d_backward_data(None, None, None, None, None, 1, 3, 3, 4, 4, 3, 1, 1, None, 0, None) == -1
    assert lib.grpg_lpips_max_pool_backward(None, None, None, None, ctypes.c_longlong(1), 4, 4, 2, None) == -1
    assert lib.grpg_lpips_distance_backward(None, None, None, 1, 64, 4, None, None) == -1
