"""CPU tests (-m "not gpu") of LPIPS (gaussianrpg_amd/lpips.py, csrc/lpips.hip): the shape plan and the workspace
arithmetic against the native size queries (pure queries: no device), the two state dicts in both key spellings, every
refusal that needs no device, the float64 truth against the fixture tests/golden/ref_lpips.json, and the acceptance
bounds of tests/lpips_truth.py against seven planted contract errors: bounds that let one of them through would prove
nothing on the GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lpips_truth as T
from gaussianrpg_amd import build, harness
from gaussianrpg_amd import lpips as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(T.GOLDEN, "ref_lpips.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
    if not os.path.exists(path):
        build.build_native()
    import torch  # noqa: F401  (loads the same libamdhip64 the extension will use)
    lib = ctypes.CDLL(path)
    for name in ("grpg_lpips_workspace_bytes", "grpg_lpips_workspace_map_offset", "grpg_lpips_conv_packed_bytes",
                 "grpg_lpips_distance_workspace_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
    return lib


_truths = {}


def truth(case, variant=None):
    key = (case, variant)
    if key not in _truths:
        net, features, lin, x, y = T.case_inputs(case)
        _truths[key] = T.truth64(net, features, lin, x, y, variant)
    return _truths[key]


# ---- tables, plan, arena ----

def test_the_packages_tables_are_the_written_out_stacks():
    for net in ("alex", "vgg"):
        assert LP.LAYERS[net] == T.LAYERS[net] and LP.TARGETS[net] == T.TARGETS[net] and LP.CHANNELS[net] == T.CHANNELS[net]
        assert all(T.LAYERS[net][i - 1][0] == "relu" for i in T.TARGETS[net])       # a tap is a ReLU's output
    assert LP.conv_indices("alex") == [0, 3, 6, 8, 10]
    assert LP.conv_indices("vgg") == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert len(T.LAYERS["alex"]) == 13 and len(T.LAYERS["vgg"]) == 31
    assert LP.MEAN == T.MEAN and LP.STD == T.STD


def test_launch_budget():
    a = LP.shape_plan("alex", 1, 64, 64)["launches"]
    v = LP.shape_plan("vgg", 1, 64, 64)["launches"]
    assert (a["conv"], a["pool"], a["distance"] + a["finish"], a["total"]) == (5, 2, 6, 13)
    assert (v["conv"], v["pool"], v["distance"] + v["finish"], v["total"]) == (13, 4, 6, 23)      # the fifth pool never runs


@pytest.mark.parametrize("case", list(T.CASES))
def test_shape_plan_and_arena_of_every_case(lib, golden, case):
    net, pairs, h, w, _ = T.CASES[case]
    P = LP.shape_plan(net, pairs, h, w)
    assert [list(t[1:]) for t in P["taps"]] == golden["cases"][case]["tap_shapes"]
    assert [t[0] for t in P["taps"]] == list(T.CHANNELS[net])
    assert [list(m.shape[1:]) for m in truth(case)["maps"]] == [list(t[1:]) for t in P["taps"]]
    # the arena: two activations of the largest layer, the maps, one slot per workgroup and pair; 256-byte aligned
    most = max(2 * pairs * s["c_out"] * s["hw_out"][0] * s["hw_out"][1] for s in P["steps"])
    assert P["act_bytes"] == -(-4 * most // 256) * 256 and P["map_offsets"][0] == 2 * P["act_bytes"]
    assert all(o % 256 == 0 for o in P["map_offsets"] + P["slot_offsets"])
    ends = P["map_offsets"][1:] + P["slot_offsets"][:1]
    assert all(e - o >= 4 * pairs * th * tw for o, e, (_, th, tw) in zip(P["map_offsets"], ends, P["taps"]))
    # ... and it is what the native call lays out
    n = LP.NETS[net]
    assert lib.grpg_lpips_workspace_bytes(n, pairs, h, w) == P["workspace_bytes"]
    assert [lib.grpg_lpips_workspace_map_offset(n, pairs, h, w, l) for l in range(5)] == P["map_offsets"]


def test_minimum_sizes_and_the_readme_resolution(lib):
    assert [t[1:] for t in LP.shape_plan("alex", 1, 31, 31)["taps"]] == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert [t[1:] for t in LP.shape_plan("vgg", 1, 16, 16)["taps"]] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    P = LP.shape_plan("alex", 1, 1066, 1600)
    assert P["steps"][0]["hw_out"] == (265, 399)                 # conv1: 399 x 265
    assert [s["hw_out"] for s in P["steps"] if s["kind"] == "pool"] == [(132, 199), (65, 99)]
    assert lib.grpg_lpips_workspace_bytes(0, 1, 1066, 1600) == P["workspace_bytes"]
    for net, least in (("alex", 31), ("vgg", 16)):
        for h, w in ((least - 1, 64), (64, least - 1), (0, 0)):
            with pytest.raises(ValueError, match="too small"):
                LP.shape_plan(net, 1, h, w)
            assert lib.grpg_lpips_workspace_bytes(LP.NETS[net], 1, h, w) == 0
    with pytest.raises(ValueError, match="pairs"):
        LP.shape_plan("alex", 0, 64, 64)
    assert lib.grpg_lpips_workspace_bytes(0, 0, 64, 64) == 0 and lib.grpg_lpips_workspace_bytes(2, 1, 64, 64) == 0
    # a layer of 2^31 pixels: VGG16's first at 2 x 1 x 32768 x 32768
    with pytest.raises(ValueError, match="2\\^31"):
        LP.shape_plan("vgg", 1, 32768, 32768)
    assert lib.grpg_lpips_workspace_bytes(1, 1, 32768, 32768) == 0
    assert lib.grpg_lpips_workspace_map_offset(0, 1, 64, 64, 5) == 0


def test_packed_bytes_query(lib):
    assert lib.grpg_lpips_conv_packed_bytes(64, 3, 11) == 4 * 128 * (368 + 1)        # K = 363 -> 368, M 64 -> 128
    assert lib.grpg_lpips_conv_packed_bytes(192, 64, 5) == 4 * 256 * (1600 + 1)
    assert lib.grpg_lpips_conv_packed_bytes(8, 8, 1) == 0 and lib.grpg_lpips_conv_packed_bytes(0, 3, 3) == 0
    assert lib.grpg_lpips_distance_workspace_bytes(2, 64, 257) == 256 and lib.grpg_lpips_distance_workspace_bytes(0, 64, 4) == 0
    assert lib.grpg_lpips_distance_workspace_bytes(1, 512, 8 * 65) == 512 and lib.grpg_lpips_distance_workspace_bytes(1, 769, 4) == 0
    assert [LP.distance_px(c) for c in (64, 192, 193, 384, 385, 512)] == [32, 32, 16, 16, 8, 8]


def test_the_unit_is_built_with_the_detectors_flags():
    assert build.HIP_UNITS["lpips.hip"] == build.HIP_UNITS["detector.hip"]
    assert "-ffp-contract=off" in build.HIP_UNITS["lpips.hip"] and "lpips.hip" in build.REMARK_UNITS


# ---- the state dicts ----

@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_both_key_spellings_of_both_state_dicts(net):
    features, lin = T.build_features(net), T.build_lin(net)
    want = LP.feature_parameters(net, features)
    assert len(want) == len(LP.conv_indices(net))
    whole = {"features." + k: v for k, v in features.items()}
    whole["classifier.1.weight"] = torch.zeros(2, 2)                     # the rest of the model is ignored
    for (w, b), (w2, b2), i in zip(want, LP.feature_parameters(net, whole), LP.conv_indices(net)):
        assert torch.equal(w, features["%d.weight" % i]) and torch.equal(b, features["%d.bias" % i])
        assert torch.equal(w, w2) and torch.equal(b, b2)
    a, b = LP.lin_parameters(net, lin), LP.lin_parameters(net, T.renamed(lin))
    assert sorted(T.renamed(lin)) == ["%d.1.weight" % l for l in range(5)]
    for l, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v) and list(u.shape) == [T.CHANNELS[net][l]]
        assert torch.equal(u, lin["lin%d.model.1.weight" % l].reshape(-1))
    crit = LP.LPIPS(net, whole, T.renamed(lin))
    assert crit.net_type == net and len(crit.params) == len(want) and len(crit.lin) == 5


def test_refusals_that_need_no_device():
    features, lin = T.build_features("alex"), T.build_lin("alex")
    with pytest.raises(ValueError, match="squeeze"):
        LP.LPIPS("squeeze", features, lin)
    with pytest.raises(ValueError, match="choose net_type"):
        LP.LPIPS("resnet", features, lin)
    with pytest.raises(ValueError, match="ships no weights"):
        LP.LPIPS("alex")
    with pytest.raises(KeyError, match="3.weight"):
        LP.LPIPS("alex", {k: v for k, v in features.items() if k != "3.weight"}, lin)
    with pytest.raises(ValueError, match="shape"):
        LP.LPIPS("vgg", features, lin)                                      # AlexNet's tensors under VGG16's keys
    with pytest.raises(KeyError, match="lin4"):
        LP.LPIPS("alex", features, {k: v for k, v in lin.items() if not k.startswith("lin4")})
    narrow = dict(lin)
    narrow["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match="192 channels"):
        LP.LPIPS("alex", features, narrow)
    with pytest.raises(TypeError, match="torch.Tensor"):
        LP.LPIPS("alex", dict(features, **{"0.bias": [0.0] * 64}), lin)
    crit = LP.LPIPS("alex", features, lin)
    x = torch.zeros(3, 40, 40)
    with pytest.raises(TypeError, match="torch.Tensor"):
        crit(x.numpy(), x)
    with pytest.raises(TypeError, match="float32"):
        crit(x.half(), x.half())
    with pytest.raises(TypeError, match="float32"):
        crit(x.double(), x.double())
    with pytest.raises(ValueError, match="same shape"):
        crit(x, torch.zeros(3, 40, 41))
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        crit(torch.zeros(1, 40, 40), torch.zeros(1, 40, 40))
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        crit(torch.zeros(40, 40), torch.zeros(40, 40))
    with pytest.raises(ValueError, match="too small"):
        crit(torch.zeros(3, 30, 40), torch.zeros(3, 30, 40))
    with pytest.raises(ValueError, match="contiguous"):
        crit(torch.zeros(3, 40, 80)[:, :, ::2], torch.zeros(3, 40, 80)[:, :, ::2])
    with pytest.raises(ValueError, match="no CPU path"):
        crit(x, x)
    with pytest.raises(TypeError, match="criterion"):
        LP.lpips(x, x, "alex")
    with pytest.raises(TypeError, match="criterion"):
        LP.image_metrics(x, x, None)


# ---- truth and fixture ----

def test_fixture_hashes_match_the_generators(golden):
    assert sorted(golden["cases"]) == sorted(T.CASES)
    for net in ("alex", "vgg"):
        assert golden["nets"][net]["sha256_weights"] == T.weights_hash(net)
    for case, (net, pairs, h, w, seed) in T.CASES.items():
        x, y = T.build_pair(pairs, h, w, seed)
        row = golden["cases"][case]
        assert row["sha256_input"] == T.sha256(x, y) and (row["net"], row["pairs"], row["h"], row["w"]) == (net, pairs, h, w)
        assert float(np.abs(x * 255 - np.round(x * 255)).max()) < 1e-4 and float(np.abs(y * 255 - np.round(y * 255)).max()) < 1e-4
        assert x.min() >= 0 and y.max() <= 1 and float(np.abs(x - y).mean()) > 0.03


@pytest.mark.parametrize("case", list(T.CASES))
def test_live_truth_agrees_with_the_recorded_truth(golden, case):
    t, row = truth(case), golden["cases"][case]
    for got, want in ((t["values"], row["truth_values"]), (t["taps"], row["truth_taps"])):
        got, want = np.asarray(got.tolist()), np.asarray(want)
        assert got.shape == want.shape and float(np.abs(got / want - 1).max()) <= 1e-10
    assert abs(t["total"] / row["truth_total"] - 1) <= 1e-10
    # the reference's float32 result lies within ITS budget of the truth: the triangle inequality of the value bound
    assert abs(row["reference"] - row["truth_total"]) <= row["pairs"] * sum(golden["nets"][row["net"]]["map_mean_abs"]) * T.MARGIN
    assert float(t["taps"].min()) > 0                                          # no degenerate tap


def test_about_half_of_every_taps_activations_are_alive():
    for case in ("alex_2x67x93", "vgg_2x24x40"):
        net, features, lin, x, y = T.case_inputs(case)
        for l, f in enumerate(T.features64(net, features, x)):
            alive = float((f > 0).double().mean())
            assert 0.2 <= alive <= 0.8, (case, l, alive)


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_the_torch_route_computes_the_truth(golden, net):
    """harness.lpips_torch in float64 IS the truth (another walk of the same tables), and in float32 it is as close to
    it as the reference's modules."""
    case = "alex_2x67x93" if net == "alex" else "vgg_2x24x40"
    _, features, lin, x, y = T.case_inputs(case)
    t = truth(case)
    v64, maps64 = harness.lpips_torch(net, features, lin, dtype=torch.float64, per_tap=True)(torch.from_numpy(x), torch.from_numpy(y))
    assert list(v64.shape) == [1, 1, 1, 1] and abs(float(v64) / t["total"] - 1) <= 1e-12
    for m, want in zip(maps64, t["maps"]):
        assert T.rel_l2(m[:, 0], want) <= 1e-12
    v32, maps32 = harness.lpips_torch(net, features, T.renamed(lin), per_tap=True)(torch.from_numpy(x), torch.from_numpy(y))
    assert v32.dtype == torch.float32
    acc = T.acceptance(net, golden, {case: ([m[:, 0] for m in maps32], torch.stack([m.mean((1, 2, 3)) for m in maps32], 1).sum(1), t)})
    assert T.within(acc), acc


# ---- the bounds discriminate ----

@pytest.mark.parametrize("variant", list(T.VARIANTS))
def test_acceptance_bounds_catch_a_planted_contract_error(golden, variant):
    nets = [T.VARIANTS[variant]] if T.VARIANTS[variant] else ["alex", "vgg"]
    for net in nets:
        cases = [T.VGG_POOL5_CASE] if variant == "vgg_fifth_pool" else [c for c, row in T.CASES.items() if row[0] == net]
        results = {}
        for case in cases:
            wrong, right = truth(case, variant), truth(case)
            results[str(case)] = (wrong["maps"], wrong["values"], right)
        acc = T.acceptance(net, golden, results)
        print(variant, net, "map ratios", ["%.3g" % r for r in acc["map_ratio"]],
              "worst value ratio %.3g" % max(r for v in acc["value_ratio"].values() for r in v))
        assert not T.within(acc)
        assert max(acc["map_ratio"]) > 100 * T.MARGIN          # and not by a hair
        # the truth itself passes with nothing to spare needed
        assert T.within(T.acceptance(net, golden, {k: (r["maps"], r["values"], r) for k, (_, _, r) in results.items()}))
