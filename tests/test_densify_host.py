"""CPU tests (-m "not gpu") of the fused densify-and-prune (gaussianrpg_amd/optim.py, csrc/densify.hip): the tests'
float64 statement (tests/densify_truth.py) against the harness's restatement of the reference's PyTorch sequence run
in float64 with the same noise, the margin builder for every seed the GPU tests use, the C entries' size query and
loud failure without a device, and every refusal of the Python layer."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import densify_truth as truth
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.optim import DensifyModel, DensifyRule, FusedAdam, densify_and_prune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")

SPHERE = dict(sphere_center=(1.0, -2.0, 0.5), sphere_radius=6.0)
BOX = dict(box_min=(-1.4, -1.2, -1.6), box_max=(1.5, 1.3, 1.1))


def rules():
    """name -> (rule, xyz scale of the drawn inputs): the rules the GPU tests use."""
    base = truth.default_rule_values()
    return {
        "plain": (DensifyRule(prune_big=True, **base), 1.0),
        "plain_nobig": (DensifyRule(prune_big=False, **base), 1.0),
        "sphere": (DensifyRule(prune_big=True, **SPHERE, **base), 1.0),
        "box": (DensifyRule(prune_big=True, **BOX, **base), 0.07),
        "box_nobig": (DensifyRule(prune_big=False, **BOX, **base), 0.07),
    }


# (P, width set, rule, seed) of every input the GPU tests build (tests/test_gpu_densify.py imports this table)
GPU_CASES = [(P, w, "sphere" if w == "deg1" else "box", 100 + k)
             for w in ("deg1", "wide") for k, P in enumerate((1, 2, 255, 256, 257, 4097))]
GPU_CASES += [(600, "deg1", r, 200 + k) for k, r in enumerate(("plain", "plain_nobig", "sphere", "box", "box_nobig"))]
GPU_CASES += [(5000, "deg1", "sphere", 300)] + [(300, "deg1", ("box", "plain", "box_nobig")[k % 3], 301 + k)
                                                for k in range(10)]
GPU_CASES += [(1000, "deg1", "sphere", 400), (513, "wide", "box", 401)]


def _as_torch(rows, dtype):
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype) for k, v in rows.items()}


@pytest.mark.parametrize("rule_name", ["plain", "sphere", "box", "plain_nobig", "box_nobig"])
@pytest.mark.parametrize("col", [0, 1])
def test_truth_equals_reference_sequence_in_float64(rule_name, col):
    rule, scale = rules()[rule_name]
    rule = copy.copy(rule)
    rule.grad_column = col
    P = 700
    rows, _ = truth.build_inputs(P, truth.WIDTHS["wide"], rule, 7, xyz_scale=scale)
    rng = np.random.default_rng(8)
    params = {k: rows[k] for k in truth.GROUPS}
    m = {k: rng.standard_normal(v.shape) for k, v in params.items() if k != "f_dc"}      # f_dc: no state yet
    v = {k: rng.random(a.shape) for k, a in m.items()}
    t = truth.evaluate(params, rows["accum"], rows["denom"], rows["split_noise"], rows["box_noise"], rule, m, v)
    tr = _as_torch(rows, torch.float64)
    ref = hz.densify_and_prune_reference(
        {k: tr[k] for k in truth.GROUPS}, {k: (torch.from_numpy(m[k]), torch.from_numpy(v[k])) for k in m},
        tr["accum"], tr["denom"], rule, tr["split_noise"], tr["box_noise"])
    assert np.array_equal(ref["src_index"].numpy(), t.src_index)
    for key in ("points_total", "points_clone", "points_split", "points_below_min_opacity", "points_big_ws",
                "points_pruned"):
        assert ref["scalars"][key] == t.counts[key], key
    n = t.counts["n_out"]
    assert t.counts["points_clone"] > 50 and t.counts["points_split"] > 50 and 0 < t.counts["points_pruned"]
    assert min(t.counts["stream"]) > 0
    for name in truth.GROUPS:
        got = ref["tensors"][name].numpy()
        assert got.shape == t.values[name].shape == (n,) + truth.WIDTHS["wide"][name]
        assert truth.rel_l2(got, t.values[name]) <= 1e-12, name
        if name in m:
            assert np.array_equal(ref["moments"][name][0].numpy(), t.exp_avg[name])
            assert np.array_equal(ref["moments"][name][1].numpy(), t.exp_avg_sq[name])
        else:
            assert name not in ref["moments"]
    assert ref["xyz_gradient_accum"].shape == (n, 2) and ref["denom"].shape == (n, 1)
    assert ref["max_radii2D"].shape == (n,) and not ref["xyz_gradient_accum"].any()
    # the rules bite: the box noise slots differ, the sphere exempts, prune_big off keeps the big rows
    if rule_name == "box":
        assert (t.pruned[0] != t.pruned[1])[t.clone].any()
    if rule_name == "sphere":
        plain = truth.evaluate(params, rows["accum"], rows["denom"], rows["split_noise"], rows["box_noise"],
                               rules()["plain"][0])
        assert plain.counts["points_big_ws"] > t.counts["points_big_ws"] > 0
    if rule_name.endswith("nobig"):
        assert t.counts["points_big_ws"] == 0 and t.counts["points_pruned"] == t.counts["points_below_min_opacity"]


def test_special_rows_of_the_truth():
    """0 / 0 is not selected; accum > 0 over denom = 0 is (the reference's inf >= max_grad)."""
    rule, _ = rules()["plain"]
    rows, _ = truth.build_inputs(400, truth.WIDTHS["deg1"], rule, 9)
    zero = rows["denom"].reshape(-1) == 0
    nan_rows = zero & (rows["accum"][:, 0] == 0)
    inf_rows = zero & (rows["accum"][:, 0] > 0)
    assert nan_rows.sum() > 3 and inf_rows.sum() > 3
    t = truth.evaluate({k: rows[k] for k in truth.GROUPS}, rows["accum"], rows["denom"], rows["split_noise"],
                       rows["box_noise"], rule)
    assert not (t.clone | t.split)[nan_rows].any() and (t.clone | t.split)[inf_rows].all()


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "%d-%s-%s-%d" % c)
def test_margin_builder_leaves_no_fragile_row(case):
    P, widths, rule_name, seed = case
    rule, scale = rules()[rule_name]
    rows, redrawn = truth.build_inputs(P, truth.WIDTHS[widths], rule, seed, xyz_scale=scale)   # asserts none remains
    for col in (0, 1):
        r = copy.copy(rule)
        r.grad_column = col
        t = truth.evaluate({k: rows[k] for k in truth.GROUPS}, rows["accum"], rows["denom"], rows["split_noise"],
                           rows["box_noise"], r)
        assert (t.margin >= truth.MARGIN).all()
    assert redrawn <= 0.2 * P + 5
    again, _ = truth.build_inputs(P, truth.WIDTHS[widths], rule, seed, xyz_scale=scale)
    assert all(np.array_equal(rows[k], again[k]) for k in rows)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    return ctypes.CDLL(LIB)


def test_workspace_bytes_needs_no_device(lib):
    lib.grpg_densify_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_densify_workspace_bytes.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]

    def size(*P):
        return lib.grpg_densify_workspace_bytes((ctypes.c_longlong * len(P))(*P), len(P))

    assert size(0) > 0 and size(0) == size(0)
    assert size(1) < size(257) < size(4097) < size(1_900_000)
    assert size(1_900_000) < 2 * 1_900_000                 # about a byte per row plus per-workgroup counters
    assert size(1_900_000, *([10_000] * 10)) > size(1_900_000)
    assert size(256) == size(1)                             # whole workgroups of 256 rows
    assert size(-1) == 0 and size(5, -2) == 0 and size(1 << 40) == 0
    assert lib.grpg_densify_workspace_bytes(None, 3) == 0
    assert lib.grpg_densify_workspace_bytes((ctypes.c_longlong * 1)(5), 0) == 0


def test_c_entries_fail_loudly_without_a_device(lib):
    lib.grpg_densify_plan.restype = ctypes.c_int
    lib.grpg_densify_apply.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    # without a device both calls fail with GRPG_ERR_NO_DEVICE before they look at their arguments; with one, a NULL
    # model table is GRPG_ERR_INVALID_ARGUMENT: loud either way, never a silent success
    want = -1 if torch.cuda.is_available() else -2
    assert lib.grpg_densify_plan(None, 2, None, None, None, None, None) == want
    if want == -2:
        assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_densify_apply(None, 2, None, None, None, None, None) == want
    if want == -2:
        assert b"no usable HIP device" in lib.grpg_last_error()


def _cpu_model(P=6, rule=None, cls=FusedAdam, dtype=torch.float32, drop=None, rows=None):
    g = torch.Generator().manual_seed(4)
    groups = []
    for name, tail in truth.WIDTHS["deg1"].items():
        if name == drop:
            continue
        n = (rows or {}).get(name, P)
        groups.append({"params": [torch.nn.Parameter(torch.randn((n,) + tail, generator=g).to(dtype))], "lr": 1e-3,
                       "name": name})
    opt = cls(groups, lr=0.0, eps=1e-15)
    rule = rule or DensifyRule(prune_big=True, **truth.default_rule_values())
    return DensifyModel(opt, torch.zeros(P, 2), torch.zeros(P, 1), rule)


def test_python_refusals():
    base = truth.default_rule_values()
    with pytest.raises(KeyError, match="no group named 'scaling'"):
        densify_and_prune([_cpu_model(drop="scaling")])
    with pytest.raises(ValueError, match="same P"):
        densify_and_prune([_cpu_model(rows={"f_rest": 5})])
    with pytest.raises(TypeError, match="float32"):
        densify_and_prune([_cpu_model(cls=torch.optim.Adam, dtype=torch.float64)])
    m = _cpu_model()
    m.xyz_gradient_accum = torch.zeros(6, 4)[:, ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        densify_and_prune([m])
    m = _cpu_model()
    g = m.optimizer.param_groups[1]
    g["params"][0] = torch.nn.Parameter(torch.zeros(6, 2, 3)[:, :1])
    with pytest.raises(RuntimeError, match="contiguous"):
        densify_and_prune([m])
    for bad in (0.0, -1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_grad"):
            densify_and_prune([_cpu_model(rule=DensifyRule(**dict(base, max_grad=bad), prune_big=True))])
    with pytest.raises(ValueError, match="box rule must set prune_big"):
        densify_and_prune([_cpu_model(rule=DensifyRule(**BOX, **base))])
    with pytest.raises(ValueError, match="box_min and box_max"):
        densify_and_prune([_cpu_model(rule=DensifyRule(box_min=(0, 0, 0), prune_big=True, **base))])
    with pytest.raises(ValueError, match="grad_column"):
        densify_and_prune([_cpu_model(rule=DensifyRule(grad_column=2, prune_big=True, **base))])
    with pytest.raises(TypeError, match="FusedAdam or torch.optim.Adam"):
        densify_and_prune([_cpu_model(cls=lambda groups, lr, eps: torch.optim.SGD(groups, lr=lr))])
    # everything else in order, the tensors on the host: refused by name, with no fallback; nothing has changed
    for cls in (FusedAdam, torch.optim.Adam):
        m = _cpu_model(cls=cls)
        before = [g["params"][0] for g in m.optimizer.param_groups]
        with pytest.raises(RuntimeError, match="no CPU path"):
            densify_and_prune([m])
        assert all(a is g["params"][0] for a, g in zip(before, m.optimizer.param_groups))
    assert densify_and_prune([]) == []


def test_rule_constructors_mirror_the_reference_classes():
    bg = DensifyRule.background(0.0006, 0.005, True, scene_radius=30.0, sphere_center=[1, 2, 3], sphere_radius=12.5,
                                grad_abs=True)
    assert (bg.extent, bg.grad_column, bg.prune_big, bg.box_min) == (30.0, 1, True, None)
    assert bg.sphere_center == (1.0, 2.0, 3.0) and bg.sphere_radius == 12.5
    assert (bg.percent_dense, bg.percent_big_ws) == (0.01, 0.1)            # config.py:57, 67
    ac = DensifyRule.actor(0.0002, 0.005, False, extent=4.0, box_min=[-1, -2, -3], box_max=[1, 2, 3])
    assert (ac.extent, ac.grad_column, ac.prune_big, ac.sphere_center) == (4.0, 0, False, None)
    assert ac.box_min == (-1.0, -2.0, -3.0) and ac.box_max == (1.0, 2.0, 3.0)
    assert len(bg._row()) == len(ac._row()) == 19
