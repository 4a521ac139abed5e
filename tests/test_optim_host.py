"""CPU tests (-m "not gpu") of the fused Adam step and the densification statistics (gaussianrpg_amd/optim.py,
csrc/optim.hip): the tests' float64 statement (tests/optim_truth.py) against torch.optim.Adam run in float64, the
C entries' size query and loud failure without a device, FusedAdam's refusals and its state-dict interchange with
torch.optim.Adam."""
import ctypes
import os

import numpy as np
import pytest
import torch

import optim_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
SHAPES = ((3,), (1, 3), (3, 3), (1,), (3,), (4,), (0,))     # per-Gaussian shapes of the reference's seven groups


def _grad_schedule(P, steps, seed):
    """Per group and step: a float64 gradient, None (the group is skipped at that step) or zeros."""
    rng = np.random.default_rng(seed)
    sched = []
    for k, tail in enumerate(SHAPES):
        per_step = []
        for s in range(steps):
            if k == 1 and s in (0, 1, 5, 6, 13):            # f_dc: no gradient on some steps, the first ones included
                per_step.append(None)
            elif k == 3:                                     # opacity: zero gradients from step 1 on
                per_step.append(np.zeros((P,) + tail))
            elif k == 4 and s < 3:                           # scaling: zero gradients first, then real ones
                per_step.append(np.zeros((P,) + tail))
            else:
                g = rng.standard_normal((P,) + tail) * 10.0 ** rng.uniform(-8, -2, (P,) + tail)
                g[rng.random((P,) + tail) < 0.3] = 0.0
                per_step.append(g)
        sched.append(per_step)
    return sched


def test_truth_equals_torch_adam_in_float64():
    P, steps = 257, 20
    rng = np.random.default_rng(5)
    p0 = [rng.standard_normal((P,) + tail) for tail in SHAPES]
    sched = _grad_schedule(P, steps, 6)
    params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p0]
    opt = torch.optim.Adam([{"params": [p], "lr": lr, "name": name}
                            for p, (name, lr) in zip(params, truth.REF_GROUPS)], lr=0.0, eps=truth.REF_EPS)
    for s in range(steps):
        for p, per_step in zip(params, sched):
            p.grad = None if per_step[s] is None else torch.from_numpy(per_step[s].copy())
        opt.step()
    for k, (p, a, per_step, (name, lr)) in enumerate(zip(params, p0, sched, truth.REF_GROUPS)):
        st = truth.adam(a, per_step, lr)
        if p.numel() == 0:
            continue
        assert int(opt.state[p]["step"]) == st.t == sum(g is not None for g in per_step), name
        for got, want, what in ((p.detach().numpy(), st.p, "p"), (opt.state[p]["exp_avg"].numpy(), st.m, "exp_avg"),
                                (opt.state[p]["exp_avg_sq"].numpy(), st.v, "exp_avg_sq"),
                                (p.detach().numpy() - a, st.p - st.p0, "displacement")):
            assert truth.rel_l2(got, want) <= 1e-12, (name, what, truth.rel_l2(got, want))
    # the skipped-step rule and the zero-gradient rule, spelled out
    assert truth.adam(p0[1], sched[1], 0.0025).t == steps - 5
    z = truth.adam(p0[3], sched[3], 0.05)
    assert np.array_equal(z.p, p0[3]) and not z.m.any() and not z.v.any() and z.t == steps


def test_truth_densify_loop_equals_vectorized():
    rng = np.random.default_rng(2)
    P, ranges = 40, [(0, 17), (17, 18), (20, 40)]
    grad = rng.standard_normal((P, 3))
    radii = rng.integers(0, 4, P)
    mk = lambda: ([np.zeros((e - s, 2)) for s, e in ranges], [np.zeros((e - s, 1)) for s, e in ranges],   # noqa: E731
                  [np.zeros(e - s) for s, e in ranges])
    a, b = mk(), mk()
    truth.densify(grad, radii, ranges, *a)
    truth.densify_vectorized(grad, radii, ranges, *b)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    assert a[1][0].sum() == (radii[:17] > 0).sum() and a[2][2].max() == radii[20:].max()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    return ctypes.CDLL(LIB)


class _Seg(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_longlong), ("step_size", ctypes.c_float),
                ("bc2_sqrt", ctypes.c_float), ("beta2", ctypes.c_float), ("one_minus_beta1", ctypes.c_float),
                ("one_minus_beta2", ctypes.c_float), ("eps", ctypes.c_float)]


def test_adam_workspace_bytes_needs_no_device(lib):
    lib.grpg_adam_workspace_bytes.restype = ctypes.c_size_t
    sizes = [lib.grpg_adam_workspace_bytes(n) for n in (0, 1, 7, 77, 1000)]
    assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] == 77 * sizes[1]
    assert lib.grpg_adam_workspace_bytes(-3) == 0


def test_c_entries_fail_loudly_without_a_device(lib):
    lib.grpg_adam_step.restype = ctypes.c_int
    lib.grpg_densify_stats.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    seg = _Seg(None, None, None, None, 0, 1e-3, 1.0, 0.999, 0.1, 0.001, 1e-15)
    # without a device every call fails with GRPG_ERR_NO_DEVICE before it looks at its arguments; with one, these
    # arguments (NULL tables) are GRPG_ERR_INVALID_ARGUMENT: loud either way, never a silent success
    want = -1 if torch.cuda.is_available() else -2
    assert lib.grpg_adam_step(None, 3, None, None, None) == want
    if want == -2:
        assert b"no usable HIP device" in lib.grpg_last_error()
        assert lib.grpg_adam_step(ctypes.byref(seg), 1, None, None, None) == -2
    assert lib.grpg_densify_stats(8, None, None, None, 1, None, None, None, None, None, None) == want
    if want == -2:
        assert b"no usable HIP device" in lib.grpg_last_error()


def _cpu_params(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn((5,) + tail, generator=g).to(dtype)) for tail in SHAPES]


def _groups(params):
    return [{"params": [p], "lr": lr, "name": name} for p, (name, lr) in zip(params, truth.REF_GROUPS)]


def test_fused_adam_refusals():
    from gaussianrpg_amd.optim import FusedAdam, densification_stats_update, fused_adam_step
    params = _cpu_params()
    opt = FusedAdam(_groups(params), lr=0.0, eps=1e-15)
    assert [g["name"] for g in opt.param_groups] == [n for n, _ in truth.REF_GROUPS]
    assert opt.param_groups[0]["lr"] == 1.6e-4 and opt.param_groups[0]["eps"] == 1e-15
    opt.step()                                    # no gradient anywhere: nothing to do, no state, no device needed
    assert len(opt.state) == 0
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_adam_step([opt, opt])
    assert len(opt.state) == 0                    # a refused step changes nothing
    with pytest.raises(ValueError, match="weight_decay"):
        FusedAdam(_groups(_cpu_params()), weight_decay=0.1)
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(_groups(_cpu_params()), amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedAdam(_groups(_cpu_params()), maximize=True)
    with pytest.raises(TypeError, match="float32"):
        FusedAdam(_groups(_cpu_params(torch.float64)))
    with pytest.raises(ValueError, match="betas"):
        FusedAdam(_groups(_cpu_params()), betas=(0.9, 1.0))
    opt.param_groups[0]["weight_decay"] = 0.01    # a group edited after construction is checked at the step
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()
    with pytest.raises(TypeError, match="FusedAdam instances"):
        fused_adam_step([torch.optim.Adam(_cpu_params())])
    with pytest.raises(RuntimeError, match="no CPU path"):
        densification_stats_update(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), [(0, 4)],
                                   [torch.zeros(4, 2)], [torch.zeros(4, 1)], [torch.zeros(4)])


def _fill_state(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for k, group in enumerate(opt.param_groups):
        for p in group["params"]:
            opt.state[p] = {"step": torch.tensor(float(3 + k)), "exp_avg": torch.randn(p.shape, generator=g),
                            "exp_avg_sq": torch.rand(p.shape, generator=g)}


def _assert_same_state(a, b):
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert ga["lr"] == gb["lr"] and ga["name"] == gb["name"] and ga["eps"] == gb["eps"]
        assert tuple(ga["betas"]) == tuple(gb["betas"])
        for pa, pb in zip(ga["params"], gb["params"]):
            sa, sb = a.state[pa], b.state[pb]
            assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
            assert float(sa["step"]) == float(sb["step"])
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


def test_state_dict_interchange_with_torch_adam():
    from gaussianrpg_amd.optim import FusedAdam
    fused = FusedAdam(_groups(_cpu_params()), lr=0.0, eps=1e-15)
    _fill_state(fused, 11)
    adam = torch.optim.Adam(_groups(_cpu_params()), lr=0.0, eps=1e-15)
    adam.load_state_dict(fused.state_dict())              # FusedAdam -> torch.optim.Adam
    _assert_same_state(fused, adam)
    for p in (q for g in adam.param_groups for q in g["params"]):
        p.grad = torch.full_like(p, 1e-3)
    adam.step()                                           # the loaded optimizer is a working torch.optim.Adam
    assert float(adam.state[adam.param_groups[0]["params"][0]]["step"]) == 4.0
    back = FusedAdam(_groups(_cpu_params()), lr=0.0, eps=1e-15)
    back.load_state_dict(adam.state_dict())               # torch.optim.Adam -> FusedAdam
    _assert_same_state(adam, back)
    assert all(g["weight_decay"] == 0 and not g["amsgrad"] for g in back.param_groups)
    # what a non-final checkpoint stores survives torch.save / torch.load unchanged in layout
    sd = fused.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(sd["param_groups"][0]) == set(adam.state_dict()["param_groups"][0])
