"""GPU tests of gaussianrpg_amd.optim.densify_and_prune (csrc/densify.hip) against the float64 statement of
tests/densify_truth.py.  Every input keeps densify_truth.MARGIN from every threshold (tests/test_densify_host.py
checks the builder for each case used here), so structure -- counts, row order, src_index -- is compared exactly and
no row is exempted.  Copied values and the moments of originals are compared bit for bit, new moments and the fresh
statistics as exact zeros; the children's xyz offsets and scaling against the truth with the harness's restatement
of the reference's sequence, run by PyTorch in float32 on the CPU, as the yardstick (at most 4 x its error).

Measured figures are printed before they are asserted and collected in bench_out/densify_parity.json."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import densify_truth as truth
import optim_truth
import test_densify_host as host
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.optim import DensifyModel, DensifyRule, FusedAdam, densify_and_prune, fused_adam_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LRS = dict(optim_truth.REF_GROUPS)
COUNT_KEYS = ("points_total", "points_clone", "points_split", "points_below_min_opacity", "points_big_ws",
              "points_pruned")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _record(key, value):
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "densify_parity.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(rows, rule, moments m, v) of one entry of host.GPU_CASES; shared, never modified."""
    P, widths, rule_name, seed = case
    rule, scale = host.rules()[rule_name]
    rows, _ = truth.build_inputs(P, truth.WIDTHS[widths], rule, seed, xyz_scale=scale)
    rng = np.random.default_rng(seed + 5000)
    m = {k: rng.standard_normal(rows[k].shape).astype(np.float32) for k in truth.GROUPS}
    v = {k: rng.random(rows[k].shape).astype(np.float32) for k in truth.GROUPS}
    return rows, rule, m, v


def _model(rows, rule, m, v, dev, cls=FusedAdam, stateful=truth.GROUPS, view=lambda a: a):
    """A DensifyModel on the device: one named group per tensor, state (step 3 + k) for the groups in `stateful`,
    the noise given.  `view` places every array (aligned by default)."""
    put = lambda a: view(torch.from_numpy(np.ascontiguousarray(a)).to(dev))   # noqa: E731
    groups = [{"params": [torch.nn.Parameter(put(rows[name]))], "lr": LRS[name], "name": name}
              for name in truth.GROUPS]
    opt = cls(groups, lr=0.0, eps=optim_truth.REF_EPS)
    for k, g in enumerate(opt.param_groups):
        if g["name"] in stateful:
            opt.state[g["params"][0]] = {"step": torch.tensor(float(3 + k)), "exp_avg": put(m[g["name"]]),
                                         "exp_avg_sq": put(v[g["name"]])}
    return DensifyModel(opt, put(rows["accum"]), put(rows["denom"]), rule, put(rows["split_noise"]),
                        put(rows["box_noise"]))


def _truth(rows, rule, m=None, v=None):
    return truth.evaluate({k: rows[k] for k in truth.GROUPS}, rows["accum"], rows["denom"], rows["split_noise"],
                          rows["box_noise"], rule, m, v)


def _check(tag, res, model, rows, t, m, v, stateful=truth.GROUPS):
    """Everything that is exact; returns the children's (xyz offset, scaling) relative L2 errors."""
    c, n = t.counts, t.counts["n_out"]
    print("%s: P %d -> %d rows %s, clone %d split %d below %d big %d pruned %d" % (
        tag, c["points_total"], n, c["stream"], c["points_clone"], c["points_split"], c["points_below_min_opacity"],
        c["points_big_ws"], c["points_pruned"]))
    print("%s: got %s" % (tag, res.scalars))
    assert res.scalars == {k: c[k] for k in COUNT_KEYS}
    assert res.src_index.dtype == torch.int32 and res.src_index.shape == (n,)
    src = res.src_index.cpu().numpy().astype(np.int64)
    assert np.array_equal(src, t.src_index)
    old, child = t.stream < 2, t.stream >= 2
    opt = model.optimizer
    for k, g in enumerate(opt.param_groups):
        name = g["name"]
        p = g["params"][0]
        assert res.params[name] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert p.shape == (n,) + rows[name].shape[1:] and p.dtype == torch.float32
        got = p.detach().cpu().numpy()
        want = rows[name][src]
        rows_exact = old if name in ("xyz", "scaling") else np.ones(n, dtype=bool)
        assert np.array_equal(got[rows_exact].view(np.uint32), want[rows_exact].view(np.uint32)), name
        if name in stateful:
            st = opt.state[p]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0 + k
            for key, mom in (("exp_avg", m), ("exp_avg_sq", v)):
                got_m = st[key].cpu().numpy()
                assert got_m.shape == got.shape
                orig = t.stream == 0
                assert np.array_equal(got_m[orig].view(np.uint32), mom[name][src][orig].view(np.uint32)), (name, key)
                assert not got_m[~orig].view(np.uint32).any(), (name, key)      # exact +0.0
        else:
            assert p not in opt.state or len(opt.state[p]) == 0
    assert len(opt.state) == len(stateful)
    for got, shape in ((res.xyz_gradient_accum, (n, 2)), (res.denom, (n, 1)), (res.max_radii2D, (n,))):
        assert got.shape == shape and got.dtype == torch.float32
        assert not got.cpu().numpy().view(np.uint32).any()
    parent = rows["xyz"][src][child].astype(np.float64)
    xyz = opt.param_groups[0]["params"][0].detach().cpu().numpy().astype(np.float64)
    sc = opt.param_groups[4]["params"][0].detach().cpu().numpy()
    return (truth.rel_l2(xyz[child] - parent, t.values["xyz"][child] - parent),
            truth.rel_l2(sc[child], t.values["scaling"][child]))


def _yardstick(rows, rule, t):
    """The children's errors of the reference's sequence evaluated by PyTorch in float32 on the CPU."""
    tr = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in rows.items()}
    ref = hz.densify_and_prune_reference({k: tr[k] for k in truth.GROUPS}, {}, tr["accum"], tr["denom"], rule,
                                         tr["split_noise"], tr["box_noise"])
    assert np.array_equal(ref["src_index"].numpy(), t.src_index)        # the margin at work: float32 decides alike
    child = t.stream >= 2
    parent = rows["xyz"][t.src_index][child].astype(np.float64)
    return (truth.rel_l2(ref["tensors"]["xyz"].numpy().astype(np.float64)[child] - parent,
                         t.values["xyz"][child] - parent),
            truth.rel_l2(ref["tensors"]["scaling"].numpy()[child], t.values["scaling"][child]))


@pytest.mark.parametrize("case", host.GPU_CASES[:12], ids=lambda c: "%d-%s" % c[:2])
def test_parity(dev, case):
    rows, rule, m, v = _inputs(case)
    t = _truth(rows, rule, m, v)
    model = _model(rows, rule, m, v, dev)
    (res,) = densify_and_prune([model])
    tag = "parity_%d_%s" % case[:2]
    fused = _check(tag, res, model, rows, t, m, v)
    yard = _yardstick(rows, rule, t)
    out = {"children": int((t.stream >= 2).sum()),
           "xyz_offset": {"fused": fused[0], "torch": yard[0]}, "scaling": {"fused": fused[1], "torch": yard[1]}}
    print(tag, out)
    _record(tag, out)
    if case[0] >= 255:
        assert t.counts["points_clone"] > 0.1 * case[0] and t.counts["points_split"] > 0.1 * case[0]
        assert t.counts["points_below_min_opacity"] > 0.05 * case[0] and t.counts["points_big_ws"] > 0
    assert fused[0] <= 4.0 * yard[0], (tag, "xyz offset", fused[0], yard[0])
    assert fused[1] <= 4.0 * yard[1], (tag, "scaling", fused[1], yard[1])


def _benign(P, seed):
    """Rows nothing happens to under the plain rule: no gradient, small scales, opaque."""
    rule, _ = host.rules()["plain"]
    rows, _ = truth.build_inputs(P, truth.WIDTHS["deg1"], rule, seed, special=False)
    rows = {k: a.copy() for k, a in rows.items()}
    rows["accum"][:] = 0.0
    rows["denom"][:] = 1.0
    rows["scaling"] = np.minimum(rows["scaling"], np.float32(np.log(0.05)))
    rows["opacity"] = np.abs(rows["opacity"]) + np.float32(0.5)
    return rows, rule


def _run_exact(tag, dev, rows, rule, seed):
    rng = np.random.default_rng(seed)
    m = {k: rng.standard_normal(rows[k].shape).astype(np.float32) for k in truth.GROUPS}
    v = {k: rng.random(rows[k].shape).astype(np.float32) for k in truth.GROUPS}
    t = _truth(rows, rule, m, v)
    assert (t.margin >= truth.MARGIN).all()
    model = _model(rows, rule, m, v, dev)
    (res,) = densify_and_prune([model])
    _check(tag, res, model, rows, t, m, v)
    return res, model, t


def test_degenerate_models(dev):
    # nothing selected: the outputs are the inputs, bit for bit (checked against input[src_index] = input)
    rows, rule = _benign(300, 1)
    res, model, t = _run_exact("nothing_selected", dev, rows, rule, 2)
    assert t.counts["n_out"] == 300 and np.array_equal(t.src_index, np.arange(300))
    assert res.scalars["points_clone"] == res.scalars["points_split"] == res.scalars["points_pruned"] == 0
    # every row split: 2 P children, no original
    every = {k: a.copy() for k, a in rows.items()}
    every["accum"][:] = 1.0
    every["scaling"][:] = np.float32(np.log(0.3))
    res, model, t = _run_exact("every_row_split", dev, every, rule, 3)
    assert t.counts["stream"] == [0, 0, 300, 300] and res.scalars["points_split"] == 300
    # every row pruned: 0-row parameters in an optimizer that still steps, and densifies again
    gone = {k: a.copy() for k, a in rows.items()}
    gone["opacity"][:] = -10.0
    gone["accum"][::2] = 1.0                                         # clones and children of transparent rows go too
    res, model, t = _run_exact("every_row_pruned", dev, gone, rule, 4)
    assert t.counts["n_out"] == 0 and res.scalars["points_pruned"] == 300 + int(t.clone.sum()) + 2 * int(t.split.sum())
    for p in res.params.values():
        p.grad = torch.zeros_like(p)
    fused_adam_step([model.optimizer])
    again = densify_and_prune([DensifyModel(model.optimizer, res.xyz_gradient_accum, res.denom, rule)])[0]
    assert again.scalars["points_total"] == 0 and again.src_index.numel() == 0
    assert all(p.shape[0] == 0 for p in again.params.values())
    # 0 / 0 rows are not selected; accum > 0 over denom = 0 is (inf >= max_grad), as in the reference
    zero = {k: a.copy() for k, a in rows.items()}
    zero["denom"][:] = 0.0
    zero["accum"][100:] = np.float32(1e-9)
    res, model, t = _run_exact("zero_denominators", dev, zero, rule, 5)
    assert res.scalars["points_clone"] == 200 and res.scalars["points_split"] == 0 and t.counts["n_out"] == 500
    assert np.array_equal(t.src_index, np.concatenate([np.arange(300), np.arange(100, 300)]))
    # a model without rows, alone and between two others
    empty = {k: a[:0].copy() for k, a in rows.items()}
    res, model, t = _run_exact("no_rows", dev, empty, rule, 6)
    assert t.counts["n_out"] == 0 and res.scalars["points_total"] == 0
    trio = [(every, 3), (empty, 6), (zero, 5)]
    models, truths = [], []
    for r, seed in trio:
        rng = np.random.default_rng(seed)
        m = {k: rng.standard_normal(r[k].shape).astype(np.float32) for k in truth.GROUPS}
        v = {k: rng.random(r[k].shape).astype(np.float32) for k in truth.GROUPS}
        models.append(_model(r, rule, m, v, dev))
        truths.append((r, _truth(r, rule, m, v), m, v))
    for k, (res, model, (r, t, m, v)) in enumerate(zip(densify_and_prune(models), models, truths)):
        _check("trio_%d" % k, res, model, r, t, m, v)


@pytest.mark.parametrize("case", host.GPU_CASES[12:17], ids=lambda c: c[2])
@pytest.mark.parametrize("col", [0, 1])
def test_each_rule(dev, case, col):
    rows, rule, m, v = _inputs(case)
    rule = copy.copy(rule)
    rule.grad_column = col
    t = _truth(rows, rule, m, v)
    model = _model(rows, rule, m, v, dev)
    (res,) = densify_and_prune([model])
    _check("rule_%s_col%d" % (case[2], col), res, model, rows, t, m, v)
    other = copy.copy(rule)
    other.grad_column = 1 - col
    assert not np.array_equal(_truth(rows, other).src_index, t.src_index)            # the column matters
    plain = copy.copy(host.rules()["plain"][0])
    plain.grad_column = col
    tp = _truth(rows, plain)
    if case[2] == "sphere":      # rows far from the centre keep their size
        assert 0 < t.counts["points_big_ws"] < tp.counts["points_big_ws"]
    if case[2] == "box":         # the clone's and the children's own noise slots decide on their own
        assert (t.pruned[0] != t.pruned[1])[t.clone].any() and (t.pruned[2] != t.pruned[3])[t.split].any()
        assert t.counts["points_pruned"] > tp.counts["points_pruned"]
    if case[2] in ("plain_nobig", "box_nobig"):
        assert t.counts["points_big_ws"] == 0 < tp.counts["points_big_ws"]
        assert t.counts["points_pruned"] == t.counts["points_below_min_opacity"]


def _snapshot(res, model):
    out = [res.src_index.cpu(), res.xyz_gradient_accum.cpu(), res.denom.cpu(), res.max_radii2D.cpu()]
    for g in model.optimizer.param_groups:
        p = g["params"][0]
        out.append(p.detach().cpu())
        st = model.optimizer.state.get(p)
        if st:
            out += [st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
                                    for x, y in zip(a, b))


def test_eleven_models_in_one_call(dev):
    cases = host.GPU_CASES[17:28]
    assert [c[0] for c in cases] == [5000] + [300] * 10 and len({c[2] for c in cases}) == 4

    def build():
        return [_model(*_inputs(c), dev, stateful=truth.GROUPS if k % 2 == 0 else ()) for k, c in enumerate(cases)]

    together = build()
    results = densify_and_prune(together)
    singles = build()
    for k, (c, model, res, single) in enumerate(zip(cases, together, results, singles)):
        rows, rule, m, v = _inputs(c)
        _check("eleven_%d" % k, res, model, rows, _truth(rows, rule, m, v), m, v,
               stateful=truth.GROUPS if k % 2 == 0 else ())
        (alone,) = densify_and_prune([single])
        assert alone.scalars == res.scalars
        assert _same(_snapshot(alone, single), _snapshot(res, model)), k


@pytest.mark.parametrize("cls", [FusedAdam, torch.optim.Adam], ids=["fused", "torch"])
@pytest.mark.parametrize("stateful", [truth.GROUPS, (), ("xyz", "opacity", "f_rest")], ids=["state", "none", "some"])
def test_surgery(dev, cls, stateful):
    case = host.GPU_CASES[28]
    rows, rule, m, v = _inputs(case)
    t = _truth(rows, rule, m, v)
    model = _model(rows, rule, m, v, dev, cls=cls, stateful=stateful)
    opt = model.optimizer
    keys = [set(g) for g in opt.param_groups]
    (res,) = densify_and_prune([model])
    _check("surgery_%s_%d" % (cls.__name__, len(stateful)), res, model, rows, t, m, v, stateful=stateful)
    assert [set(g) for g in opt.param_groups] == keys and [g["name"] for g in opt.param_groups] == list(truth.GROUPS)
    assert [g["lr"] for g in opt.param_groups] == [LRS[n] for n in truth.GROUPS]
    # one more step on the new rows, against the truth continued from the moved moments and the kept step counts
    n = t.counts["n_out"]
    rng = np.random.default_rng(11)
    before, grads = {}, {}
    for g in opt.param_groups:
        p = g["params"][0]
        before[g["name"]] = p.detach().cpu().numpy().astype(np.float64)
        grads[g["name"]] = (rng.standard_normal(p.shape) * 1e-3).astype(np.float32)
        p.grad = torch.from_numpy(grads[g["name"]]).to(dev)
    if cls is FusedAdam:
        fused_adam_step([opt])
    else:
        opt.step()
    torch.cuda.synchronize()
    for k, g in enumerate(opt.param_groups):
        name, p = g["name"], g["params"][0]
        if p.numel() == 0:
            continue
        st = optim_truth.AdamState(before[name])
        if name in stateful:
            st.m, st.v, st.t = t.exp_avg[name].copy(), t.exp_avg_sq[name].copy(), 3 + k
        st.step(grads[name], LRS[name])
        state = opt.state[p]
        assert float(state["step"]) == st.t == (4 + k if name in stateful else 1)
        # float32 evaluation of m + (g - m)(1 - b1) and v b2 + g g (1 - b2): three and four roundings of 2^-24 each
        # on terms of one sign or, for m, of the magnitude of m and g -- 1e-6 relative in L2 is > 4 x that
        em = truth.rel_l2(state["exp_avg"].cpu().numpy(), st.m)
        ev = truth.rel_l2(state["exp_avg_sq"].cpu().numpy(), st.v)
        print("surgery %s %s: exp_avg %.3e exp_avg_sq %.3e" % (cls.__name__, name, em, ev))
        assert em <= 1e-6 and ev <= 1e-6, (name, em, ev)
        if LRS[name] > 0:
            after = p.detach().cpu().numpy().astype(np.float64)
            # the update itself to 1e-5 relative, plus one rounding of p (2^-24 |p| per element) over |displacement|
            tol = 1e-5 + 2.0 ** -24 * np.linalg.norm(after) / np.linalg.norm(st.p - st.p0)
            ed = truth.rel_l2(after - before[name], st.p - st.p0)
            print("surgery %s %s: displacement %.3e (bound %.3e)" % (cls.__name__, name, ed, tol))
            assert ed <= tol, (name, ed, tol)
    # the state dict of the operated optimizer loads into the other class and back
    sd = opt.state_dict()
    fresh = [{"params": [torch.nn.Parameter(g["params"][0].detach().clone())], "lr": g["lr"], "name": g["name"]}
             for g in opt.param_groups]
    other = (torch.optim.Adam if cls is FusedAdam else FusedAdam)(fresh, lr=0.0, eps=optim_truth.REF_EPS)
    other.load_state_dict(sd)
    for ga, gb in zip(opt.param_groups, other.param_groups):
        sa, sb = opt.state.get(ga["params"][0], {}), other.state.get(gb["params"][0], {})
        assert set(sa) == set(sb)
        if sa:
            assert float(sa["step"]) == float(sb["step"]) and torch.equal(sa["exp_avg"], sb["exp_avg"])
            assert torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and sb["exp_avg"].shape[0] == n


def test_deterministic_side_stream_and_misaligned_views(dev):
    case = host.GPU_CASES[29]
    rows, rule, m, v = _inputs(case)
    t = _truth(rows, rule, m, v)

    def run(stream=None, view=lambda a: a):
        model = _model(rows, rule, m, v, dev, view=view)
        if stream is None:
            (res,) = densify_and_prune([model])
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                (res,) = densify_and_prune([model])
            torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        return res, model

    res, model = run()
    _check("determinism", res, model, rows, t, m, v)
    first = _snapshot(res, model)
    assert _same(_snapshot(*run()), first)
    assert _same(_snapshot(*run(stream=torch.cuda.Stream())), first)

    def shifted(a):               # the same values at a 4-byte offset into a larger buffer: no 16-byte alignment
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=a.device)
        out = buf[1:].view(a.shape)
        out.copy_(a)
        assert out.data_ptr() % 16 == 4 or a.numel() == 0
        return out

    assert _same(_snapshot(*run(view=shifted)), first)


def test_generator_draws_and_rejections_on_device(dev):
    """Without noise the call draws its own: equal seeds give equal results, the law is the standard normal's."""
    case = host.GPU_CASES[12]
    rows, rule, m, v = _inputs(case)

    def run(seed):
        model = _model(rows, rule, m, v, dev)
        model.split_noise = model.box_noise = None
        gen = torch.Generator(device=dev).manual_seed(seed)
        (res,) = densify_and_prune([model], generator=gen)
        return res, model

    a, b, c = run(5), run(5), run(6)
    assert _same(_snapshot(*a), _snapshot(*b)) and not _same(_snapshot(*a), _snapshot(*c))
    assert a[0].scalars == c[0].scalars                       # plain rule: the draws move children, not decisions
    t = _truth(rows, rule)
    src = a[0].src_index.cpu().numpy()
    assert np.array_equal(src, t.src_index)
    child = t.stream >= 2
    xyz = a[1].optimizer.param_groups[0]["params"][0].detach().cpu().numpy().astype(np.float64)
    R = truth.quat_matrix(rows["rotation"][src][child].astype(np.float64))
    z = np.einsum("njk,nj->nk", R, xyz[child] - rows["xyz"][src][child]) / np.exp(rows["scaling"][src][child])
    print("recovered draws: n %d mean %.3f std %.3f" % (z.size, z.mean(), z.std()))
    # mean and standard deviation of n standard-normal draws lie within 5 / sqrt(n) and 5 / sqrt(2 n) of 0 and 1
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 5 / np.sqrt(2 * z.size)
    model = _model(rows, rule, m, v, dev)
    model.denom = model.denom.cpu()
    with pytest.raises(RuntimeError, match="no CPU path"):
        densify_and_prune([model])
