"""CPU side of tests/preprocess_bwd_truth.py (the float64 truth of the per-Gaussian preprocess backward, the link of the
training gradient between the blend backward and the composed chain rule; the GPU side is
tests/test_gpu_preprocess_bwd_truth.py).  X comes from oracle.backward on each case's frame under the random loss planes
of tests/test_gpu_backward.py.

  * truth(exact=True) IS the gradient: float64 autograd through oracle/torch_splat.preprocess of the scalar
    sum_i X_i . (mean2D, conic, colour, depth)_i gives the same numbers on every row, once the two places where the
    reference knowingly differs from the exact derivative are added back -- the d tx / d tz term it drops where the
    forward clamped tx or ty (tests/test_oracle_golden.py states it) and the depth term's homogeneous divisor, which
    the forward never applies.  Both differences are asserted in closed form, on the rows they concern.
    Measured: 4e-12 of the row's scale at worst over all cases, fields and rows (needles, scale ratio 1 : 1000,
    included); the bar is 1e-9, what float64 leaves after the cancellation in a c - b^2 of those rows.
  * the group conditions: every visible group keeps >= 32 populated rows, no row near a kink.
  * the bars tell right from wrong: the float32 yardstick Y passes the exact-zero checks in every case, and Y carrying
    each planted error is rejected by (a) or (b) in the group and field the error is expected in.  Outcome: every
    planted error is rejected in every case that reaches its line; `w + 1e-7 dropped` cannot be seen at w >= 0.2 (5e-7
    of the mean2D share, under the 2^-20 floor) and is carried by the case proj-w-small, made for it.
Every figure goes to bench_out/preprocess_bwd_host.json (committed copy: profiles/preprocess_bwd_host.json).
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import preprocess_bwd_truth as pt
from oracle import torch_splat as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTOGRAD_BAR = 1e-9


def _record(case, key, value):
    out = os.path.join(ROOT, "bench_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "preprocess_bwd_host.json")
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data.setdefault(case, {})[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


_FRAMES = {}


def _frame(case):
    """the case's scene, the oracle's forward and backward of it, X, T and Y -- computed once, never changed"""
    if case not in _FRAMES:
        cs = pt.scene(case)
        fwd = pt.oracle_forward(cs)
        g = torch.Generator().manual_seed(100)       # the planes of tests/test_gpu_backward.py _run
        gc = torch.randn(3, pt.H, pt.W, generator=g)
        gd = 0.1 * torch.randn(1, pt.H, pt.W, generator=g)
        ga = torch.randn(1, pt.H, pt.W, generator=g)
        back = oracle.backward(fwd, gc, gd, ga)
        X = pt.records_of(back)
        _FRAMES[case] = dict(cs=cs, fwd=fwd, back=back, X=X, T=pt.truth(cs, X, fwd["radii"]), Y=pt.yardstick(cs, X, fwd))
    return _FRAMES[case]


def _autograd(cs, X):
    """float64 autograd through oracle/torch_splat.preprocess of sum_i X_i . (what the blend reads of Gaussian i).  The
    record's mean2D part is d/d(NDC) (pixels x W / 2, H / 2); its conic part holds HALF the derivative with respect to
    the off-diagonal entry (backward.cu:619-621)."""
    sc = cs.scene
    d = lambda t: None if t is None else t.double().clone().requires_grad_(True)     # noqa: E731
    lv = dict(means3D=d(sc.means3D), shs=None if cs.colors is not None else d(sc.shs), colors=d(cs.colors),
              scales=None if cs.cov is not None else d(sc.scales), rotations=None if cs.cov is not None else d(sc.rotations),
              cov=d(cs.cov))
    pre = ts.preprocess(lv["means3D"], sc.opacity.double(), image_height=pt.H, image_width=pt.W, tanfovx=cs.cam.tanfovx,
                        tanfovy=cs.cam.tanfovy, viewmatrix=cs.cam.viewmatrix.double(), projmatrix=cs.cam.projmatrix.double(),
                        campos=cs.cam.campos.double(), sh_degree=sc.sh_degree, scale_modifier=cs.scale_modifier,
                        shs=lv["shs"], colors_precomp=lv["colors"], scales=lv["scales"], rotations=lv["rotations"],
                        cov3D_precomp=lv["cov"])
    x = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in X.items()}
    m2 = pre["means2D"] * torch.tensor([2.0 / pt.W, 2.0 / pt.H], dtype=torch.float64)
    loss = ((m2 * x["mean2D"][:, :2]).sum() + (pre["depths"] * x["depth"]).sum() + (pre["rgb"] * x["color"]).sum()
            + (pre["conic"] * x["conic"][:, [0, 1, 3]] * torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)).sum())
    loss.backward()
    g = lambda k: None if lv[k] is None else lv[k].grad.numpy()      # noqa: E731
    return dict(means3D=g("means3D"), cov3D=g("cov"), sh=g("shs"), rotations=g("rotations"),
                scales=None if lv["scales"] is None else g("scales") / cs.scale_modifier), pre


@pytest.mark.parametrize("case", list(pt.CASES))
def test_exact_truth_is_the_float64_autograd_gradient(case):
    fr = _frame(case)
    cs, X, radii = fr["cs"], fr["X"], fr["fwd"]["radii"]
    E = pt.truth(cs, X, radii, exact=True)
    G, pre = _autograd(cs, X)
    assert np.array_equal(pre["radii"].numpy(), radii)
    clamped_rows = (E["ratio_x"] > 1.0) | (E["ratio_y"] > 1.0)
    worst = {}
    for field in pt.FIELDS:
        if G[field] is None:
            assert E[field] is None or field == "cov3D"      # dL/dcov3D is an intermediate where scales / rotations are given
            continue
        e = E[field]
        if field == "means3D":
            # the reference's two stated departures from the exact derivative, in closed form
            e = e + E["clamp_term"] + E["depth_term"]
            assert not E["clamp_term"][~clamped_rows].any()
            assert (np.abs(E["clamp_term"][clamped_rows & pt.populated(X, radii)]).max(1) > 0).all()
            if case == "view-w-row":
                assert float(np.abs(E["depth_term"]).max()) > 0
            else:
                assert not E["depth_term"].any()
        n = e.shape[0]
        scale = E["S_mean"] if field == "means3D" else np.abs(e.reshape(n, -1)).max(1)
        live = scale > 0
        assert not G[field].reshape(n, -1)[~live].any()
        worst[field] = float((np.abs(G[field] - e).reshape(n, -1)[live].max(1) / scale[live]).max())
        print("%-16s %-10s worst row |autograd - truth(exact)| / scale = %.2e" % (case, field, worst[field]))
    _record(case, "autograd", worst)
    for field, w in worst.items():
        assert w <= AUTOGRAD_BAR, (field, w)
    # on the clamped rows the reference (and the truth with it) is NOT the exact derivative: the term is there
    rel = np.abs(E["clamp_term"]).max(1)[clamped_rows & pt.populated(X, radii)] / E["S_mean"][clamped_rows & pt.populated(X, radii)]
    assert float(np.median(rel)) > 1e-3, float(np.median(rel))


@pytest.mark.parametrize("case", list(pt.CASES))
def test_conditions_yardstick_and_planted_errors(case):
    fr = _frame(case)
    cs, X, T, Y, fwd = fr["cs"], fr["X"], fr["T"], fr["Y"], fr["fwd"]
    P = cs.scene.means3D.shape[0]
    assert 1500 <= P <= 2500 and P % 256 != 0
    counts = pt.conditions(cs, X, fwd["radii"], T, fwd)
    print(case, "populated rows", counts)
    _record(case, "populated_rows", counts)
    # the yardstick is what oracle.backward computes behind its own blend
    assert np.array_equal(Y["means3D"], fr["back"]["dL_dmeans3D"])
    assert not pt.exact_zero_violations(Y, T, cs, fwd["radii"])
    report = pt.compare(Y, T, Y, cs)
    assert not pt.failures(report)
    _record(case, "yardstick", {"/".join(k): v for k, v in report.items()})
    expect = pt.expected_rejections(cs)
    outcome = {}
    for name, bad in pt.planted_errors(cs, X, fwd["radii"]).items():
        rep = pt.compare(pt.with_plant(Y, T, bad), T, Y, cs)
        failed = pt.failures(rep)
        for k in expect[name]:
            v = rep[k]
            print("%-48s %-22s err %.2e bar %.2e | worst row %.2e bar %.2e  %s" % (
                name, "/".join(k), v["err"], v["bar"], v["worst"], v["worst_bar"], "rejected" if k in failed else "PASSES"))
            outcome["%s @ %s" % (name, "/".join(k))] = dict(err=v["err"], bar=v["bar"], worst=v["worst"],
                                                            worst_bar=v["worst_bar"], rejected=k in failed)
    _record(case, "planted", outcome)
    missed = [k for k, v in outcome.items() if not v["rejected"]]
    assert not missed, missed


def test_every_planted_error_is_reached_by_some_case():
    reached = set()
    for case in pt.CASES:
        reached |= set(pt.expected_rejections(pt.scene(case)))
    assert reached == set(pt.PLANTS)
