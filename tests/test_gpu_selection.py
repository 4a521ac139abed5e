"""GPU tests of the selection property of every fused op that selects its elements (tests/selection_truth.py has the
case table and says what is out of scope): what a deselected element holds must not reach the result.

Per case and poison (NaN, +Inf, -Inf, and 1e30 as the control that a multiply by a 0/1 mask hides) the op runs on
clean inputs (deselected elements 0.0) and on poisoned ones:
  * every returned value and every gradient has the same bits in both runs (bytes compared, so NaN cannot hide);
  * the gradient is exactly 0 at every deselected element and holds no NaN;
  * the poisoned run's values meet the op's own bars against the float64 truth, taken from the op's test file.
The float64 truth gives the same bits for clean and poisoned inputs (tests/test_selection_host.py), so it is evaluated
once per case.  The reverse check: one NaN at a SELECTED element makes the value NaN exactly when the truth's is."""
import numpy as np
import pytest
import torch

import reg_loss_truth
import normal_loss_truth
import selection_truth as st
import semantic_loss_truth
import test_gpu_aux_loss as t_aux
import test_gpu_loss as t_ssim
import test_gpu_normal_loss as t_normal
import test_gpu_optim as t_optim
import test_gpu_reg_losses as t_reg
import test_gpu_semantic_loss as t_semantic

pytestmark = pytest.mark.gpu

CASES = st.CASES
SSIM_KIND = {"ssim": "ssim", "l1_loss": "l1", "l1_ssim_loss": "mix"}
STATS_KEYS = ("loss", "n_valid", "n_bad", "n_correct")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shared():
    """case id -> (float64 truth of the clean inputs, fused run of the clean inputs), each made once."""
    return {}


# ---- the fused ops: {name: device tensor} -> {output: tensor} ----

def _opacities(x, case):
    ops = [x[n] for n in case.kwargs["names"]]
    return ops[0] if len(ops) == 1 else ops


def _fused(case, x):
    from gaussianrpg_amd import loss
    op = case.op
    if op == "ssim":
        return {"loss": loss.ssim(x["img1"], x["img2"], mask=x["mask"])}
    if op == "l1_loss":
        return {"loss": loss.l1_loss(x["img1"], x["img2"], x["mask"])}
    if op == "l1_ssim_loss":
        l, l1, ss = loss.l1_ssim_loss(x["img1"], x["img2"], x["mask"])
        return {"loss": l, "l1": l1, "ssim": ss}
    if op == "psnr":
        return {"psnr": loss.psnr(x["img1"], x["img2"], x["mask"])}
    if op == "lidar_depth_loss":
        return {"loss": loss.lidar_depth_loss(x["depth"], x["acc"], x["lidar"], x["mask"])}
    if op == "aux_loss_lidar":
        l, terms = loss.aux_loss(x["depth"], x["acc"], lidar_depth=x["lidar"], mask=x["mask"],
                                 lambda_depth_lidar=st.LAMBDA_LIDAR)
        return dict(terms, loss=l)
    if op == "aux_loss_lidar_sky":
        l, terms = loss.aux_loss(x["depth"], x["acc"], lidar_depth=x["lidar"], mask=x["mask"], sky_mask=x["sky"],
                                 sky_scale=st.SKY_SCALE, lambda_depth_lidar=st.LAMBDA_LIDAR, lambda_sky=st.LAMBDA_SKY)
        return dict(terms, loss=l)
    if op == "semantic_loss":
        return {"loss": loss.semantic_loss(x["semantic"], x["gt"], **case.kwargs)}
    if op == "semantic_loss_stats":
        s = loss.semantic_loss_stats(x["semantic"], x["gt"], **case.kwargs)
        return {k: s[k] for k in STATS_KEYS}
    if op == "normal_loss":
        return {"loss": loss.normal_loss(x["normals"], x["mono"], x["wvt"], x["mask"], x.get("sky"), **case.kwargs)}
    if op == "normal_loss_terms":
        return dict(loss.normal_loss_terms(x["normals"], x["mono"], x["wvt"], x["mask"], x.get("sky"), **case.kwargs))
    if op == "opacity_sparse_loss":
        return {"loss": loss.opacity_sparse_loss(_opacities(x, case), x["radii"])}
    if op == "gaussian_reg_loss":
        l, terms = loss.gaussian_reg_loss(scaling=x["scaling"], opacities=_opacities(x, case), radii=x["radii"],
                                          lambda_scale_flatten=st.LAMBDA_SCALE, lambda_opacity_sparse=st.LAMBDA_OPACITY)
        return dict(terms, loss=l)
    assert op == "densify_stats"
    from gaussianrpg_amd.optim import densification_stats_update
    sizes = [e - s for s, e in st.DENSIFY_RANGES]
    accum, denom, max_radii = ([t.clone() for t in x[k].split(sizes)] for k in ("accum", "denom", "max_radii"))
    densification_stats_update(x["grad_xyz"], x["radii"], st.DENSIFY_RANGES, accum, denom, max_radii)
    return {"accum": torch.cat(accum), "denom": torch.cat(denom), "max_radii": torch.cat(max_radii)}


def _run(case, inputs, dev):
    x = {n: t.to(dev) for n, t in inputs.items()}
    for n in case.grads:
        x[n] = x[n].clone().requires_grad_(True)
    out = _fused(case, x)
    grads = {}
    if case.grads:
        out["loss"].backward()
        grads = {n: x[n].grad for n in case.grads}
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in out.items()}, grads


# ---- the float32 PyTorch path of each op (the second half of every value bar) ----

def _ref32(case, x):
    op = case.op
    if op == "psnr":
        return {"psnr": reg_loss_truth.psnr32(x["img1"], x["img2"], x["mask"])}
    if op.startswith(("lidar", "aux_loss")):
        lid = t_aux.torch32_lidar(x["depth"], x["acc"], x["lidar"], x["mask"])
        if op == "lidar_depth_loss":
            return {"loss": lid}
        if op == "aux_loss_lidar":
            return {"loss": st.LAMBDA_LIDAR * lid, "lidar_depth_loss": lid}
        sky = t_aux.torch32_sky(x["acc"], x["sky"], st.SKY_SCALE)
        return {"loss": st.LAMBDA_LIDAR * lid + st.LAMBDA_SKY * sky, "lidar_depth_loss": lid, "sky_loss": sky}
    if op.startswith("semantic"):
        return {"loss": semantic_loss_truth.loss32(x["semantic"], x["gt"], case.kwargs["mode"])}
    if op.startswith("normal"):
        l1, cos, _ = normal_loss_truth.terms32(x["normals"], x["mono"], x["wvt"], x["mask"], x.get("sky"), **case.kwargs)
        return {"loss": l1 + cos, "normal_l1_loss": l1, "normal_cos_loss": cos}
    o = reg_loss_truth.opacity_sparse32([x[n] for n in case.kwargs["names"]], x["radii"])
    if op == "opacity_sparse_loss":
        return {"loss": o}
    s = reg_loss_truth.scale_flatten32(x["scaling"])
    return {"loss": st.LAMBDA_SCALE * s + st.LAMBDA_OPACITY * o, "scale_flatten_loss": s, "opacity_sparse_loss": o}


def _val_ok_of(op):
    if op.startswith(("lidar", "aux_loss")):
        return t_aux._val_ok
    if op.startswith("semantic"):
        return t_semantic._val_ok
    if op.startswith("normal"):
        return t_normal._val_ok
    return t_reg._val_ok


def _meets_its_bars(case, inputs, out, truth, dev):
    """The values of a (poisoned) run against the float64 truth, by the op's own bars."""
    x = {n: t.to(dev) for n, t in inputs.items()}
    what = "%s %s" % (case.op, case.name)
    if case.op in SSIM_KIND:
        mask = x["mask"].bool()
        if x["mask"].dtype != torch.bool:      # a uint8 mask of 255s is the bool mask
            again, _ = _run(case, dict(inputs, mask=inputs["mask"].bool()), dev)
            for k in out:
                assert st.same_bits(out[k], again[k]), (what, k)
        t_ssim._check_against_truth(SSIM_KIND[case.op], x["img1"], x["img2"], mask)      # value and gradient
        return
    if case.op == "densify_stats":
        # the bars of test_gpu_optim.test_densification_stats: accum[:,0] within 2 ulp, everything else exact
        got = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
        ref = {k: v.numpy() for k, v in truth.items()}
        sel = case.selected["grad_xyz"][:, 0].numpy()
        assert (np.abs(got["accum"][sel, 0] - ref["accum"][sel, 0]) <= 2.0 * t_optim._ulp32(ref["accum"][sel, 0])).all()
        assert np.array_equal(got["accum"][sel, 1], ref["accum"][sel, 1].astype(np.float32).astype(np.float64))
        assert np.array_equal(got["accum"][~sel], ref["accum"][~sel])                    # untouched rows
        assert np.array_equal(got["denom"], ref["denom"]) and np.array_equal(got["max_radii"], ref["max_radii"])
        return
    ref32 = _ref32(case, x)
    for k, v in out.items():
        if v.dtype == torch.int64:
            assert int(v) == int(truth[k]), (what, k, int(v), int(truth[k]))
        else:
            _val_ok_of(case.op)(v, truth[k], ref32[k], what + " " + k)


def _clean(case, shared, dev):
    if case.id not in shared:
        truth, _ = st.evaluate(case, case.clean())
        shared[case.id] = (truth, _run(case, case.clean(), dev))
    return shared[case.id]


@pytest.mark.parametrize("poison", [p for p, _ in st.POISONS])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_deselected_elements_do_not_reach_the_result(dev, shared, case, poison):
    value = dict(st.POISONS)[poison]
    truth, (out0, grads0) = _clean(case, shared, dev)
    failures = []
    for target in case.targets:
        inputs = case.poisoned(value, target)
        out, grads = _run(case, inputs, dev)
        print("%s poison %s in %s: %s" % (case.id, poison, "+".join(target),
                                         {k: v.flatten()[:4].tolist() for k, v in out.items()}))
        for k in out0:
            if not st.same_bits(out[k], out0[k]):
                failures.append("%s: value %s differs from the clean run" % (target, k))
        for n in case.grads:
            g, desel = grads[n], ~case.grad_selected[n].to(dev)
            if not st.same_bits(g, grads0[n]):
                failures.append("%s: gradient of %s differs from the clean run" % (target, n))
            if bool(torch.isnan(g).any()):
                failures.append("%s: NaN in the gradient of %s" % (target, n))
            if bool(desel.any()) and not bool((g[desel] == 0).all()):
                failures.append("%s: nonzero gradient of %s at a deselected element" % (target, n))
        assert not failures, (case.id, poison, failures)
        _meets_its_bars(case, inputs, out, truth, dev)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_clean_run_has_exact_zeros_at_deselected_elements(dev, shared, case):
    truth, (out0, grads0) = _clean(case, shared, dev)
    for n in case.grads:
        g, desel = grads0[n], ~case.grad_selected[n].to(dev)
        assert not bool(torch.isnan(g).any()), (case.id, n)
        assert not bool(desel.any()) or bool((g[desel] == 0).all()), (case.id, n)
    _meets_its_bars(case, case.clean(), out0, truth, dev)


REVERSE = [c for c in CASES if c.reverse is not None]


@pytest.mark.parametrize("case", REVERSE, ids=[c.id for c in REVERSE])
def test_nan_at_a_selected_element_shows(dev, case):
    """The other direction: the selection must not hide what it does select."""
    inputs = case.nan_at_selected()
    truth, _ = st.evaluate(case, inputs)
    out, _ = _run(case, inputs, dev)
    for k, v in out.items():
        if v.dtype == torch.int64:
            assert int(v) == int(truth[k]), (case.id, k)
        else:
            assert torch.equal(torch.isnan(v).cpu(), torch.isnan(truth[k])), (case.id, k, v, truth[k])
    assert any(bool(torch.isnan(v).any()) for v in truth.values() if v.is_floating_point()), case.id
