"""Host checks of the selection case table (tests/selection_truth.py): the float64 statements of the reference give
the same bits whatever the deselected elements hold, and the same gradient at every selected element.  That is what
licenses the bit-for-bit assertion of tests/test_gpu_selection.py; it also keeps the table honest: every case has
selected and deselected elements, the SSIM cases a deselected element inside a selected one's window (across a tile
seam where the image has one), the plane cases a quad that holds both kinds."""
import pytest
import torch

import selection_truth as st

CASES = st.CASES
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def clean_runs():
    return {}


def _clean(case, cache):
    if case.id not in cache:
        cache[case.id] = st.evaluate(case, case.clean())
    return cache[case.id]


@pytest.mark.parametrize("poison", [p for p, _ in st.POISONS])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_truth_ignores_deselected_elements(case, poison, clean_runs):
    value = dict(st.POISONS)[poison]
    vals0, grads0 = _clean(case, clean_runs)
    assert vals0 and all(v.numel() > 0 for v in vals0.values())
    for target in case.targets:
        vals, grads = st.evaluate(case, case.poisoned(value, target))
        for k in vals0:
            assert st.same_bits(vals[k], vals0[k]), (case.id, poison, target, k, vals[k], vals0[k])
        for n in case.grads:
            sel = case.grad_selected[n]
            assert st.same_bits(grads[n][sel], grads0[n][sel]), (case.id, poison, target, n)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_has_both_kinds_of_element(case):
    assert case.targets and all(n in case.selected for t in case.targets for n in t)
    for target in case.targets:         # the inputs poisoned together (the models of a list) count as one
        sel = torch.cat([case.selected[n].reshape(-1) for n in target])
        assert bool(sel.any()) and not bool(sel.all()), (case.id, target)
    for n in case.selected:
        assert case.inputs[n].dtype == torch.float32
    for n in case.grads:
        assert case.grad_selected[n].shape == case.inputs[n].shape
    vals, _ = st.evaluate(case, case.clean())
    if "loss" in vals:
        assert bool(torch.isfinite(vals["loss"]).all()), (case.id, vals["loss"])      # a NaN could hide a NaN


@pytest.mark.parametrize("case", [c for c in CASES if c.op in ("ssim", "l1_loss", "l1_ssim_loss")],
                         ids=lambda c: c.id)
def test_ssim_cases_poison_inside_a_selected_window(case):
    within, across = st.ssim_halo_ok(case.selected["img1"])
    assert within
    H, W = case.inputs["img1"].shape[-2:]
    assert (across is None) == (H <= st.SSIM_TILE[0] and W <= st.SSIM_TILE[1])
    assert across in (None, True)


@pytest.mark.parametrize("case", [c for c in CASES if c.op in ("psnr", "lidar_depth_loss", "aux_loss_lidar",
                                                                "aux_loss_lidar_sky", "normal_loss",
                                                                "normal_loss_terms")], ids=lambda c: c.id)
def test_plane_cases_mix_both_kinds_in_a_quad(case):
    for n, sel in case.selected.items():
        assert st.shares_a_quad(sel[0] if sel.dim() == 3 else sel), (case.id, n)


@pytest.mark.parametrize("case", [c for c in CASES if c.reverse is not None], ids=lambda c: c.id)
def test_reverse_inputs_differ_at_one_selected_element(case):
    clean, rev = case.clean(), case.nan_at_selected()
    changed = torch.isnan(rev[case.reverse]) & ~torch.isnan(clean[case.reverse])
    assert int(changed.sum()) == 1 and bool((changed & case.selected[case.reverse]).any())


def test_table_covers_the_ops():
    ops = {c.op for c in CASES}
    assert ops == {"ssim", "l1_loss", "l1_ssim_loss", "psnr", "lidar_depth_loss", "aux_loss_lidar",
                   "aux_loss_lidar_sky", "semantic_loss", "semantic_loss_stats", "normal_loss", "normal_loss_terms",
                   "opacity_sparse_loss", "gaussian_reg_loss", "densify_stats"}
    assert [p for p, _ in st.POISONS] == ["nan", "+inf", "-inf", "1e30"]
