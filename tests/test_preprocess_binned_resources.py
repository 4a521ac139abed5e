"""What hipcc decided for the preprocess launches of an evaluation frame (no GPU needed; the reading of
tests/test_preprocess_resources.py, which holds the training frame's kernels to the same budget): the specialised
instantiations of preprocess_binned_kernel / preprocess_composed_binned_kernel -- what bench.py's forward loop
launches -- keep __launch_bounds__(256, 8): at most 64 VGPRs, no scratch, eight workgroups' LDS per CU, with the alpha
box of blend_math.h in them."""
import pytest

from gaussianrpg_amd import build

HOT = "preprocess_binned_kernelILb1EE"
GENERIC = "preprocess_binned_kernelILb0EE"
COMPOSED_HOT = "preprocess_composed_binned_kernelILb1ELb1EE"
COMPOSED_M4 = "preprocess_composed_binned_kernelILb1ELb0EE"
COMPOSED_ANY = "preprocess_composed_binned_kernelILb0ELb0EE"


@pytest.fixture(scope="module")
def resources():
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    return build.kernel_resources("preprocess.hip")


def _one(res, tag):
    hits = [k for k in res if tag in k]
    assert len(hits) == 1, (tag, sorted(res))
    return res[hits[0]]


@pytest.mark.parametrize("tag", [HOT, COMPOSED_HOT])
def test_hot_binned_instantiations_fit_eight_waves_without_scratch(resources, tag):
    r = _one(resources, tag)
    assert r["scratch"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 64, r
    assert r["occupancy"] == 8, r
    assert 8 * r["lds"] <= 160 * 1024, r


def test_other_binned_instantiations_have_no_more_scratch_than_their_twins(resources):
    assert _one(resources, GENERIC)["scratch"] == 0
    assert _one(resources, COMPOSED_M4)["scratch"] == 0
    assert _one(resources, COMPOSED_ANY)["scratch"] <= 208
