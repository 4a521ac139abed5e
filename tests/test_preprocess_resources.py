"""What hipcc decided for the preprocess launches (no GPU needed): build_native() keeps the compiler's per-kernel
resource report of preprocess.hip next to the object (gaussianrpg_amd/build.py REMARK_UNITS).  The specialised
instantiation preprocess_kernel<HOT = true> -- what launch_preprocess picks for the default hierarchical frame with the
fat depth sort, i.e. what bench.py launches -- is budgeted for eight waves per SIMD (__launch_bounds__(256, 8)): at
most 64 VGPRs and NO scratch, and its LDS lets eight workgroups share a CU.  The other instantiations keep the
scratch their parent had."""
import pytest

from gaussianrpg_amd import build

# Itanium manglings: preprocess_kernel<bool HOT>, preprocess_composed_kernel<bool M4, bool HOT>
HOT = "preprocess_kernelILb1EE"
GENERIC = "preprocess_kernelILb0EE"
COMPOSED_HOT = "preprocess_composed_kernelILb1ELb1EE"
COMPOSED_M4 = "preprocess_composed_kernelILb1ELb0EE"
COMPOSED_ANY = "preprocess_composed_kernelILb0ELb0EE"


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


def _fits_eight_waves(r):
    assert r["scratch"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 64, r
    assert r["occupancy"] == 8, r
    assert 8 * r["lds"] <= 160 * 1024, r   # eight workgroups of four waves per CU fit its LDS


def test_hot_instantiation_fits_eight_waves_without_scratch(resources):
    _fits_eight_waves(_one(resources, HOT))


def test_composed_hot_instantiation_fits_eight_waves_without_scratch(resources):
    _fits_eight_waves(_one(resources, COMPOSED_HOT))


def test_other_instantiations_have_no_more_scratch_than_their_parent(resources):
    # the parent of this budget: generic 0, composed M4 0, composed any-M 208 bytes per lane (its 48-float SH array)
    assert _one(resources, GENERIC)["scratch"] == 0
    assert _one(resources, COMPOSED_M4)["scratch"] == 0
    assert _one(resources, COMPOSED_ANY)["scratch"] <= 208


def test_every_preprocess_instantiation_is_reported(resources):
    names = [k for k in resources if "preprocess_kernel" in k or "preprocess_composed_kernel" in k]
    assert len(names) == 5, sorted(names)
