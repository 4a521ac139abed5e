"""What hipcc decided for the render launch (no GPU needed): build_native() keeps the compiler's per-kernel resource
report of render_fwd.hip next to the object (gaussianrpg_amd/build.py REMARK_UNITS).  The plain evaluation
instantiation of render_forward_kernel -- WRITE_AUX = false, NSEM = 0, LAYERS = false, EPI = false: what bench.py and
every no-grad caller launch -- is budgeted for five waves per SIMD (render_fwd.hip render_min_waves): at most 96
VGPRs and NO scratch.  A five-wave kernel that spills is a loss that was measured once (DESIGN_EXPERIMENTS.md)."""
import pytest

from gaussianrpg_amd import build


@pytest.fixture(scope="module")
def resources():
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    res = {k: v for k, v in build.kernel_resources("render_fwd.hip").items() if "render_forward_kernel" in k}
    assert len(res) >= 7, sorted(res)   # plain / semantic x evaluation / training, epilogue, layered x 2
    return res


def _plain_eval(res):
    # render_forward_kernel<WRITE_AUX = false, GPI_L, NSEM = 0, LAYERS = false, EPI = false>
    hits = [k for k in res if "render_forward_kernelILb0ELi" in k and k.split("render_forward_kernelILb0ELi")[1][1:].startswith("ELi0ELb0ELb0EE")]
    assert len(hits) == 1, hits
    return res[hits[0]]


def test_plain_evaluation_kernel_fits_five_waves_without_scratch(resources):
    r = _plain_eval(resources)
    assert r["scratch"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 96, r
    assert r["occupancy"] == 5, r
    assert 5 * r["lds"] <= 160 * 1024, r   # five workgroups of four waves per CU fit its LDS


def test_no_render_instantiation_spills(resources):
    # the parent of this budget had 0 bytes of scratch in every instantiation
    assert {k: v["scratch"] for k, v in resources.items() if v["scratch"] != 0} == {}


def test_other_instantiations_keep_their_budgets(resources):
    # training 4 waves, semantic planes 3, layered and frame-epilogue frames 4
    occ = sorted(v["occupancy"] for v in resources.values())
    assert occ == [3, 3, 4, 4, 4, 4, 5], occ
