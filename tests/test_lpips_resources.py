"""What hipcc decided for LPIPS's kernels (no GPU needed): build_native() keeps the compiler's per-kernel resource report
of lpips.hip next to the object (gaussianrpg_amd/build.py REMARK_UNITS).  Promised by the sources and DESIGN.md section
32: no scratch in any kernel; the convolution's LDS is the detector's -- two 16-deep tiles with rows padded by 32 floats
-- and so is its register budget: the 128 x 128 shape's 2 x 64 accumulator registers leave room for at least two
workgroups per SIMD, the 64 x 64 shape for at least four; the distance's static LDS is 64 norms and one float per wave
(its feature tile, at most 48 KiB, is sized at the launch); the finish keeps one float per thread; the pool and the
weight repack none."""
import pytest

from gaussianrpg_amd import build


@pytest.fixture(scope="module")
def resources():
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    return build.kernel_resources("lpips.hip")


def _one(res, word):
    hits = [v for n, v in res.items() if word in n]
    assert len(hits) == 1, (word, sorted(res))
    return hits[0]


def test_the_unit_has_its_ten_kernels_and_none_spills(resources):
    # conv: 2 tile shapes x k in {3, 5, 11}; pool; distance; finish; weight repack
    assert len(resources) == 10, sorted(resources)
    assert {n: r["scratch"] for n, r in resources.items() if r["scratch"] != 0} == {}


@pytest.mark.parametrize("bm,waves", [(128, 2), (64, 4)])
@pytest.mark.parametrize("k", [3, 5, 11])
def test_conv_tile_shapes(resources, bm, k, waves):
    r = _one(resources, "lpips_conv_kernelILi%dELi%dELi%dEE" % (bm, bm, k))
    print("conv %dx%d k=%d: %d VGPRs + %d AGPRs, %d SGPRs, occupancy %d, LDS %d" %
          (bm, bm, k, r["vgprs"], r["agprs"], r["sgprs"], r["occupancy"], r["lds"]))
    assert r["lds"] == 2 * 16 * (bm + 32) * 4          # As + Bs: 16 rows of bm + 32 floats
    assert r["vgprs"] + r["agprs"] >= (bm // 64) ** 2 * 16     # the accumulators live in registers
    assert r["vgprs"] + r["agprs"] <= 512 // waves     # at most 256 / 128 registers
    assert r["occupancy"] >= waves
    assert r["occupancy"] * r["lds"] <= 160 * 1024     # that many workgroups of four waves fit a CU's LDS


def test_pool_distance_finish_and_repack(resources):
    for word, lds in (("lpips_pool_kernel", 0), ("lpips_pack_kernel", 0), ("lpips_distance_kernel", 64 * 4 + 4 * 4),
                      ("lpips_finish_kernel", 1024 * 4)):
        r = _one(resources, word)
        print("%s: %d VGPRs, occupancy %d, LDS %d" % (word, r["vgprs"], r["occupancy"], r["lds"]))
        assert r["lds"] == lds and r["occupancy"] == 8 and r["vgprs"] <= 64
