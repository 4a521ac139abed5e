"""What hipcc decided for the detector's kernels (no GPU needed): build_native() keeps the compiler's per-kernel resource
report of detector.hip next to the object (gaussianrpg_amd/build.py REMARK_UNITS).  Promised by the sources: no scratch
in any kernel, and the LDS of a workgroup -- two 16-deep tiles with rows padded by 32 floats for the convolution, the
haloed tile and three row-pass planes for the pool.  Registers and occupancy of each tile shape are recorded (printed),
with the one budget the design leans on: the 128 x 128 shape's 64 accumulator registers leave room for at least two
workgroups per SIMD, the 64 x 64 shape for at least four."""
import pytest

from gaussianrpg_amd import build


@pytest.fixture(scope="module")
def resources():
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    return build.kernel_resources("detector.hip")


def _conv(res, bm, k):
    hits = [v for n, v in res.items() if "conv_kernelILi%dELi%dELi%dEE" % (bm, bm, k) in n]
    assert len(hits) == 1, sorted(res)
    return hits[0]


def test_the_unit_has_its_six_kernels_and_none_spills(resources):
    assert len(resources) == 6, sorted(resources)     # conv: 2 tile shapes x k in {1, 3}; pool; weight repack
    assert {n: r["scratch"] for n, r in resources.items() if r["scratch"] != 0} == {}


@pytest.mark.parametrize("bm,waves", [(128, 2), (64, 4)])
@pytest.mark.parametrize("k", [1, 3])
def test_conv_tile_shapes(resources, bm, k, waves):
    r = _conv(resources, bm, k)
    print("conv %dx%d k=%d: %d VGPRs + %d AGPRs, %d SGPRs, occupancy %d, LDS %d" %
          (bm, bm, k, r["vgprs"], r["agprs"], r["sgprs"], r["occupancy"], r["lds"]))
    assert r["lds"] == 2 * 16 * (bm + 32) * 4          # As + Bs: 16 rows of bm + 32 floats
    assert r["vgprs"] + r["agprs"] >= (bm // 64) ** 2 * 16     # the accumulators live in registers
    assert r["occupancy"] >= waves
    assert r["occupancy"] * r["lds"] <= 160 * 1024     # that many workgroups of four waves fit a CU's LDS


def test_pool_kernel(resources):
    hits = [v for n, v in resources.items() if "spp_kernel" in n]
    assert len(hits) == 1
    r = hits[0]
    print("pool: %d VGPRs, occupancy %d, LDS %d" % (r["vgprs"], r["occupancy"], r["lds"]))
    assert r["lds"] == (28 * 29 + 3 * 28 * 17) * 4 and r["occupancy"] == 8
