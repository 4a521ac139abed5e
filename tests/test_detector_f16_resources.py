"""What hipcc decided for the half detector's kernels (no GPU needed): build_native() keeps the compiler's per-kernel
resource report of detector_f16.hip next to the object (gaussianrpg_amd/build.py REMARK_UNITS).  Promised by the
source's header: no scratch in any kernel; the LDS of a convolution workgroup is (BM + BN) rows of 32 + 8 halves -- two
k-minor tiles, 32 deep, rows padded by one 16-byte access; the pool's is detector.hip's in halves.  Registers and
occupancy are recorded (printed), with the budget the design leans on: the 128 x 128 shape's 64 accumulator registers
leave room for at least two workgroups per SIMD, the 64 x 64 shape for at least four."""
import pytest

from gaussianrpg_amd import build


@pytest.fixture(scope="module")
def resources():
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    return build.kernel_resources("detector_f16.hip")


def _conv(res, bm, k):
    hits = [v for n, v in res.items() if "conv_f16_kernelILi%dELi%dELi%dEE" % (bm, bm, k) in n]
    assert len(hits) == 1, sorted(res)
    return hits[0]


def test_the_unit_has_its_six_kernels_and_none_spills(resources):
    assert len(resources) == 6, sorted(resources)     # conv: 2 tile shapes x k in {1, 3}; pool; weight repack
    assert sum("spp_f16_kernel" in n for n in resources) == 1 and sum("pack_f16_kernel" in n for n in resources) == 1
    assert {n: r["scratch"] for n, r in resources.items() if r["scratch"] != 0} == {}


@pytest.mark.parametrize("bm,waves", [(128, 2), (64, 4)])
@pytest.mark.parametrize("k", [1, 3])
def test_conv_tile_shapes(resources, bm, k, waves):
    r = _conv(resources, bm, k)
    print("conv f16 %dx%d k=%d: %d VGPRs + %d AGPRs, %d SGPRs, occupancy %d, LDS %d" %
          (bm, bm, k, r["vgprs"], r["agprs"], r["sgprs"], r["occupancy"], r["lds"]))
    assert r["lds"] == (bm + bm) * (32 + 8) * 2         # As + Bs: bm rows each of 40 halves
    assert r["vgprs"] + r["agprs"] >= (bm // 64) ** 2 * 16     # the accumulators live in registers
    assert r["occupancy"] >= waves
    assert r["occupancy"] * r["lds"] <= 160 * 1024     # that many workgroups of four waves fit a CU's LDS


def test_pool_kernel(resources):
    r = [v for n, v in resources.items() if "spp_f16_kernel" in n][0]
    print("pool f16: %d VGPRs, occupancy %d, LDS %d" % (r["vgprs"], r["occupancy"], r["lds"]))
    tile, rows = 28 * 29 * 2, 3 * 28 * 17 * 2            # the haloed tile, then (16-byte aligned) the row-pass planes
    assert r["lds"] == -(-tile // 16) * 16 + rows and r["occupancy"] == 8


def test_the_f32_unit_is_as_it_was():
    assert len(build.kernel_resources("detector.hip")) == 6
