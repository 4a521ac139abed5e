"""What hipcc decided for the LPIPS backward's kernels (no GPU needed): build_native() keeps the compiler's per-kernel
resource report of lpips_bwd.hip next to the object (gaussianrpg_amd/build.py REMARK_UNITS).  Promised by the sources and
DESIGN.md section 33: eight kernels -- backward-data in 2 tile shapes x k in {3, 5}, the strided first layer, the
pool, the distance, the weight repack -- and no scratch in any; the matrix kernel's LDS and register budget are the
forward convolution's (two 16-deep tiles with rows padded by 32 floats; at most 256 registers for the 128 x 128 shape,
two workgroups per SIMD, at most 128 for the 64 x 64 shape, four); the strided kernel, the pool and the repack use no
LDS; the distance's static LDS is 64 norms and 32 coefficients (its feature tile, at most 48 KiB, is sized at the
launch).  lpips.hip keeps its ten kernels (tests/test_lpips_resources.py)."""
import os
import re

import pytest

from gaussianrpg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def resources():
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    build.build_native()
    return build.kernel_resources("lpips_bwd.hip")


def _one(res, word):
    hits = [v for n, v in res.items() if word in n]
    assert len(hits) == 1, (word, sorted(res))
    return hits[0]


def test_the_unit_has_the_documented_kernels_and_none_spills(resources):
    assert len(resources) == 8, sorted(resources)
    assert {n: r["scratch"] for n, r in resources.items() if r["scratch"] != 0} == {}
    # the kernel list of DESIGN.md section 33 is the unit's
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("## 33."):]
    documented = set(re.findall(r"`(lpips_bwd_\w+_kernel)", section))
    built = set(re.search(r"(lpips_bwd_\w+?_kernel)", n).group(1) for n in resources)
    assert documented == built, (sorted(documented), sorted(built))
    assert build.HIP_UNITS["lpips_bwd.hip"] == build.HIP_UNITS["lpips.hip"] and "lpips_bwd.hip" in build.REMARK_UNITS


@pytest.mark.parametrize("bm,waves", [(128, 2), (64, 4)])
@pytest.mark.parametrize("k", [3, 5])
def test_conv_tile_shapes(resources, bm, k, waves):
    r = _one(resources, "lpips_bwd_conv_kernelILi%dELi%dELi%dEE" % (bm, bm, k))
    print("backward-data %dx%d k=%d: %d VGPRs + %d AGPRs, %d SGPRs, occupancy %d, LDS %d" %
          (bm, bm, k, r["vgprs"], r["agprs"], r["sgprs"], r["occupancy"], r["lds"]))
    assert r["lds"] == 2 * 16 * (bm + 32) * 4          # As + Bs: 16 rows of bm + 32 floats
    assert r["vgprs"] + r["agprs"] >= (bm // 64) ** 2 * 16     # the accumulators live in registers
    assert r["vgprs"] + r["agprs"] <= 512 // waves     # at most 256 / 128 registers
    assert r["occupancy"] >= waves
    assert r["occupancy"] * r["lds"] <= 160 * 1024     # that many workgroups of four waves fit a CU's LDS


def test_strided_pool_distance_and_repack(resources):
    for word, lds in (("lpips_bwd_conv_strided_kernel", 0), ("lpips_bwd_pool_kernel", 0), ("lpips_bwd_pack_kernel", 0),
                      ("lpips_bwd_distance_kernel", 64 * 4 + 32 * 4)):
        r = _one(resources, word)
        print("%s: %d VGPRs, occupancy %d, LDS %d" % (word, r["vgprs"], r["occupancy"], r["lds"]))
        assert r["lds"] == lds and r["occupancy"] == 8 and r["vgprs"] <= 64
