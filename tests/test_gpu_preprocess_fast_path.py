"""The specialised preprocess instantiation against the generic one (-m gpu), bit for bit.

launch_preprocess (csrc/preprocess.hip) sends the default hierarchical frame -- scales / rotations and SH colours
given, four SH coefficients, 16-byte aligned inputs, no layer marks -- to preprocess_kernel<HOT = true> and every
other call to preprocess_kernel<false>.  Both run the same expressions in the same order, so one scene sent through
both must give the same bits in every array of the frame, with no tolerance anywhere.  The generic instantiation is
reached the way test_gpu_forward.test_misaligned_input_views reaches it: the identical values as views that start 4
bytes into a larger allocation (vec_ok == 0).  Both frames are also held to the oracle in the arrays
test_gpu_forward._check compares exactly.

A culled Gaussian's record is never written (preprocess.hip: "its sector is not written") and nothing reads it, so
means2D / depths / conic_opacity / rgb are compared on the visible rows (radii, compared whole, fixes which those are).

Sizes: a partial wave, a partial and a whole workgroup (P = 1 .. 257, 1000), and a workgroup's 256 Gaussians at the
edge of a depth-sort chunk of DS_CHUNK = 8192, whose row of the pass-0 table the kernel's atomics address
(P = 8191 .. 8193, 20 000)."""
import numpy as np
import pytest
import torch

import oracle
from gaussianrpg_amd import harness as hz
from helpers import oracle_kwargs

pytestmark = pytest.mark.gpu

EXACT = ("radii", "tiles_touched", "keys_sorted", "point_list", "ranges", "color", "depth", "alpha")
VISIBLE_ROWS = ("means2D", "depths", "conic_opacity", "rgb")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _shifted(t, dev):
    """The same values as a contiguous view starting 4 bytes into a larger allocation."""
    flat = torch.zeros(t.numel() + 1, device=dev)
    flat[1:] = t.reshape(-1).to(dev)
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _frame(dev, d, cam, sh_degree, scale_modifier):
    """One forward call on the device tensors of `d` as they are -> every array of the frame as numpy."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from gaussianrpg_amd.rasterizer import _C, debug_export
    camd = hz.CameraTensors(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy,
                            cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev))
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    rs = GaussianRasterizationSettings(**hz.settings_kwargs(camd, sh_degree, bg=bg, scale_modifier=scale_modifier))
    P = d.means3D.shape[0]
    e = torch.Tensor([])
    R, color, depth, alpha, semantic, radii, geom, binning, img = _C.rasterize_gaussians(
        rs.bg, d.means3D, e, torch.zeros(P, 0, device=dev), d.opacity, d.scales, d.rotations, rs.scale_modifier, e,
        rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, d.shs, rs.sh_degree,
        rs.campos, rs.prefiltered, rs.debug)
    dbg = debug_export(geom, binning, img, P, R, rs.image_height, rs.image_width)
    torch.cuda.synchronize()
    return dict(R=int(R), color=color.cpu().numpy(), depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy(),
                radii=radii.cpu().numpy(), **{k: v.cpu().numpy() for k, v in dbg.items()})


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(hot, gen):
    assert hot["R"] == gen["R"]
    vis = hot["radii"] > 0
    for k in EXACT:
        assert hot[k].shape == gen[k].shape and hot[k].dtype == gen[k].dtype, k
        np.testing.assert_array_equal(_bits(hot[k]), _bits(gen[k]), err_msg=k)
    for k in VISIBLE_ROWS:
        np.testing.assert_array_equal(_bits(hot[k][vis]), _bits(gen[k][vis]), err_msg=k)


def _same_as_oracle(got, o):
    # the arrays test_gpu_forward._check compares exactly
    assert got["R"] == o["num_rendered"]
    np.testing.assert_array_equal(got["radii"], o["radii"])
    np.testing.assert_array_equal(got["tiles_touched"].view(np.uint32), o["tiles_touched"])
    np.testing.assert_array_equal(got["keys_sorted"].view(np.uint64), o["keys_sorted"])
    np.testing.assert_array_equal(got["point_list"].view(np.uint32), o["point_list"])
    np.testing.assert_array_equal(got["ranges"].view(np.uint32), o["ranges"])
    vis = o["radii"] > 0
    np.testing.assert_array_equal(got["means2D"][vis], o["means2D"][vis])
    np.testing.assert_array_equal(got["depths"][vis], o["depths"][vis])
    np.testing.assert_array_equal(got["conic_opacity"][vis], o["conic_opacity"][vis])
    np.testing.assert_array_equal(got["rgb"][vis], o["features"][vis])


def _pair(dev, sc, cam, sh_degree=1, scale_modifier=1.0):
    """(hot frame, generic frame, oracle) of one scene, both frames already compared with each other and the oracle."""
    assert sc.shs.shape[1] == 4   # M == 4: what the specialised instantiation is for
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                       **oracle_kwargs(cam, sh_degree, bg=torch.tensor([0.1, 0.2, 0.3]), scale_modifier=scale_modifier))
    d = sc.to(dev)
    for t in (d.means3D, d.scales, d.shs):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
    hot = _frame(dev, d, cam, sh_degree, scale_modifier)
    g = hz.Scene(_shifted(sc.means3D, dev), d.opacity, _shifted(sc.scales, dev), _shifted(sc.rotations, dev),
                 _shifted(sc.shs, dev), sc.sh_degree)
    gen = _frame(dev, g, cam, sh_degree, scale_modifier)
    _same_bits(hot, gen)
    _same_as_oracle(hot, o)
    _same_as_oracle(gen, o)
    return hot, gen, o


@pytest.mark.parametrize("P", [1, 63, 64, 255, 256, 257, 1000, 8191, 8192, 8193, 20000])
def test_hot_and_generic_instantiation_agree_bit_for_bit(dev, P):
    hot, _, o = _pair(dev, hz.toy_scene(P, seed=40 + P % 7, sh_degree=1), hz.trajectory_camera(0, W=96, H=64))
    if P >= 63:
        assert (o["radii"] > 0).any() and (o["radii"] == 0).any()   # both branches of the cull were taken


def test_odd_sized_image(dev):
    _pair(dev, hz.toy_scene(1000, seed=51, sh_degree=1), hz.trajectory_camera(0, W=203, H=121))


def test_everything_culled(dev):
    # the camera turned away (half a turn about its y axis): the whole cloud is behind the near plane
    cam = hz.make_camera(np.diag([-1.0, 1.0, -1.0]), np.zeros(3), W=96, H=64, fx=hz.WAYMO_FX * 96 / hz.WAYMO_W,
                         fy=hz.WAYMO_FY * 96 / hz.WAYMO_W, cx=48.0, cy=32.0)
    hot, gen, _ = _pair(dev, hz.toy_scene(1000, seed=52, sh_degree=1), cam)
    for f in (hot, gen):
        assert f["R"] == 0 and not f["radii"].any() and not f["tiles_touched"].any()


def test_degree_zero_active_on_four_coefficients(dev):
    # D = 0 on M = 4: only the DC term enters the colour
    sc = hz.toy_scene(1000, seed=53, sh_degree=1)
    hot, _, _ = _pair(dev, sc, hz.trajectory_camera(0, W=96, H=64), sh_degree=0)
    hot1, _, _ = _pair(dev, sc, hz.trajectory_camera(0, W=96, H=64), sh_degree=1)
    vis = hot["radii"] > 0
    assert not np.array_equal(hot["rgb"][vis], hot1["rgb"][vis])


def test_scale_modifier(dev):
    _pair(dev, hz.toy_scene(1000, seed=54, sh_degree=1), hz.trajectory_camera(0, W=96, H=64), scale_modifier=0.7)
