"""-m gpu: an evaluation frame bins the 3-sigma rectangle cut to the alpha ellipse's box (preprocess.hip
binned_rect); the frame it returns -- colour, depth, alpha, radii, num_rendered -- stays bit for bit what the training
entry `_C.rasterize_gaussians`, which bins the reference's rectangle, returns.  Scenes: tests/alpha_rect_check.py
(what the restatement predicts for them: tests/test_alpha_rect_host.py).  The binned instance count of a frame is read
from the geometry blob's header (BlobHeader.R, written by the tile scan of the hierarchical binning)."""
import numpy as np
import pytest
import torch

import alpha_rect_check as ar
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

SCENES = ar.scenes()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def _settings(dev, sc, W, H, bg=(0.2, 0.1, 0.3)):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(**hz.settings_kwargs(ar.camera(W, H, dev), sc.sh_degree,
                                                              bg=torch.tensor(bg, device=dev)))


def _call(rs, d):
    e = torch.Tensor([])
    P = d.means3D.shape[0]
    return (rs.bg, d.means3D, e, torch.zeros(P, 0, device=d.means3D.device), d.opacity, d.scales, d.rotations,
            rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
            rs.image_width, d.shs, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)


_REF = {}


def _reference(dev, name):
    """The training entry's frame of a scene, computed once: dict(R, color, depth, alpha, radii, predicted)."""
    if name not in _REF:
        from gaussianrpg_amd.rasterizer import _C, debug_export
        sc, W, H = SCENES[name]
        d = sc.to(dev)
        rs = _settings(dev, sc, W, H)
        R, color, depth, alpha, _sem, radii, geom, binning, img = _C.rasterize_gaussians(*_call(rs, d))
        dbg = debug_export(geom, binning, img, d.means3D.shape[0], R, H, W)
        torch.cuda.synchronize()
        m2, co = dbg["means2D"].cpu().numpy(), dbg["conic_opacity"].cpu().numpy()
        pred = ar.predicted_counts(m2[:, 0], m2[:, 1], co[:, :3], co[:, 3], radii.cpu().numpy(), W, H)
        _REF[name] = dict(R=R, color=color, depth=depth, alpha=alpha, radii=radii, predicted=pred, rs=rs, d=d)
    return _REF[name]


def _same(ref, color, depth, alpha, radii, R=None):
    torch.cuda.synchronize()
    for k, got in (("color", color), ("depth", depth), ("alpha", alpha)):
        a, b = got.cpu().numpy(), ref[k].cpu().numpy()
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (
            "%s: %d of %d values differ" % (k, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size))
    assert torch.equal(radii, ref["radii"])
    if R is not None:
        assert R == ref["R"]


def _binned_count(geom):
    return int(geom[8:12].cpu().numpy().view(np.uint32)[0])     # BlobHeader.R


def _eval(ref):
    from gaussianrpg_amd.rasterizer import _C
    with torch.no_grad():
        out = _C.rasterize_gaussians_eval(*_call(ref["rs"], ref["d"]))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_evaluation_entry_equals_training_entry(dev, name):
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.rasterizer import _C
    ref = _reference(dev, name)
    d = ref["d"]
    _C.reset_capacity_hints()
    for _ in range(2):     # the first frame of a shape runs synchronously, the second on the remembered capacity
        with torch.no_grad():
            color, radii, depth, alpha, _ = GaussianRasterizer(ref["rs"])(
                means3D=d.means3D, means2D=None, opacities=d.opacity, shs=d.shs, scales=d.scales, rotations=d.rotations)
        _same(ref, color, depth, alpha, radii)
        R, color, depth, alpha, _sem, radii, geom = _eval(ref)[:7]
        _same(ref, color, depth, alpha, radii, R)
        # the device binned what the restatement says, never more than the reference
        R_ref, binned, kept, vis = ref["predicted"]
        print("%s: num_rendered %d, binned on the device %d, restatement %d (%d of %d Gaussians kept)" % (
            name, R, _binned_count(geom), binned, kept, vis))
        assert R_ref == R
        assert _binned_count(geom) == binned <= R


def test_the_feature_is_on(dev):
    """The scene the restatement gives a kept ratio <= 0.8: the device's count says the same."""
    ref = _reference(dev, "faint")
    geom = _eval(ref)[6]
    R_ref, binned, kept, vis = ref["predicted"]
    assert binned <= 0.8 * R_ref and kept < vis
    assert _binned_count(geom) == binned < ref["R"]


def test_a_frame_whose_rectangles_are_all_empty_is_the_background(dev):
    ref = _reference(dev, "all_empty")
    R, color, depth, alpha, _sem, radii, geom = _eval(ref)[:7]
    assert R == ref["R"] > 0 and int((radii > 0).sum()) > 100        # visible to the caller ...
    assert _binned_count(geom) == 0                                   # ... and nothing reaches the sort
    assert torch.equal(color, ref["rs"].bg[:, None, None].expand_as(color))
    assert float(alpha.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0
    _same(ref, color, depth, alpha, radii, R)


def _raw_models(d, split):
    """The scene as two raw-parameter models (background, one actor with the identity pose)."""
    from gaussianrpg_amd.composed import ActorPose, ModelParams
    logit = lambda p: torch.log(p / (1.0 - p))   # noqa: E731
    part = lambda s: ModelParams(d.means3D[s].contiguous(), torch.log(d.scales[s]).contiguous(),   # noqa: E731
                                 d.rotations[s].contiguous(), logit(d.opacity[s]).contiguous(),
                                 d.shs[s][:, :1].contiguous(), d.shs[s][:, 1:].contiguous())
    return [part(slice(0, split)), part(slice(split, None))], [None, ActorPose([1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0)]


def test_composed_evaluation_entry(dev):
    from gaussianrpg_amd.composed import ComposedRasterizer, compose
    from gaussianrpg_amd.rasterizer import _C
    sc, W, H = SCENES["faint"]
    d = sc.to(dev)
    rs = _settings(dev, sc, W, H)
    models, poses = _raw_models(d, 2000)
    means, scales, rots, opac, shs = compose(models, poses)
    flat = hz.Scene(means, opac, scales, rots, shs, 1)
    R, color, depth, alpha, _sem, radii = _C.rasterize_gaussians(*_call(rs, flat))[:6]
    want = dict(R=R, color=color, depth=depth, alpha=alpha, radii=radii)
    fused = ComposedRasterizer(rs)
    for _ in range(2):
        with torch.no_grad():
            c, r, dp, a = fused(models, poses)
        _same(want, c, dp, a, r, fused.num_rendered)
    assert R > 10_000


def test_layered_evaluation_entry(dev):
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.rasterizer import _C
    ref = _reference(dev, "faint")
    d, rs = ref["d"], ref["rs"]
    P = d.means3D.shape[0]
    mask = (torch.arange(P, device=dev) % 3) == 0
    white = torch.ones(3, device=dev)
    with torch.no_grad():
        o = GaussianRasterizer(rs).forward_layers(d.means3D, d.opacity, mask, shs=d.shs, scales=d.scales,
                                                  rotations=d.rotations)
    _same(ref, o["color"], o["depth"], o["alpha"], o["radii"])
    for key, m in (("background", ~mask), ("object", mask)):    # the layer planes: the subset alone, on white
        sub = hz.scene_subset(d, m)
        out = _C.rasterize_gaussians(*_call(rs._replace(bg=white), sub))
        torch.cuda.synchronize()
        assert torch.equal(o["color_" + key], out[1]) and torch.equal(o["alpha_" + key], out[3]), key


def test_frame_epilogue_evaluation_entry(dev):
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd import trajectory as tj
    ref = _reference(dev, "elongated")
    d = ref["d"]
    with torch.no_grad():
        o = GaussianRasterizer(ref["rs"]).forward_frame(d.means3D, d.opacity, shs=d.shs, scales=d.scales,
                                                        rotations=d.rotations, planes=True, rgb8=True)
    clamped = dict(ref, color=torch.clamp(ref["color"], 0.0, 1.0))
    _same(clamped, o["rgb"], o["depth"], o["alpha"], o["radii"], o["num_rendered"])
    assert torch.equal(o["rgb8"], tj.pack_hwc(clamped["color"], truncate=True))


def test_deferred_frames(dev):
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.rasterizer import _C, frame_ok
    ref = _reference(dev, "opacity_sweep")
    d = ref["d"]
    _C.reset_capacity_hints()
    r = GaussianRasterizer(ref["rs"])
    kw = dict(means3D=d.means3D, opacities=d.opacity, shs=d.shs, scales=d.scales, rotations=d.rotations)
    for _ in range(3):      # (the first one has no capacity history and runs synchronously inside)
        ticket, color, radii, depth, alpha, _ = r.forward_deferred(**kw)
        assert frame_ok(ticket) is True
        _same(ref, color, depth, alpha, radii)


def test_capacity_overflow_redo(dev):
    from gaussianrpg_amd.rasterizer import _C
    ref = _reference(dev, "elongated")
    sc, W, H = SCENES["elongated"]
    try:
        # far too small for the binned instances and coarse pairs alike: the speculative tail is thrown away and redone
        _C.set_capacity_hint(sc.means3D.shape[0], W, H, 2000, 500)
        R, color, depth, alpha, _sem, radii, geom = _eval(ref)[:7]
        _same(ref, color, depth, alpha, radii, R)
        assert 2000 < _binned_count(geom) == ref["predicted"][1]
    finally:
        _C.reset_capacity_hints()
