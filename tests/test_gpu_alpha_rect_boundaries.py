"""-m gpu: evaluation tile lists at the exact lengths where the render changes path, for frames that bin the alpha
rectangle (preprocess.hip binned_rect).

tests/test_gpu_render_occupancy.py and tests/test_gpu_list_boundaries.py pad their lists with fillers of opacity 0.003:
below 0.999/255, so an evaluation frame no longer lists them at all -- their evaluation lists are now the handful of
contributors (the frames still equal the training entry's, which is what those tests assert; the LENGTHS they aim at
are reached on the training entry only).  Here the fillers survive the binned rectangle and still never blend:
opacity 1.07/255 with the centre on a pixel CORNER.  The nearest pixel centres are (0.5, 0.5) away: Q = 0.5 / 2.55 =
0.196 for a 1.5 px splat (+0.3 low-pass), above t = 2 ln 1.07 = 0.135, so no pixel accepts a filler; its alpha box is
+-sqrt(t * 2.55) = +-0.59 px and keeps the one tile the corner lies in, where the reference's rectangle (radius 5) has
up to four.  The evaluation list of the stacked tile is then exactly n long (read from the frame's ranges), the frame equals
the training entry's bit for bit, and the opaque last entry shows that the walk reached the list's end.
"""
import numpy as np
import pytest
import torch

from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

PRODUCER_SPAN = 4 * 256   # render_fwd.hip ListStream<4>, as tests/test_gpu_render_occupancy.py
SH_C0 = 0.28209479177387814
# light path and the light / heavy boundary; the class boundaries -- the reference's and the evaluation frame's own
# (common.h tile_classes_binned: 11/16 of them = 176, 1408, 5632); the producer's window span behind either
LENGTHS = [1, 63, 64, 65, 175, 176, 177, 255, 256, 257, 1407, 1408, 1409, 2047, 2048, 5631, 5632, 5633,
           5632 + PRODUCER_SPAN - 1, 5632 + PRODUCER_SPAN, 5632 + PRODUCER_SPAN + 1, 8191, 8192, 8193,
           8192 + PRODUCER_SPAN - 1, 8192 + PRODUCER_SPAN, 8192 + PRODUCER_SPAN + 1, 3 * PRODUCER_SPAN + 5]
W = H = 64
CENTRE = (24, 24)
BG = (0.1, 0.2, 0.3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def stacked_corners(n, seed=5):
    """n isotropic 1.5 px Gaussians, 1 mm apart in depth, centred on pixel corners of tile (1, 1) at least 2.5 px
    inside it: fillers of opacity 1.07/255 (listed, never accepted), ~6 of opacity 0.2 spread along the list, and the
    last one opaque magenta exactly on pixel CENTRE."""
    f = hz.WAYMO_FX * W / hz.WAYMO_W
    g = torch.Generator().manual_seed(seed + n)
    z = 4.0 + 1e-3 * torch.arange(n, dtype=torch.float32)
    pos = torch.randint(18, 29, (n, 2), generator=g).float() + 0.5       # corners 18.5 .. 28.5
    pos[n - 1] = torch.tensor([float(CENTRE[0]), float(CENTRE[1])])
    x = (pos[:, 0] + 0.5 - W / 2.0) * z / f
    y = (pos[:, 1] + 0.5 - H / 2.0) * z / f
    means3D = torch.stack([x, y, z], 1).contiguous()
    scales = (1.5 * z / f).unsqueeze(1).repeat(1, 3).contiguous()
    rotations = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
    op = torch.full((n, 1), 1.07 / 255.0)
    op[torch.linspace(0, max(n - 2, 0), min(max(n - 1, 0), 6)).long()] = 0.2
    op[n - 1] = 0.99
    rgb = 0.2 + 0.6 * torch.rand(n, 3, generator=g)
    rgb[n - 1] = torch.tensor([1.0, 0.0, 1.0])
    shs = ((rgb - 0.5) / SH_C0).unsqueeze(1).contiguous()
    return hz.Scene(means3D, op, scales, rotations, shs, 0)


def _call(rs, d):
    e = torch.Tensor([])
    P = d.means3D.shape[0]
    return (rs.bg, d.means3D, e, torch.zeros(P, 0, device=d.means3D.device), d.opacity, d.scales, d.rotations,
            rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
            rs.image_width, d.shs, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)


def _settings(dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = hz.trajectory_camera(0, W=W, H=H, device=dev)
    return GaussianRasterizationSettings(**hz.settings_kwargs(cam, 0, bg=torch.tensor(BG, device=dev)))


def _equal(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.parametrize("n", LENGTHS)
def test_evaluation_lists_at_the_paths_boundaries(dev, n):
    from gaussianrpg_amd.rasterizer import _C, debug_export
    d = stacked_corners(n).to(dev)
    rs = _settings(dev)
    tr = _C.rasterize_gaussians(*_call(rs, d))
    with torch.no_grad():
        ev = _C.rasterize_gaussians_eval(*_call(rs, d))
    torch.cuda.synchronize()
    assert ev[0] == tr[0]
    for k, name in ((1, "color"), (2, "depth"), (3, "alpha")):
        _equal(ev[k], tr[k], name)
    assert torch.equal(ev[5], tr[5])
    assert ev[3][0, CENTRE[1], CENTRE[0]].item() > 0.98          # the walk reached the opaque last entry
    # the evaluation frame's own list of the stacked tile is n long; the training entry lists every Gaussian in the
    # one to four tiles of its radius-5 rectangle as well
    gx = (W + 15) // 16
    t = (CENTRE[1] // 16) * gx + CENTRE[0] // 16
    binned = int(ev[6][8:12].cpu().numpy().view(np.uint32)[0])     # BlobHeader.R of the geometry blob
    # (decoded for the instances the frame lists -- its point list ends there)
    rng_ev = debug_export(ev[6], ev[7], ev[8], n, binned, H, W)["ranges"].cpu().numpy().astype(np.int64)
    rng_tr = debug_export(tr[6], tr[7], tr[8], n, tr[0], H, W)["ranges"].cpu().numpy().astype(np.int64)
    assert rng_ev[t, 1] - rng_ev[t, 0] == n == rng_tr[t, 1] - rng_tr[t, 0]
    assert binned == int((rng_ev[:, 1] - rng_ev[:, 0]).sum()) <= tr[0]
    assert n < 63 or binned < tr[0]


@pytest.mark.parametrize("n", [64, 257, 8193])
def test_layered_evaluation_lists(dev, n):
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.rasterizer import _C
    d = stacked_corners(n).to(dev)
    rs = _settings(dev)
    tr = _C.rasterize_gaussians(*_call(rs, d))
    mask = (torch.arange(n, device=dev) % 2) == 1
    with torch.no_grad():
        o = GaussianRasterizer(rs).forward_layers(d.means3D, d.opacity, mask, shs=d.shs, scales=d.scales,
                                                  rotations=d.rotations)
    torch.cuda.synchronize()
    for k, name in ((1, "color"), (2, "depth"), (3, "alpha")):
        _equal(o[name], tr[k], name)
    assert torch.equal(o["radii"], tr[5])
    white = torch.ones(3, device=dev)
    for key, m in (("background", ~mask), ("object", mask)):
        sub = _C.rasterize_gaussians(*_call(rs._replace(bg=white), hz.scene_subset(d, m)))
        torch.cuda.synchronize()
        _equal(o["color_" + key], sub[1], key)
        _equal(o["alpha_" + key], sub[3], key)
