"""GPU tests (-m gpu) of the evaluation forward's render launch at five waves per SIMD.

The plain evaluation instantiation of render_forward_kernel has its own register budget, a one-splat light path and
a producer that reads the list in windows of PRODUCER_SPAN entries; the training instantiation is the kernel as it
was.  Both must give the same colour, depth and alpha bits (tests/test_gpu_forward.py holds every call to that), so
the training entry is the in-library reference here, beside the CPU oracle.

Scene: ONE STACKED TILE.  n small Gaussians centred inside one tile at increasing depth.  Most have an opacity below
1/255 -- walked, never accepted, T stays high; a few are accepted, spread along the list; one opaque, distinctly
coloured Gaussian is LAST in depth, so a tail of the list that was not read shows in the pixel.
"""
import numpy as np
import pytest
import torch

import oracle
from gaussianrpg_amd import harness as hz
from helpers import assert_image_close, oracle_kwargs

pytestmark = pytest.mark.gpu

PRODUCER_SPAN = 4 * 256   # entries per register window of the evaluation producer (render_fwd.hip ListStream<4>)
SH_C0 = 0.28209479177387814


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


def stacked_tile(n, W=64, H=64, centre=(24.0, 24.0), sigma_px=1.5, opacity=None, jitter=3.0, seed=5):
    """(scene, camera): n isotropic Gaussians of ~sigma_px pixels whose centres fall within jitter / 2 px of pixel
    `centre`, 1 mm apart in depth.  opacity None: 0.003 (never accepted) except ~6 accepted ones (0.2) spread along
    the list.  The last one is opaque magenta either way and sits exactly on `centre`: without it that pixel's
    alpha stays below 1 - 0.8^6 = 0.74, with it it reaches 0.99."""
    cam = hz.trajectory_camera(0, W=W, H=H)
    f = hz.WAYMO_FX * W / hz.WAYMO_W
    g = torch.Generator().manual_seed(seed + n)
    z = 4.0 + 1e-3 * torch.arange(n, dtype=torch.float32)
    jit = (torch.rand(n, 2, generator=g) - 0.5) * jitter
    jit[n - 1] = 0.0
    x = (centre[0] + jit[:, 0] + 0.5 - W / 2.0) * z / f
    y = (centre[1] + jit[:, 1] + 0.5 - H / 2.0) * z / f
    means3D = torch.stack([x, y, z], 1).contiguous()
    scales = (sigma_px * z / f).unsqueeze(1).repeat(1, 3).contiguous()
    rotations = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
    if opacity is None:
        op = torch.full((n, 1), 0.003)
        op[torch.linspace(0, max(n - 2, 0), min(max(n - 1, 0), 6)).long()] = 0.2
    else:
        op = torch.full((n, 1), float(opacity))
    rgb = 0.2 + 0.6 * torch.rand(n, 3, generator=g)
    op[n - 1] = 0.99
    rgb[n - 1] = torch.tensor([1.0, 0.0, 1.0])
    shs = ((rgb - 0.5) / SH_C0).unsqueeze(1).contiguous()
    return hz.Scene(means3D, op, scales, rotations, shs, 0), cam


BG = (0.1, 0.2, 0.3)
_CACHE = {}


def _both_entries(dev, key, sc, cam):
    """(evaluation outputs, training-entry outputs) of one call each: colour, radii, depth, alpha."""
    if key in _CACHE:
        return _CACHE[key]
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    camd = hz.CameraTensors(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy,
                            cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.campos.to(dev))
    r = GaussianRasterizer(GaussianRasterizationSettings(
        **hz.settings_kwargs(camd, sc.sh_degree, bg=torch.tensor(BG, device=dev))))
    d = sc.to(dev)
    kw = dict(opacities=d.opacity, shs=d.shs, scales=d.scales, rotations=d.rotations)
    with torch.no_grad():
        ev = r(means3D=d.means3D, means2D=None, **kw)[:4]
    m3 = d.means3D.clone().requires_grad_(True)
    tr = r(means3D=m3, means2D=torch.zeros_like(m3, requires_grad=True), **kw)[:4]
    torch.cuda.synchronize()
    _CACHE[key] = ([t.detach() for t in ev], [t.detach() for t in tr])
    return _CACHE[key]


def _assert_entries_equal(ev, tr):
    for name, a, b in zip(("color", "radii", "depth", "alpha"), ev, tr):
        assert torch.equal(a, b), "%s: evaluation and training entry differ in %d values" % (
            name, int((a != b).sum()))


def _assert_oracle(name, ev, sc, cam):
    o = oracle.forward(sc.means3D, sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations,
                       **oracle_kwargs(cam, sc.sh_degree, bg=torch.tensor(BG)))
    np.testing.assert_array_equal(ev[1].cpu().numpy(), o["radii"])
    for k, t in (("color", ev[0]), ("depth", ev[2]), ("alpha", ev[3])):
        assert_image_close("%s.%s" % (name, k), t.cpu().numpy(), o[k], o["fragile"])
    return o


# light path and the light / heavy boundary; the class boundaries; the producer's window span
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 8191, 8192, 8193,
           8192 + PRODUCER_SPAN - 1, 8192 + PRODUCER_SPAN, 8192 + PRODUCER_SPAN + 1, 3 * PRODUCER_SPAN + 5]
ORACLE_LENGTHS = (64, 257, 8193, 3 * PRODUCER_SPAN + 5)


@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths_around_the_paths_boundaries(dev, n):
    sc, cam = stacked_tile(n)
    ev, tr = _both_entries(dev, ("A", n), sc, cam)
    _assert_entries_equal(ev, tr)
    assert ev[3][0, 24, 24].item() > 0.98   # the walk reached the opaque last entry (stacked_tile)


@pytest.mark.parametrize("n", ORACLE_LENGTHS)
def test_list_lengths_match_oracle(dev, n):
    sc, cam = stacked_tile(n)
    ev, _ = _both_entries(dev, ("A", n), sc, cam)
    o = _assert_oracle("stack%d" % n, ev, sc, cam)
    t = (24 // 16) * o["grid"][0] + 24 // 16
    assert int(o["ranges"][t, 1] - o["ranges"][t, 0]) == n   # the list length the case is about


@pytest.mark.parametrize("n", [200, 300, 9000])
def test_clipped_tiles(dev, n):
    # 67 x 45: the stacked tile (columns 64..66, rows 32..44) is cut by the right and the bottom edge, and its
    # left neighbour by the bottom edge: waves with pixels outside the image, the live box shrunk from the start
    sc, cam = stacked_tile(n, W=67, H=45, centre=(65.0, 38.0))
    ev, tr = _both_entries(dev, ("B", n), sc, cam)
    _assert_entries_equal(ev, tr)
    assert ev[3][0, 38, 65].item() > 0.98


def test_early_termination(dev):
    # every pixel of the stacked tile saturates within the first few dozen of 9000 entries: the consumer's stop
    # reaches a producer in the middle of a window.  (Centres within 0.05 px: the oracle flags the ring of pixels where
    # alpha crosses 1/255 for one splat or another of the 9000 as fragile -- 10.1 % of the image with the centres
    # spread over 3 px, 6.3 % like this, under assert_image_close's cap of 10 %)
    sc, cam = stacked_tile(9000, sigma_px=6.0, opacity=0.9, jitter=0.1)
    ev, tr = _both_entries(dev, ("C", 9000), sc, cam)
    _assert_entries_equal(ev, tr)
    o = _assert_oracle("saturated", ev, sc, cam)
    tile = o["n_contrib"][16:32, 16:32]
    assert tile.max() < 200 and float(o["alpha"][0, 16:32, 16:32].min()) > 0.99
