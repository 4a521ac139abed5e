"""-m gpu: the depth sort (csrc/sort.hip) and the tile partition on inputs that sit ON their seams.

tests/depth_sort_truth.py builds a scene from a list of uint32 depth keys and states what the frame's binning must
be -- the visible ids in (tile, key, id) order -- in three lines of numpy; `conditions` confirms that against the CPU
oracle on every input before it is used here.  Each test then asserts EXACT equality of num_rendered, radii > 0, the
depth keys, tiles_touched, keys_sorted, point_list and ranges, decoded from the blobs of _C.rasterize_gaussians /
_eval (debug_export), and of the geometry header's V / key_base / key_far where the fat sort writes them.  No image
plane is compared with a truth: the blend is pinned elsewhere.  There is no tolerance in this file.

Routes (parametrised, never an environment variable set here): training and evaluation entry point (the latter runs
the binned preprocess with its own pass-0 histogram); sort_binning and the default binning algorithm (whether the
rectangle payload rides through the sort); every frame twice -- on fresh capacity hints (four passes enqueued, the
device decides) and on the history the first frame left (a near frame then enqueues three); the range cases also
speculatively (a far frame on a near history must ask to be rendered again); two cases through the composed entry
point, whose preprocess writes the count table and the min / max words from different code.
"""
import os

import numpy as np
import pytest
import torch

import depth_sort_truth as dt
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

# BlobHeader (csrc/common.h), in 32-bit words
HDR_R, HDR_V, HDR_KEY_BASE, HDR_KEY_FAR = 2, 6, 12, 13


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


@pytest.fixture
def restore_policy():
    """Binning policy switches are process-wide: put the defaults back whatever the test did."""
    from gaussianrpg_amd.rasterizer import _C
    alg = _C.get_binning_algorithm()
    yield _C
    _C.set_binning_mode(0)
    _C.set_binning_algorithm(alg)
    _C.reset_capacity_hints()


# The reference of a case is computed once and shared: every small case stays, of the big ones only the last (a 4 M
# scene with its truth is half a gigabyte of host memory).
_SMALL, _LAST_BIG = {}, {}


def truth(name):
    """(keys, tile, visible, Scene, CameraTensors, expected) of a case, `conditions` asserted on these very inputs."""
    store = _LAST_BIG if name in dt.BIG else _SMALL
    if name not in store:
        if store is _LAST_BIG:
            store.clear()
        keys, tile, gx, gy, cull, sc, cam, visible = dt.build(name)
        e = dt.conditions(sc, cam, keys, tile, visible)
        store[name] = (keys, tile, visible, sc, cam, e)
    return store[name]


def _settings(dev, cam):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    camd = hz.CameraTensors(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, cam.viewmatrix.to(dev),
                            cam.projmatrix.to(dev), cam.campos.to(dev))
    return GaussianRasterizationSettings(**hz.settings_kwargs(camd, 0, bg=torch.zeros(3, device=dev)))


def _call(rs, d):
    e = torch.Tensor([])
    P = d.means3D.shape[0]
    return (rs.bg, d.means3D, e, torch.zeros(P, 0, device=d.means3D.device), d.opacity, d.scales, d.rotations,
            rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
            rs.image_width, d.shs, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)


def _header(blob):
    return blob[:256].cpu().numpy().view(np.uint32)


def _decoded(num_rendered, radii, geom, binning, img, P, rs, evaluation):
    """The frame as depth_sort_truth.compare takes it, plus the geometry header."""
    from gaussianrpg_amd.rasterizer import debug_export
    torch.cuda.synchronize()
    hdr = _header(geom)
    # an evaluation frame lists what its tile scan counted (the header's R): here every visible Gaussian's alpha box
    # keeps the one tile of its rectangle, so that is num_rendered, and `compare` fails on the lengths if it is not
    listed = int(hdr[HDR_R]) if evaluation else int(num_rendered)
    dbg = debug_export(geom, binning, img, P, listed, rs.image_height, rs.image_width)
    got = {k: dbg[k].cpu().numpy() for k in ("depths", "tiles_touched", "keys_sorted", "point_list", "ranges")}
    got.update(num_rendered=int(num_rendered), radii=radii.cpu().numpy(), header=hdr)
    return got


def _frame(rs, d, entry):
    from gaussianrpg_amd.rasterizer import _C
    P = d.means3D.shape[0]
    if entry == "train":
        out = _C.rasterize_gaussians(*_call(rs, d))
    else:
        with torch.no_grad():
            out = _C.rasterize_gaussians_eval(*_call(rs, d))
    got = _decoded(out[0], out[5], out[6], out[7], out[8], P, rs, entry == "eval")
    got["planes"] = (out[1], out[2], out[3])
    return got


def _check(got, e, keys, visible, what):
    P = keys.size
    hdr = got["header"]
    print("%s: R %d  header V %d key_base %#x key_far %d  | truth V %d key_base %#x far %s" % (
        what, got["num_rendered"], hdr[HDR_V], hdr[HDR_KEY_BASE], hdr[HDR_KEY_FAR], e["V"], e["key_base"], e["far"]))
    dt.compare(got, e, keys, visible)
    if -(-P // dt.DS_CHUNK) <= dt.DS_MAX_CHUNKS:        # the fat sort: V and the range decision come from the device
        assert int(hdr[HDR_V]) == e["V"], what
        assert int(hdr[HDR_KEY_FAR] != 0) == int(e["far"]), what
        if e["V"]:
            assert int(hdr[HDR_KEY_BASE]) == e["key_base"], what


def _twice(dev, name, entry, _C):
    keys, tile, visible, sc, cam, e = truth(name)
    rs = _settings(dev, cam)
    d = sc.to(dev)
    _C.reset_capacity_hints()
    for history in ("fresh", "seen"):
        _check(_frame(rs, d, entry), e, keys, visible, "%s %s %s" % (name, entry, history))


@pytest.mark.parametrize("alg", ["sort_binning", "default"])
@pytest.mark.parametrize("entry", ["train", "eval"])
@pytest.mark.parametrize("name", dt.SMALL)
def test_seam_case_is_exact(dev, restore_policy, name, entry, alg):
    _C = restore_policy
    if alg == "sort_binning":
        _C.set_binning_algorithm(0)
    _twice(dev, name, entry, _C)


# A million Gaussians and more: the default route and sort_binning on the training entry point.
# Measured wall time per test on the MI355X box, scene, oracle and truth included (the second route of a case reuses
# them): rows_128 / rows_129 0.38 / 0.35 s; tiles_16x16_r2097153 0.71 s; the pair at the switch, fat_512_chunks 1.56 s
# and classic_512_chunks_plus_1 1.56 s; classic_seam_* 1.40 .. 1.53 s; every second route 0.04 .. 0.16 s.  None
# reaches 5 s; the whole file ran in 12.9 s.  (Scene plus oracle of a 4 M case are single-threaded host work: up to
# 3.5 s on a slower CPU, as tests/test_depth_sort_host.py notes.)
@pytest.mark.parametrize("alg", ["default", "sort_binning"])
@pytest.mark.parametrize("name", dt.BIG)
def test_big_seam_case_is_exact(dev, restore_policy, name, alg):
    _C = restore_policy
    if alg == "sort_binning":
        _C.set_binning_algorithm(0)
    _twice(dev, name, "train", _C)


def _same_planes(a, b, what):
    for x, y, k in zip(a, b, ("color", "depth", "alpha")):
        assert torch.equal(x, y), (what, k)


@pytest.mark.parametrize("name", dt.RANGE)
def test_range_case_on_a_near_history(dev, restore_policy, name):
    """Speculative: after ONE near frame of the same (P, W, H) the hint says "three passes".  A far frame enqueued on
    it synchronously is rendered again inside the call and must be exact; deferred, it must report frame_ok == False
    and the synchronous re-render must be exact.  A near frame must report True and be right on the first try: its
    planes equal, bit for bit, those of the synchronous frame whose lists are compared with the truth."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.rasterizer import frame_ok
    _C = restore_policy
    keys, tile, visible, sc, cam, e = truth(name)
    gx, gy = cam.image_width // 16, cam.image_height // 16
    rs = _settings(dev, cam)
    d = sc.to(dev)
    # the near frame: the same Gaussians, every key at the base
    nkeys = np.full(keys.size, dt.BASE + 5, np.uint32)
    nsc, _, nvis = dt.key_scene(nkeys, tile, gx, gy, seed=1)
    ne = dt.conditions(nsc, cam, nkeys, tile, nvis)
    assert not ne["far"]
    dn = nsc.to(dev)
    rast = GaussianRasterizer(rs)
    kw = dict(means3D=d.means3D, opacities=d.opacity, shs=d.shs, scales=d.scales, rotations=d.rotations)

    def near_history():
        _C.reset_capacity_hints()
        _check(_frame(rs, dn, "eval"), ne, nkeys, nvis, name + " near frame")

    near_history()
    sync = _frame(rs, d, "train")
    _check(sync, e, keys, visible, name + " synchronous on a near history")
    near_history()
    ticket, color, radii, depth, alpha, _ = rast.forward_deferred(**kw)
    ok = frame_ok(ticket)
    # (GRPG_SYNC_R=1, the exact capacity mode: a deferred frame runs synchronously, always with four passes)
    speculative = os.environ.get("GRPG_SYNC_R", "0") in ("", "0")
    print("%s: far %s, deferred frame_ok %s" % (name, e["far"], ok))
    assert ok == (not (e["far"] and speculative))
    again = _frame(rs, d, "eval")
    _check(again, e, keys, visible, name + " synchronous behind the deferred frame")
    _same_planes(again["planes"], sync["planes"], name + " eval against train")
    if ok:
        torch.cuda.synchronize()
        _same_planes((color, depth, alpha), again["planes"], name + " deferred")
        assert torch.equal(radii.cpu(), torch.from_numpy(again["radii"]))


@pytest.mark.parametrize("entry", ["train", "eval"])
@pytest.mark.parametrize("name", dt.COMPOSED)
def test_composed_entry_point_is_exact(dev, restore_policy, name, entry):
    """A background model plus one actor at the identity pose, which together hold the case's Gaussians: the composed
    preprocess writes the pass-0 table and the min / max words from its own code.  The blobs of
    _C.rasterize_gaussians_composed are decoded like the flat call's and compared with the same truth; the planes
    must equal the flat call's on compose()'s output."""
    from gaussianrpg_amd import composed as cp
    _C = restore_policy
    keys, tile, visible, sc, cam, e = truth(name)
    rs = _settings(dev, cam)
    d = sc.to(dev)
    P = keys.size
    cut = P // 3 + 1

    def model(s):
        return cp.ModelParams(d.means3D[s].contiguous(), torch.log(d.scales[s]).contiguous(), d.rotations[s].contiguous(),
                              torch.zeros_like(d.opacity[s]), d.shs[s].contiguous(),      # sigmoid(0) = 0.5
                              torch.zeros(d.shs[s].shape[0], 0, 3, device=dev))

    models = [model(slice(0, cut)), model(slice(cut, P))]
    poses = [None, cp.ActorPose([1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0)]
    # what the composition hands to the rasterizer is still the crafted key set
    means, scales, rots, opac, shs = cp.compose(models, poses)
    assert np.array_equal(means[:, 2].cpu().numpy().view(np.uint32)[visible], keys[visible])
    assert float(opac.min()) == float(opac.max()) == 0.5
    flat = hz.Scene(means, opac, scales, rots, shs, 0)
    lists, pose_t, idft_t = cp._pack(models, poses)
    _C.reset_capacity_hints()
    for history in ("fresh", "seen"):
        with torch.set_grad_enabled(entry == "train"):
            out = cp._rasterize(rs, lists, pose_t, idft_t, [], False, 0, entry == "train")
        num_rendered, color, depth, alpha, _, radii, geom, binning, img = out[:9]
        got = _decoded(num_rendered, radii, geom, binning, img, P, rs, entry == "eval")
        _check(got, e, keys, visible, "%s composed %s %s" % (name, entry, history))
        ref = _frame(rs, flat, entry)
        _check(ref, e, keys, visible, "%s flat on the composition %s %s" % (name, entry, history))
        _same_planes((color, depth, alpha), ref["planes"], name + " composed against flat")
