"""The pose correction's kernels (csrc/pose_correction.hip) against the float64 truth of tests/pose_correction_truth.py
-- at the kernel level (_C.pose_correct*, _C.pose_rows*), with one-hot gradients, through
gaussianrpg_amd.pose_correction against the reference's recorded results, through the C ABI, and on the composed route
(``PoseCorrection.rows`` -> ``ComposedRasterizer``) against the classic one.  The bounds are derived in the truth
module's docstring and shown on the CPU to hold the reference's own float32 results
(tests/test_pose_correction_host.py).  The largest err / bound per output goes to profiles/pose_correction_parity.json.

Where the composed route is asked for the bits of a frame with a STATIC background (identity row), the background's raw
rotations are fixed points of the library's own normalisation: ``compose_one``'s rigid path normalises the product
``rot (x) q`` again, which moves a third of ordinary unit quaternions by an ulp (q / |q| with |q| one rounding off 1), so
"the identity row changes nothing" holds bit for bit exactly where that second division is exact.  The comparisons
within bounds (``test_composed_route_against_classic_route``, ``test_composed_route_gradients``) use ordinary rotations.
"""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import pose_correction_truth as T
from test_gpu_device_poses import BACKWARD, World, _raw, _same
from test_pose_correction_host import golden, golden_inputs, golden_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def parity_file(dev):
    yield
    if PARITY:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "pose_correction_parity.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "what": "largest err / derived bound per output "
                       "(tests/test_gpu_pose_correction.py)", "worst": PARITY}, f, indent=1, sort_keys=True)
            f.write("\n")


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dev(a, dev):
    if a is None:
        return None
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)


def _check(what, **ratios):
    """prints and records the worst err / bound of every quantity first, then asserts"""
    print(what, ratios)
    group = what.split("/")[0]
    for k, v in ratios.items():
        key = "%s/%s" % (group, k)
        PARITY[key] = max(PARITY.get(key, 0.0), float(v))
    for k, v in ratios.items():
        assert v <= 1.0, "%s: %s err / bound = %.3g" % (what, k, v)


def _camera(id=0, frame_idx=0):
    return types.SimpleNamespace(id=id, meta=dict(frame_idx=frame_idx))


def _inputs(N, kind, seed=0):
    rot, trans = T.build_row(kind, seed)
    return dict(rot=rot, trans=trans, xyz=T.build_xyz(N, seed), rotation=T.build_rotation(N, seed + 1),
                gx=T.build_grad(N, 3, seed + 2), gr=T.build_grad(N, 4, seed + 3))


# ---------------------------------------------------------------------------------------------------------------
# 1. kernel level: float64 truth, repeatability
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", T.SIZES)
@pytest.mark.parametrize("kind", T.ROWS)
def test_kernel_matches_float64_truth(dev, N, kind):
    from gaussianrpg_amd.rasterizer import _C
    c = _inputs(N, kind, seed=N % 97)
    d = {k: _dev(v, dev) for k, v in c.items()}
    for parts in ("both", "xyz", "rotation"):
        ux, ur = parts != "rotation", parts != "xyz"
        xyz, rotation, gx, gr = (c["xyz"] if ux else None), (c["rotation"] if ur else None), \
            (c["gx"] if ux else None), (c["gr"] if ur else None)
        f = T.forward64(c["rot"], c["trans"], xyz, rotation)
        b = T.backward64(c["rot"], xyz, rotation, gx, gr)
        dx, dr, dgx, dgr = (d["xyz"] if ux else None), (d["rotation"] if ur else None), (d["gx"] if ux else None), \
            (d["gr"] if ur else None)
        runs = []
        for rep in range(2):
            ox, orot = _C.pose_correct(dx, dr, d["rot"], d["trans"])
            g = _C.pose_correct_backward(dx, dr, d["rot"], d["trans"], dgx, dgr, ux, ur, True, True)
            torch.cuda.synchronize()
            runs.append([t for t in (ox, orot) + tuple(g) if t is not None])
        assert (ox is None) == (not ux) and (orot is None) == (not ur)
        assert (g[0] is None) == (not ux) and (g[1] is None) == (not ur)
        assert tuple(g[2].shape) == (4,) and tuple(g[3].shape) == (3,)
        ratios = dict(g_rot=T.ratio(_np(g[2]), b["g_rot"], b["tol_g_rot"]),
                      g_trans=T.ratio(_np(g[3]), b["g_trans"], b["tol_g_trans"]))
        if ux:
            ratios.update(xyz=T.ratio(_np(ox), f["xyz"], f["tol_xyz"]),
                          g_xyz=T.ratio(_np(g[0]), b["g_xyz"], b["tol_g_xyz"]))
        if ur:
            ratios.update(rotation=T.ratio(_np(orot), f["rotation"], f["tol_rotation"]),
                          g_rotation=T.ratio(_np(g[1]), b["g_rotation"], b["tol_g_rotation"]))
        _check("pose_correct/%d/%s/%s" % (N, kind, parts), **ratios)
        for a_, b_ in zip(*runs):
            assert torch.equal(a_, b_), "two identical calls differ"
        if not ux:
            assert not g[3].any()                          # trans moves xyz' only
    # the inputs are left alone
    assert torch.equal(d["xyz"], _dev(c["xyz"], dev)) and torch.equal(d["rotation"], _dev(c["rotation"], dev))


def test_only_the_gradients_asked_for(dev):
    from gaussianrpg_amd.rasterizer import _C
    c = _inputs(300, "wide", seed=4)
    d = {k: _dev(v, dev) for k, v in c.items()}
    full = _C.pose_correct_backward(d["xyz"], d["rotation"], d["rot"], d["trans"], d["gx"], d["gr"])
    for k in range(4):
        need = [i == k for i in range(4)]
        got = _C.pose_correct_backward(d["xyz"], d["rotation"], d["rot"], d["trans"], d["gx"], d["gr"], *need)
        assert [t is not None for t in got] == need and torch.equal(got[k], full[k])
    # empty input: no rows, zero sums (0 / n is zero for a proper row)
    e = _C.pose_correct(d["xyz"][:0], d["rotation"][:0], d["rot"], d["trans"])
    assert tuple(e[0].shape) == (0, 3) and tuple(e[1].shape) == (0, 4)
    g = _C.pose_correct_backward(d["xyz"][:0], d["rotation"][:0], d["rot"], d["trans"], d["gx"][:0], d["gr"][:0])
    assert not g[2].any() and not g[3].any()


def test_zero_row_is_nan_as_in_the_reference(dev):
    from gaussianrpg_amd.rasterizer import _C
    c = _inputs(5, "wide")
    zero = torch.zeros(4, device=dev)
    ox, orot = _C.pose_correct(_dev(c["xyz"], dev), _dev(c["rotation"], dev), zero, _dev(c["trans"], dev))
    assert bool(torch.isnan(ox).all()) and not orot.any()      # 0 / 0 in quaternion_to_matrix; 0 (x) b = 0


# ---------------------------------------------------------------------------------------------------------------
# 2. one-hot gradients: exactly the restatement's values
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["near", "norm3"])
def test_one_hot_gradients_are_exact(dev, kind):
    from gaussianrpg_amd.rasterizer import _C
    N = 2 * T.BLOCK + 88
    c = _inputs(N, kind, seed=11)
    d = {k: _dev(v, dev) for k, v in c.items()}
    for row in (0, T.BLOCK - 1, T.BLOCK, N - 1):
        gx, gr = np.zeros_like(c["gx"]), np.zeros_like(c["gr"])
        gx[row], gr[row] = c["gx"][row], c["gr"][row]
        want = T.backward32(c["rot"], c["xyz"], c["rotation"], gx, gr)
        got = _C.pose_correct_backward(d["xyz"], d["rotation"], d["rot"], d["trans"], _dev(gx, dev), _dev(gr, dev))
        for name, w, g in zip(("g_xyz", "g_rotation", "g_rot", "g_trans"),
                              (want["g_xyz"], want["g_rotation"], want["g_rot"], want["g_trans"]), got):
            assert np.array_equal(_np(g), w), "%s at row %d: %s against %s" % (name, row, _np(g).ravel()[:8], w.ravel()[:8])
        others = np.delete(np.arange(N), row)
        assert not _np(got[0])[others].any() and not _np(got[1])[others].any()
    PARITY["one_hot/exact"] = 0.0


# ---------------------------------------------------------------------------------------------------------------
# 3. the module against the reference's recorded results
# ---------------------------------------------------------------------------------------------------------------
def _module(c, dev, **kw):
    from gaussianrpg_amd.pose_correction import PoseCorrection
    rots, trans = golden_params(c["kind"], c["num_poses"])
    pc = PoseCorrection(c["num_poses"], mode=c["mode"], **kw)
    pc.load_state_dict({"params": {"pose_correction_trans": torch.from_numpy(trans),
                                   "pose_correction_rots": torch.from_numpy(rots)}})
    return pc.to(dev), rots, trans


def test_module_meets_the_goldens(dev):
    meta, arr = golden()
    for c in meta["cases"]:
        pc, rots, trans = _module(c, dev)
        cam = _camera(c["camera_id"], c["camera_frame_idx"])
        xyz, rotation, gx, gr = golden_inputs(c)
        n, i = c["name"], c["id"]
        f = T.forward64(rots[i], trans[i], xyz, rotation)
        x = _dev(xyz, dev).requires_grad_(True)
        out = pc.correct_gaussian_xyz(cam, x)
        big = torch.zeros(c["N"], 6, device=dev)
        big[:, ::2] = _dev(gx, dev)
        assert not big[:, ::2].is_contiguous()
        out.backward(big[:, ::2])                                 # a non-contiguous upstream gradient
        b = T.backward64(rots[i], xyz, None, gx, None)
        g_rots, g_trans = pc.pose_correction_rots.grad, pc.pose_correction_trans.grad
        assert tuple(g_rots.shape) == (c["num_poses"], 4) and tuple(g_trans.shape) == (c["num_poses"], 3)
        others = [k for k in range(c["num_poses"]) if k != i]
        assert not g_rots[others].any() and not g_trans[others].any()
        ratios = dict(xyz=T.ratio(_np(out), f["xyz"], f["tol_xyz"]),
                      g_xyz=T.ratio(_np(x.grad), b["g_xyz"], b["tol_g_xyz"]),
                      g_rot=T.ratio(_np(g_rots[i]), b["g_rot"], b["tol_g_rot"]),
                      g_trans=T.ratio(_np(g_trans[i]), b["g_trans"], b["tol_g_trans"]),
                      # the reference's own float32 result lies inside the same bound: two bounds apart at the most
                      xyz_vs_golden=T.ratio(_np(out), arr[n + "/xyz"], 2 * f["tol_xyz"]),
                      g_xyz_vs_golden=T.ratio(_np(x.grad), arr[n + "/grad_xyz"], 2 * b["tol_g_xyz"]))
        pc.zero_grad()
        r = _dev(rotation, dev).requires_grad_(True)
        out = pc.correct_gaussian_rotation(cam, r)
        out.backward(_dev(gr, dev))
        b = T.backward64(rots[i], None, rotation, None, gr)
        assert pc.pose_correction_trans.grad is None or not pc.pose_correction_trans.grad.any()
        assert not pc.pose_correction_rots.grad[others].any()
        ratios.update(rotation=T.ratio(_np(out), f["rotation"], f["tol_rotation"]),
                      g_rotation=T.ratio(_np(r.grad), b["g_rotation"], b["tol_g_rotation"]),
                      g_rot_product=T.ratio(_np(pc.pose_correction_rots.grad[i]), b["g_rot"], b["tol_g_rot"]),
                      rotation_vs_golden=T.ratio(_np(out), arr[n + "/rotation"], 2 * f["tol_rotation"]))
        # both in one launch: the same bits as one launch each
        with torch.no_grad():
            bx, br = pc.correct(cam, x, r)
            assert torch.equal(bx, pc.correct_gaussian_xyz(cam, x)) and torch.equal(br, out)
            p = T.row64(rots[i])
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = p["R"], trans[i]
            tol_M = np.zeros((4, 4))
            tol_M[:3, :3] = p["tol_R"]
            ratios["matrix"] = T.ratio(_np(pc(cam)), M, tol_M)
        _check("module/" + n, **ratios)


def test_module_inactive_and_one_output_unused(dev):
    meta, _ = golden()
    c = meta["cases"][1]
    pc, rots, trans = _module(c, dev, active=False)
    cam = _camera(c["camera_id"], c["camera_frame_idx"])
    x, r = _dev(T.build_xyz(9), dev), _dev(T.build_rotation(9), dev)
    assert pc.correct_gaussian_xyz(cam, x) is x and pc.correct_gaussian_rotation(cam, r) is r
    pc.active = True
    x.requires_grad_(True)
    r.requires_grad_(True)
    ox, orot = pc.correct(cam, x, r)
    ox.sum().backward()                                           # rotation' unused: its inputs see no gradient
    assert r.grad is None and x.grad is not None and pc.pose_correction_rots.grad is not None


# ---------------------------------------------------------------------------------------------------------------
# 4. pose_rows: a copy and a scatter
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [0, 1, 10])
def test_pose_rows(dev, A):
    from gaussianrpg_amd.pose_correction import _PoseRows
    from gaussianrpg_amd.rasterizer import _C
    g = torch.Generator().manual_seed(A)
    rot, trans = torch.randn(A, 4, generator=g).to(dev), torch.randn(A, 3, generator=g).to(dev)
    n, id = 5, 3
    cr, ct = torch.randn(n, 4, generator=g).to(dev), torch.randn(n, 3, generator=g).to(dev)
    out_rot, out_trans = _C.pose_rows(rot, trans, cr, ct, id)
    assert tuple(out_rot.shape) == (A + 1, 4) and tuple(out_trans.shape) == (A + 1, 3)
    assert torch.equal(out_rot[:A], rot) and torch.equal(out_trans[:A], trans)
    assert torch.equal(out_rot[A], cr[id]) and torch.equal(out_trans[A], ct[id])          # the RAW row
    gr, gt = torch.randn(A + 1, 4, generator=g).to(dev), torch.randn(A + 1, 3, generator=g).to(dev)
    g_cr, g_ct = _C.pose_rows_backward(gr, gt, n, id)
    want_r, want_t = torch.zeros(n, 4, device=dev), torch.zeros(n, 3, device=dev)
    want_r[id], want_t[id] = gr[A], gt[A]
    assert torch.equal(g_cr, want_r) and torch.equal(g_ct, want_t)
    leaves = [t.clone().requires_grad_(True) for t in (rot, trans, cr, ct)]
    o = _PoseRows.apply(*leaves, id)
    ((o[0] * gr).sum() + (o[1] * gt).sum()).backward()
    assert torch.equal(leaves[0].grad, gr[:A]) and torch.equal(leaves[1].grad, gt[:A])
    assert torch.equal(leaves[2].grad, want_r) and torch.equal(leaves[3].grad, want_t)
    with pytest.raises(RuntimeError, match="is not one of the"):
        _C.pose_rows(rot, trans, cr, ct, n)
    with pytest.raises(RuntimeError, match=r"\[A,4\] and \[A,3\]"):
        _C.pose_rows(rot, trans[:, :2], cr, ct, 0)


# ---------------------------------------------------------------------------------------------------------------
# 5. composed route against classic route, forward
# ---------------------------------------------------------------------------------------------------------------
def _fixed_points(model, dev):
    """the model with raw rotations the library's own normalisation leaves alone (module docstring)"""
    from gaussianrpg_amd.composed import compose
    m = model
    with torch.no_grad():
        for _ in range(6):
            m = m._replace(rotation=compose([m], [None])[2])
        again = compose([m], [None])[2]
        moved = (again != m.rotation).any(1)
        rot = m.rotation.clone()
        rot[moved] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
        assert float(moved.float().mean()) < 0.05
    m = m._replace(rotation=rot.requires_grad_(True))
    with torch.no_grad():
        assert torch.equal(compose([m], [None])[2], m.rotation)
    return m


class Small:
    """background of 700 rows, two actors of 300 and 5 rows (Fourier dimensions 3 and 1), flip on the first actor; a
    pose table of three actors of which the frame shows two"""

    def __init__(self, dev):
        from gaussianrpg_amd import harness as hz
        from gaussianrpg_amd.composed import ComposedRasterizer
        from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
        from gaussianrpg_amd.tracks import PoseBatch
        g = torch.Generator().manual_seed(31)
        self.dev = dev
        self.background = _raw(hz.toy_scene(700, seed=5, sh_degree=1, depth=6.0), dev, g)
        a0 = _raw(hz.toy_scene(300, seed=6, sh_degree=1, depth=0.0, spread=0.3, scale=0.06), dev, g, 3)
        a1 = _raw(hz.toy_scene(5, seed=7, sh_degree=1, depth=0.0, spread=0.3, scale=0.06), dev, g, 1)
        self.actors = [a0._replace(flip=(torch.rand(300, generator=g) < 0.5).to(dev)), a1]
        q = torch.nn.functional.normalize(torch.tensor([[1.0, 0.0, 0.2, 0.0], [0.3, 0.1, 0.9, 0.2], [0.9, 0.0, -0.4, 0.1]]))
        t = torch.tensor([[-0.8, 0.1, 4.5], [9.0, 9.0, 9.0], [0.7, 0.0, 4.0]])
        self.batch = PoseBatch((q * torch.tensor([[1.0], [1.0], [1.7]])).unsqueeze(0).to(dev), t.unsqueeze(0).to(dev),
                               torch.ones(1, 3, dtype=torch.uint8, device=dev))
        self.visible, self.times = [2, 0], [0.4, 0.0]
        self.models = [self.background, self.actors[0], self.actors[1]]
        cam = hz.trajectory_camera(0, W=64, H=48, device=dev)
        self.settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1, bg=torch.tensor([0.2, 0.1, 0.3], device=dev)))
        self.rast = ComposedRasterizer(self.settings)


@pytest.fixture(scope="module")
def small(dev):
    return Small(dev)


def _correction(dev, kind, n=3, id=1, seed=0, **kw):
    from gaussianrpg_amd.pose_correction import PoseCorrection
    pc = PoseCorrection(n, **kw).to(dev)
    if kind != "identity":
        rot, trans = T.build_row(kind, seed)
        with torch.no_grad():
            pc.pose_correction_rots[id] = _dev(rot, dev)
            pc.pose_correction_trans[id] = _dev(trans, dev)
    return pc, _camera(id)


@pytest.mark.parametrize("kind", ["near", "wide", "norm3", "small"])
def test_composed_route_against_classic_route(dev, small, kind):
    from gaussianrpg_amd.composed import compose
    from gaussianrpg_amd.pose_correction import pose_correct
    pc, cam = _correction(dev, kind)
    NB = 700
    with torch.no_grad():
        poses, flags = pc.rows(small.batch, 0, cam, small.visible, small.times)
        assert flags == [False, True, True] and list(poses.row) == [3, 2, 0] and list(poses.posed) == [True] * 3
        got = compose(small.models, poses)
        plain = compose(small.models, small.batch.rows(0, small.visible, small.times))
        rot, trans = pc.row(cam)
        cx, cr = pose_correct(plain[0][:NB].contiguous(), plain[2][:NB].contiguous(), rot, trans)
    # the actors' rows, and every field the correction does not touch: the uncorrected composition's bits
    for k in range(5):
        assert torch.equal(got[k][NB:], plain[k][NB:]), "actors, field %d" % k
    for k in (1, 3, 4):
        assert torch.equal(got[k][:NB], plain[k][:NB]), "background, field %d" % k
    f = T.forward64(_np(rot), _np(trans), _np(plain[0][:NB]), _np(plain[2][:NB]))
    tol_composed = T.COMPOSED_QMUL_ROUND / T.QMUL_ROUND * f["tol_rotation"]
    _check("composed_forward/" + kind,
           classic_xyz=T.ratio(_np(cx), f["xyz"], f["tol_xyz"]),
           classic_rotation=T.ratio(_np(cr), f["rotation"], f["tol_rotation"]),
           composed_xyz=T.ratio(_np(got[0][:NB]), f["xyz"], f["tol_xyz"]),
           composed_rotation=T.ratio(_np(got[2][:NB]), f["rotation"], tol_composed),
           routes_xyz=T.ratio(_np(got[0][:NB]), _np(cx).astype(np.float64), 2 * f["tol_xyz"]),
           routes_rotation=T.ratio(_np(got[2][:NB]), _np(cr).astype(np.float64), f["tol_rotation"] + tol_composed))
    assert not torch.equal(got[0][:NB], plain[0][:NB])            # the correction does something


@pytest.mark.parametrize("how", ["identity", "inactive"])
def test_identity_row_and_inactive_give_the_static_frame(dev, small, how):
    models = [_fixed_points(small.background, dev)] + small.models[1:]
    pc, cam = _correction(dev, "identity" if how == "identity" else "wide", active=how != "inactive")
    base = small.batch.rows(0, small.visible, small.times)
    with torch.no_grad():
        poses, flags = pc.rows(small.batch, 0, cam, small.visible, small.times)
        if how == "inactive":
            _same(list(poses), list(base), "inactive rows")
        a, b = small.rast.forward(models, poses), small.rast.forward(models, base)
        assert int((a[1][:700] > 0).sum()) > 100 and int((a[1][700:] > 0).sum()) > 20
        _same(a, b, "forward")
        _same(small.rast.forward_layers(models, poses, flags), small.rast.forward_layers(models, base),
              "forward_layers")
        fa = small.rast.forward_frame(models, poses, object_models=flags)
        fb = small.rast.forward_frame(models, base)
        assert int(fa["rgb8"].max()) > 0
        _same(fa, fb, "forward_frame")


def test_table_without_actors(dev, small):
    """a scene without tracked actors: the PoseTable straight over the parameters"""
    from gaussianrpg_amd.composed import compose
    from gaussianrpg_amd.pose_correction import pose_correct
    pc, cam = _correction(dev, "near")
    poses, flags = pc.table(cam)
    assert flags == [False] and poses.rot is pc.pose_correction_rots and list(poses.row) == [1]
    with torch.no_grad():
        got = compose([small.background], poses)
        plain = compose([small.background], [None])
        cx, _ = pose_correct(plain[0].contiguous(), None, *pc.row(cam))
    f = T.forward64(_np(pc.row(cam)[0]), _np(pc.row(cam)[1]), _np(plain[0]), None)
    _check("composed_forward/table", xyz=T.ratio(_np(got[0]), f["xyz"], f["tol_xyz"]),
           routes_xyz=T.ratio(_np(got[0]), _np(cx).astype(np.float64), 2 * f["tol_xyz"]))
    color = small.rast.forward([small.background], poses)[0]
    color.sum().backward()
    g = pc.pose_correction_rots.grad
    assert tuple(g.shape) == (3, 4) and not g[[0, 2]].any() and bool(g[1].any())
    assert not pc.pose_correction_trans.grad[[0, 2]].any() and bool(pc.pose_correction_trans.grad[1].any())
    small.background.xyz.grad = None
    for t in small.background[:6]:
        t.grad = None


# ---------------------------------------------------------------------------------------------------------------
# 6. composed route, gradients (the loss on one 16 x 4 strip: tests/test_gpu_device_poses.py says why)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(dev):
    return World(dev)


def _strip(world, models, poses):
    with torch.no_grad():
        cover = world.rast.forward_objects(models, poses)[5][0]
    k = int(cover.view(12, 4, 4, 16).sum((1, 3)).argmax())
    mask = torch.zeros(12, 4, 4, 16, device=world.dev)
    mask[k // 4, :, k % 4, :] = 1.0
    assert float((cover * mask.view(48, 64)).sum()) > 8.0          # the actors are in it
    return mask.view(48, 64)


def _loss(planes, strip, dev):
    gen = torch.Generator().manual_seed(5)
    return sum((p * torch.rand(p.shape, generator=gen).to(dev) * strip).sum() for p in planes)


def test_composed_route_gradients(dev, world):
    """the background row's pose gradient from PoseCorrection.rows against the float64 truth, with the bar of DESIGN.md
    section 9: |A - T| / S <= max(4 |Y - T| / S, K 2^-24).  A: the composed route; Y: float32 autograd through the
    classic route (compose's activated tensors, pose_correct, the classic op); T: backward64 on the classic route's
    upstream gradients; S: the sum of the absolute float64 per-row contributions; K: composed_pose_k."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussianrpg_amd.composed import compose
    from gaussianrpg_amd.pose_correction import pose_correct
    visible, times = BACKWARD
    models = world.models(visible)
    NB, P = 2000, sum(m.xyz.shape[0] for m in models)
    pc, cam = _correction(dev, "near", seed=3)
    with torch.no_grad():
        pc.pose_correction_rots[1] *= 3.0                          # a raw row of norm 3: both normalisations work
    batch = world.batch()
    base = batch.rows(1, visible, times)
    strip = _strip(world, models, base)

    def composed():
        pc.zero_grad()
        poses, _ = pc.rows(world.batch(), 1, cam, visible, times)
        m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
        out = world.rast.forward(models, poses, means2D=m2d)
        _loss([out[0], out[2], out[3]], strip, dev).backward()
        return pc.pose_correction_rots.grad.clone(), pc.pose_correction_trans.grad.clone()

    def classic():
        pc.zero_grad()
        with torch.no_grad():
            x, s, r, o, sh = compose(models, base)
        xa, ra = x[:NB].contiguous(), r[:NB].contiguous()
        cx, cr = pose_correct(xa, ra, *pc.row(cam))
        cx.retain_grad()
        cr.retain_grad()
        m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
        out = GaussianRasterizer(world.settings)(means3D=torch.cat([cx, x[NB:]]), means2D=m2d, opacities=o, shs=sh,
                                                 scales=s, rotations=torch.cat([cr, r[NB:]]))
        _loss([out[0], out[2], out[3]], strip, dev).backward()
        return (pc.pose_correction_rots.grad.clone(), pc.pose_correction_trans.grad.clone(), xa, ra, cx.grad.clone(),
                cr.grad.clone())

    y = classic()
    y2 = classic()
    _same(list(y), list(y2), "the yardstick's own gradients, run twice")
    a, a2 = composed(), composed()      # the background's pose sum is float atomics across its workgroups
    print("the composed route repeats its own bits:", torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]))
    for g in (a[0], a[1], y[0], y[1]):                             # dense, zero outside row id
        assert tuple(g.shape)[0] == 3 and not g[[0, 2]].any() and bool(g[1].any())
    rot = _np(pc.pose_correction_rots[1])
    xa, ra, gx, gr = (_np(t) for t in y[2:])
    t = T.backward64(rot, xa, ra, gx, gr)
    c_rot, c_trans = T.row_contributions(rot, xa, ra, gx, gr)
    S = np.concatenate([np.abs(c_rot).sum(0), np.abs(c_trans).sum(0)])
    truth = np.concatenate([t["g_rot"], t["g_trans"]])
    A = np.concatenate([_np(a[0][1]), _np(a[1][1])]).astype(np.float64)
    Y = np.concatenate([_np(y[0][1]), _np(y[1][1])]).astype(np.float64)
    K = T.composed_pose_k(NB)
    err_a, err_y = np.abs(A - truth) / S, np.abs(Y - truth) / S
    bar = np.maximum(4 * err_y, K * T.U)
    print("composed pose gradient: truth", truth, "\n |A-T|/S", err_a, "\n |Y-T|/S", err_y, "\n bar", bar, "K", K)
    _check("composed_backward/pose", **{"component%d" % k: err_a[k] / bar[k] for k in range(7)})


def test_actor_gradients_do_not_see_an_identity_row(dev, world):
    """the actors' pose gradients through PoseCorrection.rows with the identity row, the background's row detached:
    bit for bit the same step through PoseBatch.rows"""
    visible, times = BACKWARD
    models = [_fixed_points(world.background, dev)] + world.models(visible)[1:]
    P = sum(m.xyz.shape[0] for m in models)
    pc, cam = _correction(dev, "identity")
    pc.pose_correction_rots.requires_grad_(False)
    pc.pose_correction_trans.requires_grad_(False)
    strip = _strip(world, models, world.batch().rows(1, visible, times))
    params = [world.actors.opt_trans, world.actors.opt_rots] + [t for m in models[1:] for t in m[:6]]

    def step(corrected):
        batch = world.batch()
        poses = pc.rows(batch, 1, cam, visible, times)[0] if corrected else batch.rows(1, visible, times)
        m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
        out = world.rast.forward(models, poses, means2D=m2d)
        return torch.autograd.grad(_loss([out[0], out[2], out[3]], strip, dev), params + [m2d])

    plain, again, got = step(False), step(False), step(True)
    assert float(plain[0].abs().max()) > 0 and float(plain[1].abs().max()) > 0
    _same(list(plain), list(again), "the yardstick's own gradients, run twice")
    _same(list(got), list(plain), "actor gradients with the identity row")


def test_forward_objects_with_a_posed_background(dev, world):
    visible, times = BACKWARD
    models = world.models(visible)
    pc, cam = _correction(dev, "identity")
    batch = world.batch()
    with torch.no_grad():
        poses, flags = pc.rows(batch, 1, cam, visible, times)
        got = world.rast.forward_objects(models, poses, flags)
        want = world.rast.forward_objects(models, batch.rows(1, visible, times))
        wrong = world.rast.forward_objects(models, poses)          # the default: the posed background counts as object
    assert float(want[5].max()) > 0
    assert torch.equal(got[5], want[5])
    assert not torch.equal(wrong[5], want[5])


# ---------------------------------------------------------------------------------------------------------------
# 7. C ABI through ctypes
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(dev):
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_pose_correct_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_pose_correct_workspace_bytes.argtypes = [ctypes.c_int]
    P, I = ctypes.c_void_p, ctypes.c_int
    for name, args in (("grpg_pose_correct_forward", [I, P, P, P, P, P, P, P]),
                       ("grpg_pose_correct_backward", [I] + [P] * 11),
                       ("grpg_pose_rows_forward", [I, P, P, I, P, P, I, P, P, P]),
                       ("grpg_pose_rows_backward", [I, I, I, P, P, P, P, P])):
        getattr(lib, name).restype = I
        getattr(lib, name).argtypes = args
    return lib


def _p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def test_cabi_forward_backward_and_argument_errors(dev, lib):
    N = 300
    c = _inputs(N, "norm3", seed=8)
    d = {k: _dev(v, dev) for k, v in c.items()}
    f = T.forward64(c["rot"], c["trans"], c["xyz"], c["rotation"])
    b = T.backward64(c["rot"], c["xyz"], c["rotation"], c["gx"], c["gr"])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd, bwd = lib.grpg_pose_correct_forward, lib.grpg_pose_correct_backward
    ox, orot = torch.empty_like(d["xyz"]), torch.empty_like(d["rotation"])
    assert fwd(N, _p(d["xyz"]), _p(d["rotation"]), _p(d["rot"]), _p(d["trans"]), _p(ox), _p(orot), stream) == 0, \
        lib.grpg_last_error()
    assert lib.grpg_pose_correct_workspace_bytes(N) == 2 * 16 * 4 and lib.grpg_pose_correct_workspace_bytes(0) == 0
    ws = torch.empty(lib.grpg_pose_correct_workspace_bytes(N), dtype=torch.uint8, device=dev)
    g_xyz, g_rotation = torch.empty_like(d["xyz"]), torch.empty_like(d["rotation"])
    g_rot, g_trans = torch.full((4,), 9.0, device=dev), torch.full((3,), 9.0, device=dev)
    assert bwd(N, _p(d["xyz"]), _p(d["rotation"]), _p(d["rot"]), _p(d["gx"]), _p(d["gr"]), _p(g_xyz), _p(g_rotation),
               _p(g_rot), _p(g_trans), _p(ws), stream) == 0, lib.grpg_last_error()
    torch.cuda.synchronize()
    _check("cabi/both", xyz=T.ratio(_np(ox), f["xyz"], f["tol_xyz"]),
           rotation=T.ratio(_np(orot), f["rotation"], f["tol_rotation"]),
           g_xyz=T.ratio(_np(g_xyz), b["g_xyz"], b["tol_g_xyz"]),
           g_rotation=T.ratio(_np(g_rotation), b["g_rotation"], b["tol_g_rotation"]),
           g_rot=T.ratio(_np(g_rot), b["g_rot"], b["tol_g_rot"]), g_trans=T.ratio(_np(g_trans), b["g_trans"], b["tol_g_trans"]))
    # either input NULL
    ox2, orot2 = torch.empty_like(ox), torch.empty_like(orot)
    assert fwd(N, _p(d["xyz"]), None, _p(d["rot"]), _p(d["trans"]), _p(ox2), None, stream) == 0
    assert fwd(N, None, _p(d["rotation"]), _p(d["rot"]), None, None, _p(orot2), stream) == 0
    g_rot_x, g_rot_r = torch.empty(4, device=dev), torch.empty(4, device=dev)
    assert bwd(N, _p(d["xyz"]), None, _p(d["rot"]), _p(d["gx"]), None, None, None, _p(g_rot_x), None, _p(ws), stream) == 0
    assert bwd(N, None, _p(d["rotation"]), _p(d["rot"]), None, _p(d["gr"]), None, None, _p(g_rot_r), None, _p(ws),
               stream) == 0
    assert bwd(N, _p(d["xyz"]), None, _p(d["rot"]), _p(d["gx"]), None, _p(g_xyz), None, None, None, None, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(ox2, ox) and torch.equal(orot2, orot)
    bx = T.backward64(c["rot"], c["xyz"], None, c["gx"], None)
    br = T.backward64(c["rot"], None, c["rotation"], None, c["gr"])
    _check("cabi/one_input", g_rot_xyz=T.ratio(_np(g_rot_x), bx["g_rot"], bx["tol_g_rot"]),
           g_rot_rotation=T.ratio(_np(g_rot_r), br["g_rot"], br["tol_g_rot"]))
    # every refused argument, and the library stays usable
    A = (_p(d["xyz"]), _p(d["rotation"]), _p(d["rot"]))
    bad = [
        fwd(-1, *A, _p(d["trans"]), _p(ox), _p(orot), stream),                                  # N < 0
        fwd(N, None, None, _p(d["rot"]), _p(d["trans"]), None, None, stream),                   # both inputs NULL
        fwd(N, _p(d["xyz"]), _p(d["rotation"]), None, _p(d["trans"]), _p(ox), _p(orot), stream),  # NULL row
        fwd(N, _p(d["xyz"]), None, _p(d["rot"]), None, _p(ox), None, stream),                   # xyz without trans
        fwd(N, _p(d["xyz"]), None, _p(d["rot"]), _p(d["trans"]), None, None, stream),           # input without output
        fwd(N, _p(d["xyz"]), None, _p(d["rot"]), _p(d["trans"]), _p(ox), _p(orot), stream),     # output without input
        fwd(N, _p(d["xyz"], 2), None, _p(d["rot"]), _p(d["trans"]), _p(ox), None, stream),      # misaligned
        fwd(N, _p(d["xyz"]), None, _p(d["rot"], 1), _p(d["trans"]), _p(ox), None, stream),
        bwd(-1, *A, _p(d["gx"]), _p(d["gr"]), _p(g_xyz), _p(g_rotation), _p(g_rot), _p(g_trans), _p(ws), stream),
        bwd(N, *A, None, None, None, None, _p(g_rot), _p(g_trans), _p(ws), stream),             # no upstream gradient
        bwd(N, None, _p(d["rotation"]), _p(d["rot"]), _p(d["gx"]), None, None, None, _p(g_rot), None, _p(ws), stream),
        bwd(N, *A, _p(d["gx"]), None, None, _p(g_rotation), None, None, None, stream),          # g_rotation, no upstream
        bwd(N, *A, _p(d["gx"]), _p(d["gr"]), None, None, None, None, None, stream),             # nothing to write
        bwd(N, *A, _p(d["gx"]), _p(d["gr"]), None, None, _p(g_rot), None, None, stream),        # sums, no workspace
        bwd(N, *A, _p(d["gx"]), _p(d["gr"]), None, None, _p(g_rot), None, _p(ws, 2), stream),   # misaligned workspace
        bwd(N, _p(d["xyz"]), _p(d["rotation"]), None, _p(d["gx"]), _p(d["gr"]), _p(g_xyz), None, None, None, None, stream),
    ]
    assert bad == [-1] * len(bad), bad
    assert b"pose_correct" in lib.grpg_last_error()
    rows_f, rows_b = lib.grpg_pose_rows_forward, lib.grpg_pose_rows_backward
    rot, trans = torch.randn(2, 4, device=dev), torch.randn(2, 3, device=dev)
    cr, ct = torch.randn(4, 4, device=dev), torch.randn(4, 3, device=dev)
    o_r, o_t = torch.empty(3, 4, device=dev), torch.empty(3, 3, device=dev)
    assert rows_f(2, _p(rot), _p(trans), 4, _p(cr), _p(ct), 2, _p(o_r), _p(o_t), stream) == 0, lib.grpg_last_error()
    g_cr, g_ct = torch.empty(4, 4, device=dev), torch.empty(4, 3, device=dev)
    assert rows_b(2, 4, 2, _p(o_r), _p(o_t), _p(g_cr), _p(g_ct), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(o_r, torch.cat([rot, cr[2:3]])) and torch.equal(o_t, torch.cat([trans, ct[2:3]]))
    assert torch.equal(g_cr[2], cr[2]) and not g_cr[[0, 1, 3]].any() and torch.equal(g_ct[2], ct[2])
    o1_r, o1_t = torch.empty(1, 4, device=dev), torch.empty(1, 3, device=dev)
    assert rows_f(0, None, None, 4, _p(cr), _p(ct), 3, _p(o1_r), _p(o1_t), stream) == 0        # A = 0
    torch.cuda.synchronize()
    assert torch.equal(o1_r[0], cr[3]) and torch.equal(o1_t[0], ct[3])
    bad = [
        rows_f(-1, _p(rot), _p(trans), 4, _p(cr), _p(ct), 2, _p(o_r), _p(o_t), stream),
        rows_f(2, _p(rot), _p(trans), 4, _p(cr), _p(ct), 4, _p(o_r), _p(o_t), stream),          # id outside
        rows_f(2, _p(rot), _p(trans), 4, _p(cr), _p(ct), -1, _p(o_r), _p(o_t), stream),
        rows_f(2, _p(rot), _p(trans), 0, _p(cr), _p(ct), 0, _p(o_r), _p(o_t), stream),
        rows_f(2, None, _p(trans), 4, _p(cr), _p(ct), 2, _p(o_r), _p(o_t), stream),
        rows_f(2, _p(rot), _p(trans), 4, _p(cr), _p(ct), 2, None, _p(o_t), stream),
        rows_f(2, _p(rot), _p(trans), 4, _p(cr, 2), _p(ct), 2, _p(o_r), _p(o_t), stream),
        rows_b(2, 4, 4, _p(o_r), _p(o_t), _p(g_cr), _p(g_ct), stream),
        rows_b(2, 4, 2, None, _p(o_t), _p(g_cr), _p(g_ct), stream),
    ]
    assert bad == [-1] * len(bad), bad
    assert b"pose_rows" in lib.grpg_last_error()
    assert fwd(N, _p(d["xyz"]), _p(d["rotation"]), _p(d["rot"]), _p(d["trans"]), _p(ox2), _p(orot2), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(ox2, ox)


def test_binding_argument_errors(dev):
    from gaussianrpg_amd.rasterizer import _C
    x, r = torch.zeros(4, 3, device=dev), torch.zeros(4, 4, device=dev)
    rot, trans = torch.tensor([1.0, 0, 0, 0], device=dev), torch.zeros(3, device=dev)
    with pytest.raises(RuntimeError, match="give xyz, rotation, or both"):
        _C.pose_correct(None, None, rot, trans)
    with pytest.raises(RuntimeError, match=r"float32 tensor \[N,3\]"):
        _C.pose_correct(r, None, rot, trans)
    with pytest.raises(RuntimeError, match="disagree on N"):
        _C.pose_correct(x, r[:3], rot, trans)
    with pytest.raises(RuntimeError, match=r"rot \[4\] and trans \[3\]"):
        _C.pose_correct(x, r, rot.cpu(), trans)
    with pytest.raises(RuntimeError, match=r"rot \[4\] and trans \[3\]"):
        _C.pose_correct(x, r, rot.double(), trans)
    with pytest.raises(RuntimeError, match="at least one upstream gradient"):
        _C.pose_correct_backward(x, r, rot, trans, None, None)
    with pytest.raises(RuntimeError, match="needs its forward input"):
        _C.pose_correct_backward(None, r, rot, trans, x, None)
    with pytest.raises(RuntimeError, match=r"grad_xyz must be"):
        _C.pose_correct_backward(x, r, rot, trans, x[:2], None, True, False, True, True)
    with pytest.raises(RuntimeError, match="needs its upstream gradient"):
        _C.pose_correct_backward(x, r, rot, trans, x, None, True, True, True, True)


# ---------------------------------------------------------------------------------------------------------------
# 8. the harness routes
# ---------------------------------------------------------------------------------------------------------------
def test_harness_routes_agree(dev, world):
    from gaussianrpg_amd import harness as hz
    import helpers
    visible, times = BACKWARD
    models = world.models(visible)
    pc, cam = _correction(dev, "near", seed=3)
    batch = world.batch()
    frames = {}
    for name, kw in (("composed", dict(composed=True)), ("classic", dict(composed=False)),
                     ("classic_torch", dict(composed=False, fused=False))):
        frames[name] = hz.corrected_frame(world.settings, models, batch, 1, visible, times, pc, cam, **kw)
    with torch.no_grad():
        static = world.rast.forward(models, batch.rows(1, visible, times))
    assert int((frames["composed"][1][:2000] > 0).sum()) > 500 and int((frames["composed"][1][2000:] > 0).sum()) > 20
    assert not torch.equal(frames["composed"][0], static[0].clamp(0, 1))          # the correction moves the picture
    for other in ("composed", "classic_torch"):
        for k, plane in ((0, "color"), (2, "depth"), (3, "alpha")):
            got, ref = _np(frames[other][k]).astype(np.float64), _np(frames["classic"][k]).astype(np.float64)
            beyond = np.abs(got - ref) > helpers.ATOL + helpers.RTOL * np.abs(ref)
            print("harness %s against classic, %s: %d of %d values beyond 1e-4, max |diff| %.3e"
                  % (other, plane, int(beyond.sum()), beyond.size, float(np.abs(got - ref).max())))
            PARITY["harness/%s_%s_beyond_1e4" % (other, plane)] = float(beyond.mean())
            assert int(beyond.sum()) <= max(helpers.MAX_BEYOND_MIN_PIXELS, helpers.MAX_BEYOND_FRAC * beyond.size)
    # the training step by both routes reaches the correction's parameters
    grads = {}
    for name, kw in (("composed", dict(composed=True)), ("classic", dict(composed=False))):
        pc.zero_grad()
        hz.corrected_train_step(world.settings, models, world.batch(), 1, visible, times, pc, cam, **kw)
        grads[name] = (pc.pose_correction_rots.grad.clone(), pc.pose_correction_trans.grad.clone())
        assert not grads[name][0][[0, 2]].any() and bool(grads[name][0][1].any()) and bool(grads[name][1][1].any())
    for p in world.params(models):
        p.grad = None
