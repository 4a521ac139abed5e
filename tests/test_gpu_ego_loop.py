"""GPU tests of the closed loop's tail: ``closed_loop.object_positions`` / ``closed_loop.EgoLoop`` -> C ABI
``grpg_object_positions`` / ``grpg_ego_loop_step`` -> csrc/ego_loop.hip, and ``FrameSession.frame(k, camera=CameraRow)``.

The yardstick is tests/loop_truth.py: the reference's lines restated in numpy float64 (pinned to the reference's own
results by tests/test_ego_loop_host.py) and, for the ranging, the same in longdouble.  Frames are 160 x 96, the
background 2 000 Gaussians, two small actors, the tape 12 entries; ``bs`` 1 and 2, ``max_det`` 10 and 64.

  ranging    kept count and order exact; positions within 4 x the float64 restatement's own distance from the
             longdouble truth, maximum over each group of cases (the device's atan / sin / cos are not the C library's);
             the box on the horizon row: the same kept flag, both results non-finite
  dynamics, policy, state, log, camera row    bit for bit: no transcendental is involved
No test provokes a fault: refusals are made on the host, before anything is enqueued, and that is what is asserted."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import loop_truth as lt
import test_gpu_session as tgs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
W, H, T = lt.W, lt.H, 12
BOUND = 4.0        # the project's standing margin for "as good as the reference's arithmetic"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (no ROCm device visible)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def C():
    return lt.Constants()


@pytest.fixture(scope="module")
def ranging(C):
    from gaussianrpg_amd import closed_loop as cl
    return cl.Ranging(C.K, C.extrinsics, C.cam_height, C.H, C.W, names=lt.NAMES)


def det_tensors(images, max_det, dev):
    """list over images of [n,6] rows -> (det [bs,max_det,6] with zeros below the count, count)"""
    det = np.zeros((len(images), max_det, 6), dtype=np.float32)
    for b, rows in enumerate(images):
        det[b, :len(rows)] = rows
    count = np.asarray([len(r) for r in images], dtype=np.int32)
    return torch.from_numpy(det).to(dev), torch.from_numpy(count).to(dev)


# ---- ranging ----

def measure_ranging(dev, ranging, C):
    """every case on the device and in both truths -> {case: dict(n, kept rows, errors)}; asserts what is exact"""
    from gaussianrpg_amd import closed_loop as cl
    out = {}
    for name, images in lt.ranging_cases().items():
        max_det = lt.max_det_of(name)
        det, count = det_tensors(images, max_det, dev)
        pos, n = cl.object_positions(det, count, ranging)
        pos, n = pos.cpu().numpy(), n.cpu().numpy()
        assert pos.shape == (len(images), max_det, 2) and pos.dtype == np.float64
        err_dev, err_f64, kept = [], [], 0
        for b, rows in enumerate(images):
            want64, src64 = lt.object_positions(rows, C)
            truth, src = lt.object_positions(rows, C, lt.LD)
            assert src == src64                                           # the case has its margin: both truths agree
            assert int(n[b]) == len(src), "%s image %d: kept %d, truth %d" % (name, b, n[b], len(src))
            assert not pos[b, len(src):].any()                            # zeros below n
            got = pos[b, :len(src)]
            finite = np.isfinite(truth.astype(np.float64)).all(axis=1) if len(src) else np.zeros(0, dtype=bool)
            assert (np.isfinite(got).all(axis=1) == finite).all()         # on the horizon: non-finite in both
            # order: the truth's rows are distinct, so the nearest truth row of each device row is its own
            for i in np.nonzero(finite)[0]:
                d = np.abs(truth[finite].astype(np.float64) - got[i]).sum(axis=1)
                assert int(np.argmin(d)) == int(np.count_nonzero(finite[:i])), "%s image %d: order" % (name, b)
            if finite.any():
                err_dev.append(np.abs(got[finite].astype(lt.LD) - truth[finite]).max())
                err_f64.append(np.abs(want64[finite].astype(lt.LD) - truth[finite]).max())
            kept += len(src)
        out[name] = dict(kept=kept, err_dev=float(max(err_dev, default=0.0)), err_f64=float(max(err_f64, default=0.0)))
    return out


@pytest.fixture(scope="module")
def measured(dev, ranging, C):
    return measure_ranging(dev, ranging, C)


def test_ranging_cases_hold_their_margins(C):
    for name, images in lt.ranging_cases().items():
        for rows in images:
            for row in rows:
                r = lt.range_row(row, C, lt.LD)
                if r is not None and np.isfinite(np.asarray(r[2], dtype=np.float64)).all():
                    assert abs(float(r[2][0])) > 1e-3, name


def test_ranging_kept_count_and_order(measured):
    assert measured["empty_10"]["kept"] == 0 and measured["one_10"]["kept"] == 1 and measured["filtered_10"]["kept"] == 0
    assert measured["below_above_10"]["kept"] == 3 and measured["horizon_10"]["kept"] == 3
    assert measured["full_64"]["kept"] > 20 and measured["batch2_64"]["kept"] > 40


@pytest.mark.parametrize("group", ["10", "64"])
def test_ranging_accuracy(measured, group):
    cases = [m for name, m in measured.items() if name.endswith("_" + group) and m["kept"]]
    err_dev, err_f64 = max(m["err_dev"] for m in cases), max(m["err_f64"] for m in cases)
    print("max_det %s: device %.3e, float64 restatement %.3e from the longdouble truth, ratio %.3f"
          % (group, err_dev, err_f64, err_dev / err_f64))
    assert err_f64 > 0
    assert err_dev <= BOUND * err_f64


def test_count_is_clamped_and_stale_rows_are_not_read(dev, ranging, C):
    """rows at and beyond count[b] are not looked at, whatever they hold; a count beyond max_det means max_det"""
    from gaussianrpg_amd import closed_loop as cl
    rows = lt.random_rows(10, 1)
    det, count = det_tensors([rows], 10, dev)
    det[0, 6:] = float("nan")
    count[0] = 6
    pos, n = cl.object_positions(det, count, ranging)
    want, src = lt.object_positions(rows[:6], C)
    assert int(n[0]) == len(src) and not pos[0, len(src):].cpu().numpy().any()
    det, count = det_tensors([rows], 10, dev)
    count[0] = 1000
    assert int(cl.object_positions(det, count, ranging)[1][0]) == len(lt.object_positions(rows, C)[1])


# ---- the world ----

class World:
    def __init__(self, dev):
        from gaussianrpg_amd import harness as hz
        from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
        g = torch.Generator().manual_seed(29)
        self.dev = dev
        self.background = tgs._raw(hz.toy_scene(2000, seed=3, sh_degree=1, depth=6.0), dev, g, grad=False)
        self.actor_models = []
        for k, (n, f) in enumerate(((24, 1), (40, 2))):
            o = hz.toy_scene(n, seed=50 + k, sh_degree=1, depth=0.0, spread=0.3, scale=0.06)
            self.actor_models.append(tgs._raw(hz.Scene(o.means3D, o.opacity.clamp(min=0.6), o.scales, o.rotations, o.shs, 1),
                                              dev, g, f, grad=False))
        self.actors, _ = tgs._actors(dev, ((-1.0, 4.5), (0.8, 5.0)), ((0, 7), (0, 7)), 8)
        cam = hz.trajectory_camera(0, W=W, H=H, device=dev)
        self.settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1, bg=torch.tensor([0.2, 0.1, 0.3], device=dev)))
        self.sky = torch.rand(6, 8, 8, 3, generator=g).to(dev)
        self._made = {}

    def scene(self, tape_of="brake", sky=False):
        from gaussianrpg_amd import harness as hz
        from gaussianrpg_amd.session import FrameSession
        key = (tape_of, sky)
        if key not in self._made:
            sc = hz.ClosedLoopScene(self.settings, self.background, self.actor_models, self.actors,
                                    lt.scenario(tape_of)["tape"], [(0, 7, 1.0), (0, 7, 0.5)],
                                    sky_cube=self.sky if sky else None)
            self._made[key] = (sc, FrameSession(*sc[:6], **sc.options()))
        return self._made[key]


@pytest.fixture(scope="module")
def world(dev):
    return World(dev)


def run_device(world, ranging, name, bs=1, max_det=10, sky=False):
    """the scenario through EgoLoop -> (log, the camera row after every step, the loop, the truth's run)"""
    from gaussianrpg_amd import closed_loop as cl
    sc = lt.scenario(name)
    _, session = world.scene(name, sky)
    extra = [lt.det_rows([lt.box(10, 60, conf=0.6), lt.box(150, 70, conf=0.5)])] if bs == 2 else []
    steps = [dets + extra for dets in sc["steps"]]
    loop = cl.EgoLoop(session, ranging, steps=len(steps), **sc["kw"])
    rows, ks = [], []
    for i, dets in enumerate(steps):
        det, count = det_tensors(dets, max_det, world.dev)
        loop.step(det, count, None if sc["commands"] is None else sc["commands"][i])
        rows.append(loop.camera.row.clone())
        ks.append(loop.k)
    truth = lt.Loop(sc["tape"], lt.Constants(), **sc["kw"])
    want, poses = [], []
    for i, dets in enumerate(steps):
        want.append(truth.step(dets, None if sc["commands"] is None else sc["commands"][i]))
        poses.append((truth.pose(), truth.activated, truth.entry))
    return loop.log(), [r.cpu().numpy() for r in rows], ks, loop, np.array(want, dtype=np.float64), poses, truth


# ---- dynamics, policy, state, log, camera row: bit for bit ----

@pytest.mark.parametrize("shape", [(1, 10), (2, 64)], ids=["bs1_det10", "bs2_det64"])
@pytest.mark.parametrize("name", lt.SCENARIOS)
def test_scenario_bit_for_bit(world, ranging, name, shape):
    from gaussianrpg_amd import closed_loop as cl
    log, rows, ks, loop, want, poses, truth = run_device(world, ranging, name, *shape, sky=True)
    assert log.shape == want.shape == (12, 16)
    bad = np.argwhere(log.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, "log differs at (step, column) %s: %r against %r" % (
        bad[:4].tolist(), log[tuple(bad[0])] if len(bad) else None, want[tuple(bad[0])] if len(bad) else None)
    if name == "brake":
        assert log[:, 8].tolist() == [0.0] * 4 + [1.0] * 8 and log[7, 4] > 0 and (log[8:, 4] == 0).all()
    state = loop.state()
    assert state["idx"] == want[-1, 11] and state["forward_velocity"] == want[-1, 4]
    assert state["cipv_lon_dist"] == want[-1, 2] and state["lon_velocity"] == want[-1, 9]
    assert [state["position_x"], state["position_y"], state["position_z"]] == want[-1, 5:8].tolist()
    assert state["aeb_stamp"] == truth.aeb_stamp and state["aeb_z"] == float(truth.aeb_z)
    # the camera row: the session's own row of the entry until the brake is pressed, the restated arithmetic after
    _, session = world.scene(name, True)
    baked = session._cameras.cpu().numpy()
    el = cl.EgoLoop(session, ranging)
    for i, ((R, Tv), activated, entry) in enumerate(poses):
        assert ks[i] == min((i + 1) * lt.scenario(name)["kw"]["substeps"], T - 1)
        expect = lt.camera_row(R, Tv, el._proj_t, session._Kinv) if activated else baked[entry]
        assert rows[i].tobytes() == expect.tobytes(), "camera row after step %d (activated %s)" % (i, activated)
    if name != "cruise":
        assert any(a for _, a, _ in poses) and np.abs(rows[-1][36:45]).max() > 0


def test_command_from_a_device_tensor(world, ranging):
    from gaussianrpg_amd import closed_loop as cl
    sc = lt.scenario("commanded")
    _, session = world.scene("commanded")
    loop = cl.EgoLoop(session, ranging, steps=12, **sc["kw"])
    commands = torch.tensor(sc["commands"], dtype=torch.float64, device=world.dev)
    for i, dets in enumerate(sc["steps"]):
        loop.step(*det_tensors(dets, 10, world.dev), commands[i:i + 1])
    want = lt.run_scenario("commanded")[0]
    assert loop.log().tobytes() == want.astype(np.float64).tobytes()
    with pytest.raises(ValueError, match="policy=None"):
        cl.EgoLoop(session, ranging).step(*det_tensors(sc["steps"][0], 10, world.dev), 1.0)


def test_reset_and_determinism(world, ranging):
    a = run_device(world, ranging, "fast")
    b = run_device(world, ranging, "fast")
    assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    loop = a[3]
    loop.reset()
    assert loop.k == 0 and loop.num_steps == 0 and loop.state()["idx"] == 1.0 and loop.state()["cipv_lon_dist"] == 10000.0
    sc = lt.scenario("fast")
    for dets in sc["steps"]:
        loop.step(*det_tensors(dets, 10, world.dev))
    assert loop.log().tobytes() == a[0].tobytes()
    with pytest.raises(IndexError, match="full"):
        loop.step(*det_tensors(sc["steps"][0], 10, world.dev))


# ---- plumbing: the device row as the frame's camera ----

@pytest.mark.parametrize("sky", [False, True], ids=["plain", "sky"])
def test_frame_from_the_device_row(world, ranging, sky):
    from gaussianrpg_amd.session import CameraRow
    _, _, ks, loop, _, poses, _ = run_device(world, ranging, "brake", sky=sky)
    _, session = world.scene("brake", sky)
    assert poses[-1][1] and isinstance(loop.camera, CameraRow)
    rs = world.settings
    for k in (loop.k, 3):
        a = session.frame(k, camera=loop.camera, planes=True)
        b = session.frame(k, camera=loop.camera.tensors(H, W, rs.tanfovx, rs.tanfovy), planes=True)
        tgs._same(a, b, "frame %d from the device row" % k)
        assert int(a["rgb8"].max()) > 0
    tape_row = CameraRow(session._cameras[5].clone())
    tgs._same(session.frame(5, camera=tape_row, planes=True), session.frame(5, planes=True), "the tape's own row")
    with pytest.raises(ValueError, match="K cannot be given"):
        session.frame(2, camera=loop.camera, K=np.eye(3))
    with pytest.raises(ValueError, match="host"):         # CameraTensors on the device keep raising
        from gaussianrpg_amd.session import camera_from_pose
        session.frame(2, camera_from_pose(np.eye(3), np.zeros(3), W, H, device=world.dev))


# ---- heads that decode to a scenario's detections ----

ANCHOR, STRIDE, NA = 40.0, 32, 3


def heads_for(rows, dev):
    """one detector level [1, NA * (5 + nc), H/32, W/32] whose decode + NMS + mapping gives exactly `rows`' boxes and
    classes (the confidences to ~1e-5): every box in the cell of its centre, one anchor per box of a cell"""
    nc, ny, nx = len(lt.NAMES), H // STRIDE, W // STRIDE
    head = np.full((1, NA, 5 + nc, ny, nx), -12.0, dtype=np.float32)
    used = {}
    logit = lambda s: math.log(s / (1.0 - s))      # noqa: E731
    for x1, y1, x2, y2, conf, cls in np.asarray(rows, dtype=np.float64):
        cx, cy, w, h = (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1
        gx, gy = min(int(cx // STRIDE), nx - 1), min(int(cy // STRIDE), ny - 1)
        a = used.get((gx, gy), 0)
        used[(gx, gy)] = a + 1
        assert a < NA
        head[0, a, 0, gy, gx] = logit(((cx / STRIDE - gx) + 0.5) / 2)
        head[0, a, 1, gy, gx] = logit(((cy / STRIDE - gy) + 0.5) / 2)
        head[0, a, 2, gy, gx] = logit(math.sqrt(w / ANCHOR) / 2)
        head[0, a, 3, gy, gx] = logit(math.sqrt(h / ANCHOR) / 2)
        head[0, a, 4, gy, gx] = logit(conf)
        head[0, a, 5 + int(cls), gy, gx] = 12.0
    return [torch.from_numpy(head.reshape(1, NA * (5 + nc), ny, nx)).to(dev)]


@pytest.fixture(scope="module")
def detector(dev):
    from gaussianrpg_amd.perception import DetectGeometry, LetterboxPlan
    geom = DetectGeometry(np.full((1, NA, 2), ANCHOR, dtype=np.float32), [float(STRIDE)], len(lt.NAMES))
    return geom, LetterboxPlan.for_simulator(H, W)


def test_crafted_heads_give_the_scenario_rows(dev, detector):
    from gaussianrpg_amd.perception import detections_from_heads
    geom, plan = detector
    for dets in lt.scenario("brake")["steps"]:
        det, count = detections_from_heads(heads_for(dets[0], dev), geom, max_det=10, plan=plan)
        n = int(count[0])
        got = det[0, :n].cpu().numpy()
        assert n == len(dets[0])
        assert np.array_equal(got[:, [0, 1, 2, 3, 5]], dets[0][:, [0, 1, 2, 3, 5]])
        assert n == 0 or np.abs(got[:, 4] - dets[0][:, 4]).max() < 1e-4


_HEADS = {}


def _run(world, ranging, detector, name, device_loop, steps=None, **kw):
    from gaussianrpg_amd import harness as hz
    geom, plan = detector
    sc = lt.scenario(name)
    scene, session = world.scene(name, True)
    if name not in _HEADS:           # uploaded once: an upload waits for the device
        _HEADS[name] = [heads_for(dets[0], world.dev) for dets in sc["steps"]]
    heads = _HEADS[name]
    steps = len(heads) if steps is None else steps
    return hz.closed_loop_run(scene, lambda i, frame: heads[min(i, len(heads) - 1)], steps, device_loop=device_loop,
                              session=session, ranging=ranging, geom=geom, plan=plan, max_det=10, **sc["kw"], **kw)


# ---- no host wait ----

def test_no_host_wait_until_the_log_is_read(world, ranging, detector):
    """12 steps, then the 200-step scenario: render, detect, step -- enqueued with no synchronisation torch can see"""
    from gaussianrpg_amd import closed_loop as cl
    _run(world, ranging, detector, "brake", True)            # capacities learnt, blobs grown
    _, session = world.scene("brake", True)
    kw = lt.scenario("brake")["kw"]
    loops = [cl.EgoLoop(session, ranging, steps=n, **kw) for n in (12, 200)]     # (the tape's upload waits: done here)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        short = _run(world, ranging, detector, "brake", True, read=False, loop=loops[0])
        long = _run(world, ranging, detector, "brake", True, steps=200, read=False, loop=loops[1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert short["log"] is None
    log = short["loop"].log()
    assert log.tobytes() == lt.run_scenario("brake")[0].astype(np.float64).tobytes()
    log200 = long["loop"].log()
    assert log200.shape == (200, 16) and log200[:12].tobytes() == log.tobytes()
    assert log200[-1, 11] == 201.0 and log200[-1, 4] == 0.0 and log200[-1, 8] == 1.0


# ---- both routes of closed_loop_run ----

def test_device_route_equals_the_host_route(world, ranging, detector):
    """The logs agree (decisions exactly, values to 1e-12: the host route's numpy goes through the machine's BLAS).
    The brake is pressed at step 4, so frames 0-4 are rendered from the tape's cameras -- rows and frame bytes equal
    bit for bit -- and frame 5 is the first a moved camera renders: from there the host route's float32 product and
    float32 inverse may round the projection and the centre differently, and the frames are not compared."""
    a = _run(world, ranging, detector, "brake", True, keep_frames=True, keep_rows=True)
    b = _run(world, ranging, detector, "brake", False, keep_frames=True, keep_rows=True)
    assert a["log"].tobytes() == lt.run_scenario("brake")[0].astype(np.float64).tobytes()
    exact = [1, 3, 8, 11, 13, 14]
    assert np.array_equal(a["log"][:, exact], b["log"][:, exact])
    np.testing.assert_allclose(b["log"], a["log"], rtol=1e-12, atol=1e-300)
    first_moved = 5
    rows_a = [r.cpu().numpy() for r in a["rows"]]
    for i in range(12):
        same_row = rows_a[i].tobytes() == b["rows"][i].tobytes()
        assert same_row or i >= first_moved, "camera rows differ at frame %d" % i
        if i < first_moved:
            assert torch.equal(a["frames"][i], b["frames"][i]), "frame %d" % i
        else:       # the view matrix and the ray matrix are the same bits on both routes all the way
            assert rows_a[i][:16].tobytes() == b["rows"][i][:16].tobytes()
            assert rows_a[i][36:].tobytes() == b["rows"][i][36:].tobytes()
            np.testing.assert_allclose(rows_a[i], b["rows"][i], rtol=2e-6, atol=1e-6)
    assert int(a["frames"][0].max()) > 0


# ---- the C ABI refuses before it enqueues ----

class _Ranging(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int), ("width", ctypes.c_int), ("nc", ctypes.c_int), ("reserved", ctypes.c_int),
                ("class_mask", ctypes.c_ulonglong * 2), ("fy", ctypes.c_double), ("cam_height", ctypes.c_double),
                ("k_inv", ctypes.c_double * 9), ("p_inv", ctypes.c_double * 16)]


class _Positions(ctypes.Structure):
    _fields_ = [("det", ctypes.c_void_p), ("count", ctypes.c_void_p), ("bs", ctypes.c_int), ("max_det", ctypes.c_int),
                ("ranging", _Ranging), ("pos", ctypes.c_void_p), ("n", ctypes.c_void_p), ("hip_stream", ctypes.c_void_p)]


class _Step(ctypes.Structure):
    _fields_ = [("detections", _Positions), ("policy", ctypes.c_int), ("substeps", ctypes.c_int),
                ("tape_len", ctypes.c_int), ("has_ray", ctypes.c_int), ("brake_distance", ctypes.c_double),
                ("cipv_lat_range", ctypes.c_double), ("command", ctypes.c_double), ("period", ctypes.c_double),
                ("command_device", ctypes.c_void_p), ("tape", ctypes.c_void_p), ("cameras", ctypes.c_void_p),
                ("proj_t", ctypes.c_float * 16), ("ray_k_inv", ctypes.c_double * 9), ("state", ctypes.c_void_p),
                ("log", ctypes.c_void_p), ("log_rows", ctypes.c_longlong), ("log_index", ctypes.c_longlong),
                ("camera", ctypes.c_void_p)]


def test_c_abi_refusals(dev):
    lib = ctypes.CDLL(LIB)
    lib.grpg_last_error.restype = ctypes.c_char_p
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)      # noqa: E731
    det, count = torch.zeros(1, 10, 6, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    pos, n = f64(1, 64, 2), torch.zeros(1, dtype=torch.int32, device=dev)
    tape, cameras, state, log, camera = f64(12, 13), torch.zeros(12, 48, device=dev), f64(16), f64(4, 16), torch.zeros(48, device=dev)
    state_before = state.clone()

    def request(**change):
        q = _Step()
        d = q.detections
        d.det, d.count, d.bs, d.max_det, d.pos, d.n = det.data_ptr(), count.data_ptr(), 1, 10, pos.data_ptr(), n.data_ptr()
        d.ranging.height, d.ranging.width, d.ranging.nc, d.ranging.fy, d.ranging.cam_height = H, W, 12, 100.0, 1.5
        q.policy, q.substeps, q.tape_len, q.period = 1, 1, 12, 0.02
        q.tape, q.cameras, q.state, q.camera = tape.data_ptr(), cameras.data_ptr(), state.data_ptr(), camera.data_ptr()
        q.log, q.log_rows, q.log_index = log.data_ptr(), 4, 0
        for key, value in change.items():
            target = q
            for part in key.split("__")[:-1]:
                target = getattr(target, part)
            setattr(target, key.split("__")[-1], value)
        return q

    cases = [(dict(detections__max_det=65), b"max_det must lie in [1, 64]"), (dict(detections__max_det=0), b"max_det"),
             (dict(detections__ranging__nc=129), b"nc must lie in [0, 128]"), (dict(substeps=0), b"substeps must be at least 1"),
             (dict(log_index=4), b"outside the log"), (dict(log_index=-1), b"outside the log"),
             (dict(detections__det=None), b"NULL"), (dict(state=None), b"NULL"), (dict(camera=None), b"NULL"),
             (dict(tape_len=0), b"tape is empty"), (dict(policy=7), b"policy"), (dict(period=0.0), b"period")]
    for change, text in cases:
        q = request(**change)
        assert lib.grpg_ego_loop_step(ctypes.byref(q)) == -1, change
        assert text in lib.grpg_last_error(), (change, lib.grpg_last_error())
    for change, text in cases[:3] + [cases[6]]:
        q = request(**change)
        assert lib.grpg_object_positions(ctypes.byref(q.detections)) == -1 and text in lib.grpg_last_error()
    assert lib.grpg_ego_loop_step(None) == -1 and lib.grpg_object_positions(None) == -1
    torch.cuda.synchronize()
    assert torch.equal(state, state_before) and not log.any() and not camera.any()      # nothing was enqueued
    from gaussianrpg_amd import closed_loop as cl
    with pytest.raises(ValueError, match=r"max_det must lie in \[1, 64\]"):
        cl.object_positions(torch.zeros(1, 65, 6, device=dev), count, cl.Ranging(np.eye(3), np.eye(4), 1.5, H, W))
