"""The closed loop's tail, restated from the reference's lines in numpy: the contract of csrc/ego_loop.hip
(include/grpg_rasterizer.h, ``grpg_object_positions`` / ``grpg_ego_loop_step``) and the NORMATIVE statement of the
order the library fixes per rendered frame: render, detect, (a) ranging, (b) policy and control_callback, (c)
``substeps`` ticks of next_frame, the camera row of the last tick.

  simulator.py:379-399, :163-213   ``object_positions``     the loop over reversed(det), distance()
  AEB_controller.py:52-87          ``Loop.step`` (b)        perception_callback
  simulator.py:422-426             ``Loop.step`` (b)        control_callback
  simulator.py:218-242, :264-269   ``Loop.tick``            pose selection, car dynamics, forward velocity
  AEB_controller.py:90-97          ``Loop.tick``            pose_callback

``dtype=np.float64`` is the restatement, operation for operation as numpy evaluates the reference's expressions;
``dtype=np.longdouble`` is the same arithmetic in extended precision, the truth errors are measured against.  Three
reductions of the reference go to BLAS -- ``np.matmul(k_inv, depth * point_c)``, ``np.matmul(p_inv, c_position)`` and
the dot product inside ``np.linalg.norm`` -- and an x86-64 OpenBLAS evaluates a 3- or 4-term dot product as ONE fused
chain fma(a2, x2, fma(a1, x1, a0 x0)).  The float64 restatement states that chain explicitly (``fma`` below, exact
rational arithmetic, rounded once), so it does not depend on the BLAS of the machine that runs it;
tests/golden/ref_ego_loop.npz holds what the reference's own lines gave through numpy, and the two agree bit for bit.
``np.sin`` of a Python float is the C library's double sine, ``math.sin`` here.  Decisions -- comparisons, the integer
split of the stamp -- are taken from the float64 value whatever ``dtype`` is; ``margins`` reports how far each lies
from its edge.

Nothing here imports the library.  Python floats, no device.
"""
import math
from fractions import Fraction

import numpy as np

F64, LD = np.float64, np.longdouble

# the first twelve COCO names: the class list of the tests' detector
NAMES = ["person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
         "fire hydrant", "stop sign"]
KEEP = ("person", "chair", "car", "truck", "bicycle", "motorcycle", "bus", "traffic light", "stop sign")   # simulator.py:380
W, H = 160, 96
FX = 2083.09 * W / 1920


def fma(a, b, c):
    """float64 fma: exact for finite operands (rational arithmetic, one rounding); IEEE's a * b + c otherwise"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    if a == 0.0 or b == 0.0:
        return a * b + c            # keeps the sign of a zero sum
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r != 0 else a * b + c


def dot_chain(a, x, dtype=F64):
    """sum_i a[i] x[i] as BLAS evaluates it for a handful of terms: fma(a2, x2, fma(a1, x1, a0 x0)); in longdouble
    the plain ascending sum"""
    if dtype is LD:
        acc = LD(a[0]) * LD(x[0])
        for ai, xi in zip(a[1:], x[1:]):
            acc = acc + LD(ai) * LD(xi)
        return acc
    with np.errstate(all="ignore"):
        acc = float(np.float64(a[0]) * np.float64(x[0]))
    for ai, xi in zip(a[1:], x[1:]):
        acc = fma(ai, xi, acc)
    return acc


class Constants:
    """``self.extrinsics`` / ``self.intrinsics`` / ``self.cam_height`` / ``self.H`` / ``self.W`` / ``self.names`` of
    simulator.py:131-153 for the tests' 160 x 96 frame; ``k_inv`` / ``p_inv`` as ``np.linalg.inv`` gives them"""

    def __init__(self, K=None, tx=1.544414504251094167, cam_height=1.5, H=H, W=W, names=NAMES, keep=KEEP):
        self.K = np.array([[FX, 0.0, W / 2.0], [0.0, FX, H / 2.0], [0.0, 0.0, 1.0]]) if K is None else np.array(K, dtype=F64)
        self.extrinsics = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
        self.extrinsics[2, 3] = -tx
        self.cam_height, self.H, self.W = float(cam_height), int(H), int(W)
        self.names, self.keep = list(names), tuple(keep)
        self.k_inv = np.linalg.inv(self.K)
        self.p_inv = np.linalg.inv(self.extrinsics)


def xywhn(row, C):
    """``(xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()``: float32 steps, then Python floats"""
    x = np.asarray(row[:4], dtype=np.float32)
    two = np.float32(2)
    y = np.array([(x[0] + x[2]) / two, (x[1] + x[3]) / two, x[2] - x[0], x[3] - x[1]], dtype=np.float32)
    y = y / np.array([C.W, C.H, C.W, C.H], dtype=np.float32)
    return [float(v) for v in y]


def range_row(row, C, dtype=F64, plant=()):
    """one detection row -> ``(d, appended, d before the d[0] <= 0 rule)`` of simulator.py:386-399, or None when the
    class filter drops it"""
    f = dtype
    c = int(row[5])
    if not (0 <= c < len(C.names)) or C.names[c] not in C.keep:
        return None
    b = xywhn(row, C)
    u, v, h = f(b[0]) * C.W, f(b[1]) * C.H, f(b[3]) * C.H
    u1 = u
    v1 = v - h / 2 if "v_minus_h" in plant else v + h / 2
    fy = f(C.K[1, 1])
    with np.errstate(all="ignore"):
        if f is LD:
            angle_b = np.arctan((v1 - f(C.H) / 2) / fy)
            depth = (f(C.cam_height) / np.sin(angle_b)) * np.cos(angle_b)
        else:
            angle_b = math.atan((v1 - C.H / 2) / fy)
            depth = float(np.float64(C.cam_height) / np.float64(math.sin(angle_b))) * math.cos(angle_b)
        p = [depth * u1, depth * v1, depth * f(1)]
        cp = [dot_chain(C.k_inv[i], p, f) for i in range(3)] + [f(1)]
        o = [dot_chain(C.p_inv[i], cp, f) for i in range(2)]
    d = [o[0], o[1] if "sign_c1" in plant else -o[1]]
    before = list(d)
    if float(d[0]) <= 0:
        d = [f(0), f(0)]
    return d, bool(d[0] != 0 or d[1] != 0), before


def object_positions(rows, C, dtype=F64, plant=()):
    """one image's [n,6] detections -> (positions [kept,2] in the reference's order, the source row of each)"""
    order = range(len(rows)) if "no_reversed" in plant else range(len(rows) - 1, -1, -1)
    pos, src = [], []
    for i in order:
        r = range_row(rows[i], C, dtype, plant)
        if r is not None and r[1]:
            pos.append(r[0])
            src.append(i)
    return np.array(pos, dtype=dtype).reshape(-1, 2), src


def split_stamp(t):
    """the message stamp and back: float(int(t)) + float(int(t * 1e9) % 1000000000) / 1e9"""
    t = float(t)
    return float(int(t)) + float(int(t * 1e9) % 1000000000) / 1e9


class Loop:
    """The simulator and the dummy AEB controller as one object, callbacks in the fixed order."""

    def __init__(self, tape, C, *, policy="aeb", brake_distance=24.0, cipv_lat_range=1.2, period=0.02, substeps=1,
                 dtype=F64, plant=()):
        f = self.f = dtype
        self.tape, self.C, self.policy, self.plant = tape, C, policy, tuple(plant)
        self.brake_distance, self.lat, self.period, self.substeps = brake_distance, cipv_lat_range, period, int(substeps)
        self.position = [f(0), f(0), f(0)]            # last_pose_dict['position']
        self.rotation_entry = 0                       # the tape entry whose rotation last_pose_dict holds
        self.forward_velocity, self.command_brake, self.activated = f(0), f(0), False
        self.idx, self.timestamp = 1, float(tape[0]["timestamp"])
        self.cipv_lon_dist, self.lon_velocity = f(10000.0), f(0)
        self.aeb_stamp, self.aeb_z = 0.0, f(0)
        self.entry = 0
        self.k = 0

    def tick(self):
        f, T = self.f, len(self.tape)
        if self.idx < T:
            entry = self.idx
            self.timestamp = float(self.tape[entry]["timestamp"])
        else:
            entry = self.idx % T if "idx_unclamped" in self.plant else T - 1
            self.timestamp = float(self.tape[T - 1]["timestamp"]) + (self.idx - T + 1) * self.period
        if self.activated:
            velocity_step = self.forward_velocity + self.command_brake * f(self.period)
            if velocity_step < 0 and "no_clamp" not in self.plant:
                velocity_step = f(0)
            step = velocity_step * f(self.period)
            pos = [self.position[0] + step * f(0.0), self.position[1] + step * f(0.0), self.position[2] + step * f(-1.0)]
        else:
            pos = [f(v) for v in self.tape[entry]["position"]]
            self.rotation_entry = entry
        # Beyond the tape `pose` is frames[-1] tick after tick, so `self.last_pose_dict` IS `pose`: the position update
        # of :242 writes into both and :267 takes the norm of a zero vector.  (Not activated, the two positions are
        # the same entry's anyway.)
        same_dict = self.activated and self.idx >= T and self.idx >= 2
        last = pos if same_dict else self.position
        self.idx += 1
        d = [pos[i] - last[i] for i in range(3)]
        self.forward_velocity = (np.sqrt(dot_chain(d, d, f)) if f is LD else f(math.sqrt(dot_chain(d, d)))) / f(self.period)
        self.position = pos
        self.entry = entry
        current = split_stamp(self.timestamp)
        if current - self.aeb_stamp > 0:
            self.lon_velocity = (-pos[2] - (-self.aeb_z)) / f(current - self.aeb_stamp)
            self.aeb_stamp, self.aeb_z = current, pos[2]

    def step(self, dets, command=None):
        """``dets``: the [n_b,6] rows of the frame's images.  Returns the step's log row (16 values, the columns of
        ``closed_loop.LOG_FIELDS``)."""
        f = self.f
        poses = [p for rows in dets for p in object_positions(rows, self.C, f, self.plant)[0]]
        stamp = self.timestamp
        cand = [p[0] for p in poses if float(p[1]) < self.lat and float(p[1]) > -self.lat]
        cmd = 0.0
        if self.policy == "aeb":
            if cand:
                m = cand[0]
                for x in cand[1:]:            # Python's min()
                    if float(x) < float(m):
                        m = x
                self.cipv_lon_dist = m
            elif "cipv_reset" in self.plant:
                self.cipv_lon_dist = f(10000.0)
            if float(self.cipv_lon_dist) < self.brake_distance:
                v = float(self.lon_velocity)
                cmd = -13.5 if v > 2 else (-10.0 if v > 1 else (-8.0 if v > 0.001 else 0.0))
        elif command is not None:
            cmd = float(command)
        if abs(cmd) > 0:
            self.activated, self.command_brake = True, f(cmd)
        elif "release_on_zero" in self.plant:
            self.activated, self.command_brake = False, f(0)
        for _ in range(self.substeps):
            self.tick()
        self.k = min(self.k + self.substeps, len(self.tape) - 1)
        return [f(stamp), f(len(poses)), self.cipv_lon_dist, f(cmd), self.forward_velocity] + list(self.position) + \
            [f(self.activated), self.lon_velocity, self.command_brake, f(self.idx), f(self.timestamp), f(bool(cand)),
             f(self.rotation_entry), f(0)]

    def pose(self):
        """(R, T) of the frame to render next: the held rotation, the position"""
        return (np.asarray(self.tape[self.rotation_entry]["rotation_matrix"], dtype=F64),
                np.asarray([float(v) for v in self.position], dtype=F64))

    def margins(self):
        """distance of the policy's decisions from their edges, from this object's values"""
        v, c = float(self.lon_velocity), float(self.cipv_lon_dist)
        return dict(brake=abs(c - self.brake_distance), ladder=min(abs(v - 2), abs(v - 1), abs(v - 0.001)))


# ---- the camera row ----

def view_t32(R, T):
    """harness.world2view(R, T)^T in float32: rows 0-2 are R's rows, row 3 is T, the last column (0, 0, 0, 1)"""
    v = np.zeros((4, 4), dtype=np.float32)
    v[:3, :3] = np.asarray(R, dtype=F64).astype(np.float32)
    v[3, :3] = np.asarray(T, dtype=F64).astype(np.float32)
    v[3, 3] = 1.0
    return v


def camera_parts(R, T, proj_t, ray_k_inv=None, dtype=F64):
    """(view_t float32 [4,4], projection [4,4], centre [3], ray [3,3] or None) in ``dtype``, unrounded: the projection
    sum_k view_t[i][k] proj_t[k][j] and the centre -(R T) from the float32 view matrix, k ascending, one rounded
    multiply and add per term; the ray matrix R k_inv from the float32 rotation"""
    f = dtype
    v = view_t32(R, T)
    p = np.asarray(proj_t, dtype=np.float32).reshape(4, 4)
    full = np.zeros((4, 4), dtype=f)
    for i in range(4):
        for j in range(4):
            acc = f(v[i, 0]) * f(p[0, j])
            for k in range(1, 4):
                acc = acc + f(v[i, k]) * f(p[k, j])
            full[i, j] = acc
    centre = np.zeros(3, dtype=f)
    for i in range(3):
        acc = f(v[i, 0]) * f(v[3, 0])
        acc = acc + f(v[i, 1]) * f(v[3, 1])
        acc = acc + f(v[i, 2]) * f(v[3, 2])
        centre[i] = -acc
    ray = None
    if ray_k_inv is not None:
        kk = np.asarray(ray_k_inv, dtype=F64).reshape(3, 3)
        ray = np.zeros((3, 3), dtype=f)
        for i in range(3):
            for j in range(3):
                acc = f(v[i, 0]) * f(kk[0, j])
                acc = acc + f(v[i, 1]) * f(kk[1, j])
                acc = acc + f(v[i, 2]) * f(kk[2, j])
                ray[i, j] = acc
    return v, full, centre, ray


def camera_row(R, T, proj_t, ray_k_inv=None):
    """the float32 [48] row the kernel writes for a moved camera: every value rounded once"""
    v, full, centre, ray = camera_parts(R, T, proj_t, ray_k_inv)
    row = np.zeros(48, dtype=np.float32)
    row[0:16] = v.reshape(-1)
    row[16:32] = full.astype(np.float32).reshape(-1)
    row[32:35] = centre.astype(np.float32)
    if ray is not None:
        row[36:45] = ray.astype(np.float32).reshape(-1)
    return row


# ---- the inputs the golden file, the host test and the GPU test share ----

def box(u, bottom, w=16, h=12, conf=0.9, cls=2):
    """a detection row whose bottom edge is at `bottom` and whose centre column is `u`, in frame pixels"""
    return [u - w / 2.0, bottom - h, u + w / 2.0, bottom, conf, cls]


def det_rows(boxes):
    """rows in descending confidence, float32 [n,6]"""
    rows = sorted(boxes, key=lambda r: -r[4])
    return np.asarray(rows, dtype=np.float32).reshape(-1, 6)


def random_rows(n, seed, horizon=H / 2.0):
    """n rounded boxes inside the frame with classes over 0..len(NAMES)-1: bottoms below the horizon row by at least
    two pixels or above it by at least two, never on it"""
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        bottom = float(rs.randint(horizon + 2, H + 1)) if rs.rand() < 0.75 else float(rs.randint(4, horizon - 1))
        hh = float(rs.randint(2, max(3, int(bottom) - 1)))
        u = float(rs.randint(4, W - 4))
        ww = float(rs.randint(2, 40))
        x1, x2 = max(0.0, round(u - ww / 2)), min(float(W), round(u + ww / 2))
        rows.append([x1, bottom - hh, x2, bottom, 0.99 - 0.9 * i / max(n, 1) - 0.001 * rs.rand(), float(rs.randint(0, len(NAMES)))])
    return det_rows(rows)


def ranging_cases():
    """name -> list over images of [n,6] rows (n <= max_det of the name)"""
    on_horizon = [24.0 + 0, 24.0, 56.0, 48.0, 0.8, 2.0]        # yc = 36, h = 24: v1 = 36 + 12 = 48 exactly
    cases = {
        "empty_10": [np.zeros((0, 6), dtype=np.float32)],
        "one_10": [det_rows([box(84, 70)])],
        "full_10": [random_rows(10, 1)],
        "full_64": [random_rows(64, 2)],
        "filtered_10": [det_rows([box(60 + 8 * i, 60 + i, conf=0.9 - 0.05 * i, cls=c) for i, c in enumerate((4, 6, 8, 10, 4))])],
        "below_above_10": [det_rows([box(80, 90, conf=0.9), box(30, 50, conf=0.8), box(100, 40, conf=0.7),
                                     box(140, 10, h=6, conf=0.6), box(82, 49, conf=0.5)])],
        "horizon_10": [det_rows([box(70, 66, conf=0.9), on_horizon, box(90, 80, conf=0.7)])],
        "batch2_10": [random_rows(7, 3), random_rows(10, 4)],
        "batch2_64": [random_rows(64, 5), random_rows(33, 6)],
        "batch2_one_empty_10": [np.zeros((0, 6), dtype=np.float32), random_rows(3, 7)],
    }
    return cases


def max_det_of(name):
    return int(name.rsplit("_", 1)[1])


def make_tape(T=12, dt=0.02, base=1.5e9, dz=0.03):
    """a 12-entry tape: the camera drifts and moves along -z by `dz` a tick (0.03: 1.5 m/s at the simulator's 0.02 s)"""
    tape = []
    for k in range(T):
        yaw = 0.01 * k
        R = [[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]]
        ego = np.eye(4)
        ego[:3, 3] = [0.05 + 0.01 * k, -0.03, 0.1 - 0.005 * k]
        tape.append(dict(id=100 + k, frame=k % 8, timestamp=base + dt * k, rotation_matrix=R,
                         position=[0.004 * k + 0.1, -0.002 * k - 0.05, -dz * k + 0.2], ego_pose=ego.tolist()))
    return tape


def scenario(name):
    """name -> dict(tape, steps: the detections of each step (a list over images of [n,6] rows), kw of ``Loop``)

      brake     12 steps, 1 tick a step, 0.6 m/s: an object at ~30 m, an empty frame (the CIPV distance persists), from
                step 4 one at ~20 m: the brake latches at step 4 with -8, the velocity is clamped at 0 at step 7, the
                command goes back to 0 and the brake stays; the last tick lies beyond the tape
      fast      12 steps, 2 ticks a step, 2.5 m/s: the ladder's -13.5 and -10; the loop outruns the tape at step 5,
                where the reference's pose dictionary becomes its own predecessor and the velocity drops to 0 at once
      cruise    12 steps, 1 tick a step, nothing nearer than the brake distance, one frame with candidates only outside
                the lateral range: never activated; idx passes the end of the tape
      commanded policy=None: commands 0, 0, -6.0, 0, ... from the caller"""
    tape = make_tape()
    far, near, side = box(82, 57, conf=0.9), box(84, 61, conf=0.9), box(10, 60, conf=0.6)
    braking = [[det_rows([far, side])], [det_rows([far])], [np.zeros((0, 6), dtype=np.float32)], [det_rows([side, far])]] + \
        [[det_rows([near, side, box(120, 30, conf=0.5)])]] * 4 + [[det_rows([box(84, 63)])]] * 4
    if name == "brake":
        return dict(tape=make_tape(dz=0.012), steps=braking, kw=dict(policy="aeb", substeps=1), commands=None)
    if name == "fast":
        return dict(tape=make_tape(dz=0.05), steps=braking, kw=dict(policy="aeb", substeps=2), commands=None)
    if name == "cruise":
        steps = [[det_rows([far])]] * 5 + [[det_rows([side])]] + [[det_rows([far, box(86, 56, cls=4)])]] * 6
        return dict(tape=tape, steps=steps, kw=dict(policy="aeb", substeps=1), commands=None)
    if name == "commanded":
        steps = [[det_rows([far])]] * 12
        return dict(tape=tape, steps=steps, kw=dict(policy=None, substeps=1),
                    commands=[0.0, 0.0, -6.0, 0.0, 0.0, -20.0] + [0.0] * 6)
    raise KeyError(name)


SCENARIOS = ("brake", "fast", "cruise", "commanded")


def run_scenario(name, C=None, dtype=F64, plant=()):
    """-> (log [steps,16] in dtype, the (R, T) each frame AFTER the first is rendered with, the Loop)"""
    sc = scenario(name)
    loop = Loop(sc["tape"], C or Constants(), dtype=dtype, plant=plant, **sc["kw"])
    rows, poses = [], []
    for i, dets in enumerate(sc["steps"]):
        rows.append(loop.step(dets, None if sc["commands"] is None else sc["commands"][i]))
        poses.append(loop.pose())
    return np.array(rows, dtype=dtype), poses, loop
