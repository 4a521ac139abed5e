"""Not a test: the tracklet -> actor-pose contract of gaussianrpg_amd/tracks.py (csrc/tracks.hip) restated in torch on
the CPU, line by line after ``ActorPose`` (lib/models/actor_pose.py:83-179) and ``StreetGaussianModel.parse_camera``
(lib/models/street_gaussian_model.py:268-274) with the helpers of lib/utils/general.py:148-276 -- parametrised by
dtype: float32 is the arithmetic the reference runs (tests/test_tracks_golden.py pins it bit for bit to the reference's
own output), float64 is the truth the GPU tests measure against.  ``roma.utils.unitquat_slerp`` is written out as
DESIGN.md section 21 defines it (``unitquat_slerp`` below): roma is not installed, its float32 bits are not pinned.

Also the input builders (legacy ``RandomState``: stable) and the comparator the GPU tests use, with the planted
errors (``variant=``) tests/test_tracks_host.py holds the comparator against.
"""
import hashlib

import numpy as np
import torch

BASE = 1.5e9          # Waymo stamps: about 1.5e9 s, 0.1 s apart
EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 4.0          # float32 formulas against a float64 truth: the project's margin (README, preprocess backward)
FLOOR_ULPS = 4.0      # where the restatement happens to be exact
SMALL_C = 1.0 - 1e-5  # the slerp's series branch
VARIANTS = ("swap", "bracket", "stamps32", "no_sign", "half_angle", "no_normalize", "ego_right", "weights_swapped")


# ---- lib/utils/general.py, restated ----

def quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    ow = aw * bw - ax * bx - ay * by - az * bz
    ox = aw * bx + ax * bw + ay * bz - az * by
    oy = aw * by - ax * bz + ay * bw + az * bx
    oz = aw * bz + ax * by - ay * bx + az * bw
    return torch.stack((ow, ox, oy, oz), -1)


def _sqrt_positive_part(x):
    ret = torch.zeros_like(x)
    positive_mask = x > 0
    ret[positive_mask] = torch.sqrt(x[positive_mask])
    return ret


def matrix_to_quaternion(matrix):
    batch_dim = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch_dim + (9,)), dim=-1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                             1.0 - m00 - m11 + m22], dim=-1))
    quat_by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    flr = torch.tensor(0.1).to(dtype=q_abs.dtype, device=q_abs.device)
    quat_candidates = quat_by_rijk / (2.0 * q_abs[..., None].max(flr))
    return quat_candidates[torch.nn.functional.one_hot(q_abs.argmax(dim=-1), num_classes=4) > 0.5, :].reshape(
        batch_dim + (4,))


def unitquat_slerp(q0, q1, steps, shortest_arc=True):
    """The stand-in for roma.utils.unitquat_slerp on (x,y,z,w) unit quaternions [B,4] and steps [S] -> [S,B,4]: the
    geodesic through q0, (sin((1-s) W) q0 + sin(s W) sg q1) / sin W with sg = sign(q0 . q1) (shortest arc), c =
    min(|q0 . q1|, 1), W = acos(c); for c > 1 - 1e-5 the series k (1 + (1 - k^2)(1 - c) / 3) of sin(k W) / sin W
    (W^2 = 2 (1 - c) + ...), which returns q0 for equal rotations.  Valid for s outside [0, 1]."""
    dot = (q0 * q1).sum(-1)
    sigma = torch.where(dot < 0, -torch.ones_like(dot), torch.ones_like(dot)) if shortest_arc else torch.ones_like(dot)
    c = dot.abs().clamp(max=1.0) if shortest_arc else dot.clamp(min=-1.0, max=1.0)
    small = c > SMALL_C
    om = torch.acos(torch.where(small, torch.zeros_like(c), c))     # pi / 2 where the series applies: no 0 / 0
    s = steps.to(q0.dtype).reshape(-1, 1)
    s1 = 1 - s
    w3 = (1 - c) / 3
    a = torch.where(small, s1 * (1 + (1 - s1 * s1) * w3), torch.sin(s1 * om) / torch.sin(om))
    b = torch.where(small, s * (1 + (1 - s * s) * w3), torch.sin(s * om) / torch.sin(om))
    return a[..., None] * q0 + (b * sigma)[..., None] * q1


def quaternion_slerp(q0, q1, step, dtype=torch.float32, normalize=True, shortest_arc=True):
    """general_utils.py:256-276; ``steps`` is .float() there (the reference runs float32), ``dtype`` here"""
    ndim = q0.ndim
    if ndim == 1:
        q0 = q0.unsqueeze(0)
        q1 = q1.unsqueeze(0)
    if normalize:
        q0 = torch.nn.functional.normalize(q0)
        q1 = torch.nn.functional.normalize(q1)
    q0 = q0[..., [1, 2, 3, 0]]
    q1 = q1[..., [1, 2, 3, 0]]
    steps = torch.tensor([step]).to(dtype)
    q = unitquat_slerp(q0, q1, steps, shortest_arc)
    q = q[..., [3, 0, 1, 2]].squeeze(0)
    if ndim == 1:
        q = q.squeeze(0)
    return q


# ---- a case: tracklets, stamps, obj_info ----

class Case:
    """tracklets [F,M,8] (values exact in float32), stamps float64 [F], obj_info {id: start / end}, and optionally
    camera_timestamps {cam: {'train_timestamps': [...]}}."""

    def __init__(self, tracklets, stamps, obj_info, camera_timestamps=None):
        self.tracklets = np.asarray(tracklets, dtype=np.float32).astype(np.float64)
        self.stamps = np.asarray(stamps, dtype=np.float64)
        self.obj_info = obj_info
        self.camera_timestamps = camera_timestamps
        self.ids = list(obj_info.keys())
        t = torch.from_numpy(self.tracklets).float()
        self.track_idx = [torch.argwhere(t[..., 0] == i).numpy() for i in self.ids]     # actor_pose.py:30

    @property
    def shape(self):
        return self.tracklets.shape[0], self.tracklets.shape[1], len(self.ids)

    def sha256(self):
        h = hashlib.sha256()
        h.update(self.tracklets.astype(np.float32).tobytes())
        h.update(self.stamps.tobytes())
        return h.hexdigest()


def yaw_quat(yaw):
    return np.array([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])


def _qmul_np(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rand_pose(rng, a, f):
    """a car on a gentle curve: position along a path, yaw plus a small tilt, a norm that is not exactly one"""
    trans = np.array([12.0 * a + 1.7 * f, -4.0 + 0.4 * f * (a + 1), 0.8]) + rng.normal(0, 0.05, 3)
    tilt = np.concatenate([[1.0], rng.normal(0, 0.02, 3)])
    q = _qmul_np(yaw_quat(0.4 * a + 0.06 * f + rng.normal(0, 0.01)), tilt / np.linalg.norm(tilt))
    return trans, q * (1.0 + rng.normal(0, 0.01))


def _empty(F, M):
    tr = np.zeros((F, M, 8))
    tr[..., 0] = -1.0     # padded cells
    tr[..., 4] = 1.0
    return tr


def small_scene(seed=0, step=0.1):
    """F = 8, M = 3, three actors in obj_info's order: id 3 in column 0 throughout; id 5 lives in frames 2-5 only (and
    changes column): the inactive actor in the middle of a batch; id 11 changes column at frame 4; id 7, which obj_info
    does not list, in two cells; the rest padded with -1.  Two training cameras' stamps between the tracklet stamps."""
    rng = np.random.RandomState(seed)
    F, M = 8, 3
    stamps = BASE + step * np.arange(F)
    tr = _empty(F, M)
    cells = {3: [(f, 0) for f in range(F)], 11: [(f, 1 if f < 4 else 2) for f in range(F)],
             5: [(2, 2), (3, 2), (4, 1), (5, 1)], 7: [(6, 1), (7, 1)]}
    for a, (i, where) in enumerate(cells.items()):
        for f, c in where:
            trans, q = _rand_pose(rng, a, f)
            tr[f, c] = np.concatenate([[i], trans, q])
    tr[5, 0, 4:8] *= -1.0     # q0 . q1 < 0 between frames 4 / 5 and 5 / 6 of actor 0
    info = {3: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1]),
            5: dict(start_timestamp=stamps[2], end_timestamp=stamps[5]),
            11: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1])}
    cams = {0: dict(train_timestamps=list(BASE + step * (np.arange(0, F, 2) + 0.31))),       # every other frame
            1: dict(train_timestamps=list(BASE + step * np.array([2.9])))}                    # one stamp: the fallback
    return Case(tr, stamps, info, cams)


def long_track(L, seed=0, step=0.1, irregular=False):
    """One actor over L frames in a single column (M = 2, the other column padded) plus a two-entry actor."""
    rng = np.random.RandomState(1000 + L + seed)
    F, M = max(L, 2), 2
    stamps = BASE + (np.cumsum(rng.uniform(0.02, 0.3, F)) if irregular else step * np.arange(F))
    tr = _empty(F, M)
    for f in range(L):
        trans, q = _rand_pose(rng, 0, f % 50)
        tr[f, 0] = np.concatenate([[1], trans, q])
    for f in (0, F - 1):
        trans, q = _rand_pose(rng, 1, f % 50)
        tr[f, 1] = np.concatenate([[2], trans, q])
    info = {1: dict(start_timestamp=stamps[0], end_timestamp=stamps[L - 1]),
            2: dict(start_timestamp=stamps[0], end_timestamp=stamps[F - 1])}
    return Case(tr, stamps, info)


def tie_scene():
    """stamps exact in binary (0.125 s apart): a query on entry k's own stamp leaves k - 1 and k + 1 at the same
    distance, and the lower list position wins."""
    c = long_track(9, seed=5, step=0.125)
    assert np.all((c.stamps - BASE) * 8 == np.arange(9))
    return c


def same_side_scene():
    """an irregular track with a gap: for a query just behind the gap the two closest entries both lie before it"""
    rng = np.random.RandomState(77)
    F, M = 6, 1
    stamps = BASE + np.array([0.0, 0.1, 0.2, 0.3, 1.3, 1.4])
    tr = _empty(F, M)
    for f in range(F):
        trans, q = _rand_pose(rng, 0, f)
        tr[f, 0] = np.concatenate([[4], trans, q])
    return Case(tr, stamps, {4: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1])})


BRANCHES = ("equal", "negative_dot", "near_half_pi", "near_pi")


def branch_scene(seed=3):
    """F = 4, M = 4, one actor per column; between frames 1 and 2 actor k takes branch BRANCHES[k] of the slerp:
    equal rotations (W = 0), q0 . q1 < 0, W near pi / 2 (a turn of pi - 0.1), and a raw angle near pi (q1 close to
    -q0)."""
    rng = np.random.RandomState(seed)
    F, M = 4, 4
    stamps = BASE + 0.1 * np.arange(F)
    tr = _empty(F, M)
    for a in range(M):
        for f in range(F):
            trans, q = _rand_pose(rng, a, f)
            tr[f, a] = np.concatenate([[a + 1], trans, q])
    q = tr[1, :, 4:8].copy()
    tr[2, 0, 4:8] = q[0]
    tr[2, 1, 4:8] = -_qmul_np(q[1], yaw_quat(0.3))
    tr[2, 2, 4:8] = _qmul_np(q[2], yaw_quat(np.pi - 0.1))
    tr[2, 3, 4:8] = -_qmul_np(q[3], yaw_quat(0.05))
    info = {a + 1: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1]) for a in range(M)}
    return Case(tr, stamps, info)


def opt_arrays(case, seed=0, zero_cells=()):
    """opt_trans [F,M,3] / opt_rots [F,M,1] float32; ``zero_cells``: (frame, column) cells left at zero"""
    rng = np.random.RandomState(500 + seed)
    F, M, _ = case.shape
    ot = rng.normal(0, 0.05, (F, M, 3)).astype(np.float32)
    orr = rng.normal(0, 0.1, (F, M, 1)).astype(np.float32)
    for f, c in zero_cells:
        ot[f, c] = 0
        orr[f, c] = 0
    return ot, orr


def ego_pose(candidate, seed=0):
    """float32 [4,4] whose rotation makes matrix_to_quaternion take ``candidate`` (0: near the identity, 1 / 2 / 3: a
    turn of almost pi about x / y / z), each with a small extra rotation."""
    rng = np.random.RandomState(900 + 10 * candidate + seed)
    axis = np.zeros(3)
    if candidate == 0:
        q = np.concatenate([[1.0], rng.normal(0, 0.1, 3)])
    else:
        axis[candidate - 1] = 1.0
        q = np.concatenate([[np.cos(1.5)], np.sin(1.5) * axis]) + rng.normal(0, 0.03, 4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    e = np.eye(4)
    e[:3, :3] = R
    e[:3, 3] = rng.normal(0, 50.0, 3)
    e = e.astype(np.float32)
    assert int(np.argmax([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                          1 - R[0, 0] - R[1, 1] + R[2, 2]])) == candidate
    return e


BUILDERS = dict(small_scene=small_scene, long_track=long_track, tie_scene=tie_scene, same_side_scene=same_side_scene,
                branch_scene=branch_scene)


def build_case(builder, args):
    return BUILDERS[builder](**args)


# ---- actor_pose.py:83-179 and street_gaussian_model.py:268-274, restated ----

class Truth:
    """``ActorPose`` over a Case in ``dtype``.  ``opt_trans`` / ``opt_rots``: float32 arrays or None (opt_track off);
    they become leaves of ``dtype`` that require grad.  ``variant``: one planted error of VARIANTS, or None."""

    def __init__(self, case, opt_trans=None, opt_rots=None, dtype=torch.float32, variant=None):
        assert variant is None or variant in VARIANTS
        self.case, self.dtype, self.variant = case, dtype, variant
        t = torch.from_numpy(case.tracklets).float().to(dtype)
        self.input_trans, self.input_rots = t[..., 1:4], t[..., 4:8]
        self.timestamps = case.stamps.astype(np.float32).astype(np.float64) if variant == "stamps32" else case.stamps
        self.opt_track = opt_trans is not None
        if self.opt_track:
            self.opt_trans = torch.from_numpy(np.asarray(opt_trans, np.float32)).to(dtype).requires_grad_(True)
            self.opt_rots = torch.from_numpy(np.asarray(opt_rots, np.float32)).to(dtype).requires_grad_(True)

    def find_closest_indices(self, a, timestamp):
        track_idx = self.case.track_idx[a]
        frame_timestamps = np.array(self.timestamps[track_idx[:, 0]])
        assert len(frame_timestamps) > 1
        delta = np.abs(frame_timestamps - timestamp)
        idx1, idx2 = np.argsort(delta, kind="stable")[:2]      # ties to the lower list position
        if self.variant == "swap":
            idx1, idx2 = idx2, idx1
        if self.variant == "bracket":
            order = np.argsort(frame_timestamps, kind="stable")
            after = int(np.searchsorted(frame_timestamps[order], timestamp, side="right"))
            after = min(max(after, 1), len(order) - 1)
            idx1, idx2 = order[after - 1], order[after]
            if delta[idx2] < delta[idx1]:
                idx1, idx2 = idx2, idx1
        return (idx1, idx2), track_idx[idx1], track_idx[idx2]

    def translation_(self, a, timestamp):
        pos, ind1, ind2 = self.find_closest_indices(a, timestamp)
        timestamp1, timestamp2 = self.timestamps[ind1[0]], self.timestamps[ind2[0]]
        trans1, trans2 = self.input_trans[ind1[0], ind1[1]], self.input_trans[ind2[0], ind2[1]]
        if self.opt_track:
            trans1 = trans1 + self.opt_trans[ind1[0], ind1[1]]
            trans2 = trans2 + self.opt_trans[ind2[0], ind2[1]]
        if self.variant == "weights_swapped":
            return (trans1 * (timestamp - timestamp1) + trans2 * (timestamp2 - timestamp)) / (timestamp2 - timestamp1), pos
        return (trans1 * (timestamp2 - timestamp) + trans2 * (timestamp - timestamp1)) / (timestamp2 - timestamp1), pos

    def _slerp(self, q0, q1, r):
        return quaternion_slerp(q0, q1, r, self.dtype, normalize=self.variant != "no_normalize",
                                shortest_arc=self.variant != "no_sign")

    def rotation_(self, a, timestamp):
        pos, ind1, ind2 = self.find_closest_indices(a, timestamp)
        timestamp1, timestamp2 = self.timestamps[ind1[0]], self.timestamps[ind2[0]]
        rots1, rots2 = self.input_rots[ind1[0], ind1[1]], self.input_rots[ind2[0], ind2[1]]
        if self.opt_track:
            k = 0.5 if self.variant == "half_angle" else 1.0
            opt_rots1, opt_rots2 = torch.zeros_like(rots1), torch.zeros_like(rots2)
            opt_rots1[0] = torch.cos(k * self.opt_rots[ind1[0], ind1[1]])
            opt_rots1[3] = torch.sin(k * self.opt_rots[ind1[0], ind1[1]])
            opt_rots2[0] = torch.cos(k * self.opt_rots[ind2[0], ind2[1]])
            opt_rots2[3] = torch.sin(k * self.opt_rots[ind2[0], ind2[1]])
            rots1 = quaternion_raw_multiply(rots1.unsqueeze(0), opt_rots1.unsqueeze(0)).squeeze(0)
            rots2 = quaternion_raw_multiply(rots2.unsqueeze(0), opt_rots2.unsqueeze(0)).squeeze(0)
        r = (timestamp - timestamp1) / (timestamp2 - timestamp1)
        return self._slerp(rots1, rots2, r), pos

    def camera_stamps(self, a, timestamp, cam):
        """find_closest_camera_timestamps (actor_pose.py:93-105)"""
        camera_timestamps = self.case.camera_timestamps[cam]['train_timestamps']
        info = self.case.obj_info[self.case.ids[a]]
        start, end = info['start_timestamp'], info['end_timestamp']
        camera_timestamps = np.array([x for x in camera_timestamps if x >= start and x <= end])
        if len(camera_timestamps) < 2:
            return None, None
        idx1, idx2 = np.argsort(np.abs(camera_timestamps - timestamp))[:2]
        return camera_timestamps[idx1], camera_timestamps[idx2]

    def tracking(self, a, timestamp, is_val=False, cam=None):
        """(get_tracking_rotation, get_tracking_translation, chosen)"""
        chosen = [-1, -1, -1, -1]
        if self.opt_track and is_val:
            timestamp1, timestamp2 = self.camera_stamps(a, timestamp, cam)
            if timestamp1 is not None:
                trans1, p1 = self.translation_(a, timestamp1)
                trans2, p2 = self.translation_(a, timestamp2)
                trans = (trans1 * (timestamp2 - timestamp) + trans2 * (timestamp - timestamp1)) / (timestamp2 - timestamp1)
                rots1, _ = self.rotation_(a, timestamp1)
                rots2, _ = self.rotation_(a, timestamp2)
                r = (timestamp - timestamp1) / (timestamp2 - timestamp1)
                return self._slerp(rots1, rots2, r), trans, [int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])]
        trans, p = self.translation_(a, timestamp)
        rot, _ = self.rotation_(a, timestamp)
        chosen[:2] = int(p[0]), int(p[1])
        return rot, trans, chosen

    def world(self, a, timestamp, ego, is_val=False, cam=None):
        """street_gaussian_model.py:268-274: (obj_rot [4], obj_trans [3], chosen)"""
        obj_rot, obj_trans, chosen = self.tracking(a, timestamp, is_val, cam)
        ego_pose = torch.as_tensor(ego).to(self.dtype)
        ego_pose_rot = matrix_to_quaternion(ego_pose[:3, :3].unsqueeze(0)).squeeze(0)
        if self.variant == "ego_right":
            obj_rot = quaternion_raw_multiply(obj_rot.unsqueeze(0), ego_pose_rot.unsqueeze(0)).squeeze(0)
        else:
            obj_rot = quaternion_raw_multiply(ego_pose_rot.unsqueeze(0), obj_rot.unsqueeze(0)).squeeze(0)
        obj_trans = ego_pose[:3, :3] @ obj_trans + ego_pose[:3, 3]
        return obj_rot, obj_trans, chosen

    def batch(self, timestamps, egos, is_val=False, cam=None):
        """every actor at every stamp, like ``TrackedActorPoses.poses``: dict(rot [T,A,4], trans [T,A,3] -- tensors
        with their graph --, active [T,A] uint8, chosen [T,A,4] int32)"""
        A = len(self.case.ids)
        rots, trans, active, chosen = [], [], [], []
        for t, ego in zip(timestamps, egos):
            for a, i in enumerate(self.case.ids):
                info = self.case.obj_info[i]
                on = info['start_timestamp'] <= t <= info['end_timestamp']
                active.append(1 if on else 0)
                if on:
                    r, x, c = self.world(a, t, ego, is_val, cam)
                else:
                    r = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=self.dtype)
                    x, c = torch.zeros(3, dtype=self.dtype), [-1] * 4
                rots.append(r)
                trans.append(x)
                chosen.append(c)
        T = len(timestamps)
        return dict(rot=torch.stack(rots).reshape(T, A, 4), trans=torch.stack(trans).reshape(T, A, 3),
                    active=np.array(active, np.uint8).reshape(T, A), chosen=np.array(chosen, np.int32).reshape(T, A, 4))

    def gradients(self, out, g_rot, g_trans):
        """autograd through the restatement: dense (g_opt_trans [F,M,3], g_opt_rots [F,M,1]) as numpy"""
        loss = (out["rot"] * torch.from_numpy(g_rot).to(self.dtype)).sum() + \
               (out["trans"] * torch.from_numpy(g_trans).to(self.dtype)).sum()
        g = torch.autograd.grad(loss, [self.opt_trans, self.opt_rots], allow_unused=True)
        return [np.zeros(tuple(p.shape)) if x is None else x.numpy() for x, p in zip(g, (self.opt_trans, self.opt_rots))]


def same_branches(case, timestamps, opt_trans, opt_rots, is_val=False, cam=None):
    """The value tests' precondition, asserted in float32 and float64 alike: every slerp a query makes has
    |q0 . q1| > 1e-3 (the shortest-arc sign is the same in both) and its angle W is not within 1e-3 of the small-angle
    switch (the same coefficients in both).  Returns the number of slerps looked at."""
    seen = []
    for dtype in (torch.float32, torch.float64):
        th = Truth(case, opt_trans, opt_rots, dtype)
        dots = []
        orig = th._slerp

        def spy(q0, q1, r, dots=dots, orig=orig):
            d = float((torch.nn.functional.normalize(q0.detach(), dim=-1) *
                       torch.nn.functional.normalize(q1.detach(), dim=-1)).sum())
            dots.append(d)
            return orig(q0, q1, r)
        th._slerp = spy
        eye = np.eye(4, dtype=np.float32)
        th.batch(timestamps, [eye] * len(timestamps), is_val, cam)
        seen.append(dots)
    switch = float(np.arccos(SMALL_C))
    assert len(seen[0]) == len(seen[1])
    for d32, d64 in zip(*seen):
        assert abs(d32) > 1e-3 and abs(d64) > 1e-3 and (d32 < 0) == (d64 < 0), (d32, d64)
        for d in (d32, d64):
            w = float(np.arccos(min(abs(d), 1.0)))
            assert abs(w - switch) > 1e-3, "a slerp within 1e-3 of the small-angle switch (W = %g)" % w
        assert (min(abs(d32), 1.0) > SMALL_C) == (min(abs(d64), 1.0) > SMALL_C)
    return len(seen[0])


# ---- the comparator ----

def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(-1, x.shape[-1])


def group_errors(got, f32, f64):
    """One group of rows (rot, trans, g_opt_trans, g_opt_rots) against the float64 truth: the candidate's and the
    float32 restatement's relative L2 over the group and worst row, the ratios of the two, and the bounds: MARGIN x
    the restatement's figure (its group figure; its worst row), or FLOOR_ULPS float32 ulps of the group's norm / of the
    row's own norm where that is more (the restatement happens to be exact).  A row whose truth is zero has no floor."""
    got, f32, f64 = _rows(got), _rows(f32), _rows(f64)
    assert got.shape == f32.shape == f64.shape, (got.shape, f32.shape, f64.shape)
    norm = max(float(np.linalg.norm(f64)), 1e-300)
    rel_got, rel_32 = float(np.linalg.norm(got - f64)) / norm, float(np.linalg.norm(f32 - f64)) / norm
    row_got, row_32 = np.linalg.norm(got - f64, axis=1), np.linalg.norm(f32 - f64, axis=1)
    floor = FLOOR_ULPS * EPS32 * np.linalg.norm(f64, axis=1)
    bound_rows = np.maximum(MARGIN * row_32.max(initial=0.0), floor)
    bound_l2 = max(MARGIN * rel_32, FLOOR_ULPS * EPS32)
    worst = int(np.argmax(row_got - bound_rows)) if len(row_got) else 0
    return dict(rel_l2=rel_got, rel_l2_restatement=rel_32, rel_l2_bound=bound_l2,
                rel_l2_ratio=rel_got / rel_32 if rel_32 > 0 else None,
                worst_row=float(row_got.max(initial=0.0)), worst_row_restatement=float(row_32.max(initial=0.0)),
                worst_row_ratio=float(row_got.max(initial=0.0)) / float(row_32.max()) if row_32.max(initial=0.0) > 0 else None,
                worst_row_excess=float((row_got - bound_rows).max(initial=-1.0)), worst_row_index=worst,
                ok=bool(np.all(np.isfinite(got)) and rel_got <= bound_l2 and np.all(row_got <= bound_rows)))


def compare(got, f32, f64, groups=("rot", "trans"), report=None, name=""):
    """``got`` (the candidate: dict of arrays), ``f32`` / ``f64`` (Truth.batch results or dicts of arrays): ``chosen``
    and ``active`` must equal the truth's exactly, every group must pass group_errors.  Raises AssertionError naming
    what failed; returns {group: figures}.  ``report``: a dict the figures are also filed in under ``name``."""
    as_np = lambda v: v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)   # noqa: E731
    figures = {}
    for key in ("chosen", "active"):
        if key in f64:
            assert np.array_equal(as_np(got[key]), as_np(f64[key])), "%s: %s differs from the truth's" % (name, key)
    for g in groups:
        figures[g] = group_errors(as_np(got[g]), as_np(f32[g]), as_np(f64[g]))
    if report is not None:
        report[name] = figures
    for g, f in figures.items():
        assert f["ok"], "%s / %s: beyond %gx the float32 restatement's own distance from the truth: %r" % (name, g, MARGIN, f)
    return figures
