"""Tracklets -> actor poses on the device: the step in front of ``ComposedRasterizer``.

``StreetGaussianModel.parse_camera`` (lib/models/street_gaussian_model.py:263-283) asks
``ActorPose.get_tracking_rotation`` / ``get_tracking_translation`` (lib/models/actor_pose.py:83-179) for one pose per
visible actor, every iteration and every frame: two ``argsort`` lookups with a ``.cpu()`` each, four gathers, a
quaternion product, a slerp, ``matrix_to_quaternion`` of the ego pose and two more products -- several dozen small
launches and four host waits per actor.  Here the same arithmetic is ONE launch for every actor and every query stamp
(C ABI ``grpg_track_poses_forward``, csrc/tracks.hip) and, in training, ONE memset and ONE launch back to
``opt_trans`` / ``opt_rots`` (``grpg_track_poses_backward``), with no host wait of its own.

    table  = TrackTable.from_tracklets(tracklets, tracklet_timestamps, obj_info)      # once per scene
    actors = TrackedActorPoses(table, camera_timestamps=camera_timestamps)             # opt_trans / opt_rots
    batch  = actors.poses(camera.meta['timestamp'], camera.ego_pose, is_val=..., cam=...)
    rows   = batch.rows(0, visible_actor_indices, fourier_times)                       # -> composed.PoseTable
    color, radii, depth, alpha = ComposedRasterizer(settings)(models, rows)

``batch.rows`` leaves the poses on the device: the library's segment table takes them from there, on the stream of the
rendering call (C ABI ``grpg_bind_device_poses``).  ``batch.frame`` (-> ``composed.PoseRows``) is the older hand-over
through the host -- four small launches and one device-to-host copy -- and gives the same bits.

The slerp is the geodesic on the shortest arc as DESIGN.md section 21 defines it -- what
``roma.utils.unitquat_slerp(shortest_arc=True)`` computes in real arithmetic; roma's float32 bits are not pinned.
There is no CPU path and no fallback.
"""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from .composed import PoseRows, PoseTable
from .rasterizer import _C


def closest_camera_timestamps(camera_timestamps, start: float, end: float, t: float):
    """``ActorPose.find_closest_camera_timestamps`` (actor_pose.py:93-105) in numpy on the host: the two training
    camera stamps inside [start, end] closest to ``t`` (closest first), or ``(None, None)`` when fewer than two lie
    inside.  It waits for nothing."""
    ts = np.asarray(camera_timestamps, dtype=np.float64).reshape(-1)
    ts = ts[(ts >= start) & (ts <= end)]
    if len(ts) < 2:
        return None, None
    i1, i2 = np.argsort(np.abs(ts - t))[:2]
    return ts[i1], ts[i2]


class TrackTable:
    """The static side of ``ActorPose`` (actor_pose.py:9-30), built once per scene: the tracklet stamps (float64: Waymo
    stamps are about 1.5e9 s, 0.1 s apart, and float32 cannot tell neighbours apart), ``input_trans`` / ``input_rots``,
    and per actor -- the keys of ``obj_info`` in their order -- the entry list ``argwhere(track_ids == track_id)`` as
    ``entries [E,2]`` + ``entry_offsets [A+1]``, and ``start`` / ``end``.  The host arrays are kept (the visible list
    and the validation stamps are host arithmetic); ``tensors(device)`` is the device copy the kernels read."""

    def __init__(self, stamps, input_trans, input_rots, entries, entry_offsets, start, end, track_ids):
        self.stamps = np.ascontiguousarray(stamps, dtype=np.float64)
        self.input_trans = np.ascontiguousarray(input_trans, dtype=np.float32)
        self.input_rots = np.ascontiguousarray(input_rots, dtype=np.float32)
        self.entries = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1, 2)
        self.entry_offsets = np.ascontiguousarray(entry_offsets, dtype=np.int32)
        self.start = np.ascontiguousarray(start, dtype=np.float64)
        self.end = np.ascontiguousarray(end, dtype=np.float64)
        self.track_ids = list(track_ids)
        F, M = self.input_trans.shape[:2]
        A = len(self.track_ids)
        if self.stamps.shape != (F,) or self.input_trans.shape != (F, M, 3) or self.input_rots.shape != (F, M, 4):
            raise ValueError("stamps [F], input_trans [F,M,3] and input_rots [F,M,4] must agree")
        if A < 1:
            raise ValueError("a track table needs at least one actor")
        if self.entry_offsets.shape != (A + 1,) or self.start.shape != (A,) or self.end.shape != (A,):
            raise ValueError("entry_offsets [A+1], start [A] and end [A] must agree with the %d actors" % A)
        if not np.all(np.isfinite(self.stamps)):
            raise ValueError("tracklet timestamps must be finite")
        if self.entry_offsets[0] != 0 or self.entry_offsets[-1] != len(self.entries):
            raise ValueError("entry_offsets must run from 0 to the number of entries")
        lengths = np.diff(self.entry_offsets)
        if np.any(lengths < 2):
            a = int(np.argmax(lengths < 2))
            raise ValueError("track %r has %d entries; an actor needs at least two (actor_pose.py:87)"
                             % (self.track_ids[a], int(lengths[a])))
        e = self.entries
        if len(e) and (e[:, 0].min() < 0 or e[:, 0].max() >= F or e[:, 1].min() < 0 or e[:, 1].max() >= M):
            raise ValueError("an entry lies outside the [F,M] table")
        self._dev = {}

    @property
    def shape(self):
        """(F, M, A)"""
        return self.input_trans.shape[0], self.input_trans.shape[1], len(self.track_ids)

    @classmethod
    def from_tracklets(cls, tracklets, tracklet_timestamps, obj_info):
        """tracklets ``[F,M,8]`` (track_id, x, y, z, qw, qx, qy, qz), tracklet_timestamps ``[F]``, obj_info
        ``{track_id: {'start_timestamp', 'end_timestamp', ...}}``.  The ids are compared as the reference compares
        them: after ``.float()``.  Padded cells (id -1) and ids that ``obj_info`` does not list belong to no actor."""
        tr = np.asarray(tracklets)
        if tr.ndim != 3 or tr.shape[2] != 8:
            raise ValueError("tracklets must be [F,M,8], got %s" % (tr.shape,))
        tr32 = tr.astype(np.float32)
        ids = tr32[..., 0]
        entries, offsets, start, end = [], [0], [], []
        for track_id, info in obj_info.items():
            at = np.argwhere(ids == np.float32(track_id))          # row-major, like torch.argwhere
            entries.append(at.astype(np.int32))
            offsets.append(offsets[-1] + len(at))
            start.append(float(info['start_timestamp']))
            end.append(float(info['end_timestamp']))
        cat = np.concatenate(entries, 0) if entries else np.zeros((0, 2), np.int32)
        return cls(np.asarray(tracklet_timestamps, dtype=np.float64).reshape(-1), tr32[..., 1:4], tr32[..., 4:8], cat,
                   offsets, start, end, obj_info.keys())

    def entry_list(self, a: int) -> np.ndarray:
        """The ``[L,2]`` (frame, column) list of actor ``a``."""
        return self.entries[self.entry_offsets[a]:self.entry_offsets[a + 1]]

    def tensors(self, device):
        """The table as ``_C.track_poses_forward`` takes it, resident on ``device`` (copied once)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("gaussianrpg_amd: the track table must live on a ROCm/HIP device (torch device 'cuda'): "
                               "there is no CPU path")
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        t = self._dev.get(key)
        if t is None:
            dev = [torch.from_numpy(x).to(device) for x in (self.stamps, self.input_trans, self.input_rots, self.entries,
                                                            self.entry_offsets, self.start, self.end)]
            t = self._dev[key] = dev + [torch.from_numpy(self.entry_offsets)]
        return t


class PoseBatch(NamedTuple):
    """World poses of every actor of a ``TrackTable`` at ``T`` query stamps, ego pose applied: ``rot [T,A,4]`` (w,x,y,z),
    ``trans [T,A,3]``, ``active [T,A]`` uint8 (``start <= t <= end``; an inactive row is (1,0,0,0) / (0,0,0) and never
    receives a gradient).  ``chosen [T,A,4]`` int32: the list positions the lookup used, -1 where unused."""
    rot: torch.Tensor
    trans: torch.Tensor
    active: torch.Tensor
    chosen: Optional[torch.Tensor] = None

    def frame(self, t: int, actors: Sequence[int], fourier_time: Optional[Sequence[float]] = None, static: int = 1):
        """The poses of one frame as the row set ``ComposedRasterizer`` takes: ``static`` leading static models
        (the background), then the actors ``actors`` (indices into the table's actor list, the frame's visible list)
        with their ``fourier_time``.  Four small launches (a pad and a gather for each of the two tensors) whatever the
        number of actors; the rows keep their graph."""
        n = len(actors)
        times = [0.0] * n if fourier_time is None else [float(x) for x in fourier_time]
        if len(times) != n:
            raise ValueError("one fourier_time per actor (%d for %d actors)" % (len(times), n))
        dev = self.rot.device
        # row 0 of the padded arrays is the constant of a static model; the actors' rows follow
        index = torch.tensor([0] * static + [int(a) + 1 for a in actors], dtype=torch.long).to(dev, non_blocking=True)
        rot = torch.nn.functional.pad(self.rot[t], (0, 0, 1, 0)).index_select(0, index)
        trans = torch.nn.functional.pad(self.trans[t], (0, 0, 1, 0)).index_select(0, index)
        return PoseRows(rot, trans, [False] * static + [True] * n, [0.0] * static + times)

    def rows(self, t: int, actors: Sequence[int], fourier_time: Optional[Sequence[float]] = None, static: int = 1):
        """``frame`` without its launches and without the host copy behind it: the same frame as a
        ``composed.PoseTable`` -- the batch's own ``rot[t]`` / ``trans[t]`` (views; they keep their graph) and, per
        model, the row it reads: -1 for the ``static`` leading models, the actor's index for the others.  No launch,
        no copy; the library takes the rows from device memory on the stream of the call that renders the frame."""
        n = len(actors)
        times = [0.0] * n if fourier_time is None else [float(x) for x in fourier_time]
        if len(times) != n:
            raise ValueError("one fourier_time per actor (%d for %d actors)" % (len(times), n))
        A = int(self.rot.shape[1])
        index = [int(a) for a in actors]
        for a in index:
            if a < 0 or a >= A:
                raise IndexError("actor %d is not one of the batch's %d actors" % (a, A))
        return PoseTable(self.rot[t], self.trans[t], [-1] * static + index, [False] * static + [True] * n,
                         [0.0] * static + times)


class _TrackPoses(torch.autograd.Function):
    """forward = _C.track_poses_forward, backward = _C.track_poses_backward (C ABI grpg_track_poses_*)."""

    @staticmethod
    def forward(ctx, table, timestamps, ego, val_stamps, opt_trans, opt_rots):
        rot, trans, active, chosen = _C.track_poses_forward(table, timestamps, ego, opt_trans, opt_rots, val_stamps)
        ctx.table, ctx.val_stamps = table, val_stamps
        ctx.save_for_backward(timestamps, ego, opt_trans, opt_rots)
        ctx.mark_non_differentiable(active, chosen)
        return rot, trans, active, chosen

    @staticmethod
    def backward(ctx, g_rot, g_trans, g_active, g_chosen):
        timestamps, ego, opt_trans, opt_rots = ctx.saved_tensors
        T, A = timestamps.shape[0], ctx.table[4].shape[0] - 1
        g_rot = ego.new_zeros(T, A, 4) if g_rot is None else g_rot.contiguous()
        g_trans = ego.new_zeros(T, A, 3) if g_trans is None else g_trans.contiguous()
        g_ot, g_or = _C.track_poses_backward(ctx.table, timestamps, ego, opt_trans, opt_rots, ctx.val_stamps, g_rot,
                                             g_trans)
        return None, None, None, None, g_ot, g_or


class TrackedActorPoses(torch.nn.Module):
    """``ActorPose`` (actor_pose.py) over a ``TrackTable``: the parameters ``opt_trans [F,M,3]`` and ``opt_rots
    [F,M,1]`` carry the reference's names, shapes and zero initialisation, so ``state_dict()`` loads from and into the
    reference's ``actor_pose`` -> ``params`` entry.  ``opt_track=False`` has no parameters (``cfg.model.nsg.opt_track``).
    ``camera_timestamps``: ``{cam: {'train_timestamps': [...]}}`` as the reference keeps it, for validation frames."""

    def __init__(self, table: TrackTable, opt_track: bool = True, camera_timestamps=None, device="cuda"):
        super().__init__()
        self.table = table
        self.opt_track = bool(opt_track)
        self.camera_timestamps = camera_timestamps
        F, M, _ = table.shape
        if self.opt_track:
            self.opt_trans = torch.nn.Parameter(torch.zeros(F, M, 3, device=device))
            self.opt_rots = torch.nn.Parameter(torch.zeros(F, M, 1, device=device))

    def val_stamps(self, timestamps: Sequence[float], is_val, cam) -> Optional[np.ndarray]:
        """float64 ``[T,A,2]`` on the host: per (query, actor) the two camera stamps of a validation frame
        (actor_pose.py:124-131), NaN where the plain path applies; None when no query is a validation frame."""
        T, A = len(timestamps), self.table.shape[2]
        flags = [bool(is_val)] * T if isinstance(is_val, (bool, np.bool_)) else [bool(v) for v in is_val]
        if len(flags) != T:
            raise ValueError("one is_val flag per timestamp")
        if not (self.opt_track and any(flags)):
            return None
        if self.camera_timestamps is None or cam is None:
            raise ValueError("a validation frame needs camera_timestamps and cam")
        cams = [cam] * T if isinstance(cam, (int, str)) else list(cam)
        out = np.full((T, A, 2), np.nan, dtype=np.float64)
        for i, (t, v) in enumerate(zip(timestamps, flags)):
            if not v:
                continue
            train = self.camera_timestamps[cams[i]]['train_timestamps']
            for a in range(A):
                c1, c2 = closest_camera_timestamps(train, self.table.start[a], self.table.end[a], t)
                if c1 is not None:
                    out[i, a] = (c1, c2)
        return out

    def poses(self, timestamps, ego_pose: torch.Tensor, is_val=False, cam=None) -> PoseBatch:
        """Every actor's world pose at ``timestamps`` (a float or ``T`` floats on the host, or a float64 ``[T]`` device
        tensor) under ``ego_pose`` (float32 ``[4,4]`` or ``[T,4,4]`` on the device).  One launch; with gradients enabled
        and ``opt_track`` the result carries the graph to ``opt_trans`` / ``opt_rots``."""
        if not isinstance(ego_pose, torch.Tensor):
            raise TypeError("ego_pose must be a tensor")
        if ego_pose.dtype != torch.float32:
            raise TypeError("ego_pose must be float32, got %s" % ego_pose.dtype)
        if ego_pose.shape[-2:] != (4, 4) or ego_pose.dim() not in (2, 3):
            raise ValueError("ego_pose must be [4,4] or [T,4,4], got %s" % (tuple(ego_pose.shape),))
        if not ego_pose.is_cuda:
            raise RuntimeError("gaussianrpg_amd: ego_pose must live on a ROCm/HIP device (torch device 'cuda'): there "
                               "is no CPU path")
        dev = ego_pose.device
        if isinstance(timestamps, torch.Tensor):
            if timestamps.dtype != torch.float64:
                raise TypeError("timestamps must be float64 (float32 cannot tell neighbouring stamps apart), got %s"
                                % timestamps.dtype)
            if not timestamps.is_cuda:
                raise RuntimeError("gaussianrpg_amd: a timestamp tensor must live on the device; pass host stamps as floats")
            if is_val is not False:
                raise ValueError("validation frames take their timestamps from the host (floats)")
            ts, val = timestamps.reshape(-1).contiguous(), None
        else:
            host = np.atleast_1d(np.asarray(timestamps, dtype=np.float64)).reshape(-1)
            val = self.val_stamps(host.tolist(), is_val, cam)
            ts = torch.from_numpy(host).to(dev, non_blocking=True)
            if val is not None:
                val = torch.from_numpy(val).to(dev, non_blocking=True)
        T = ts.shape[0]
        ego = ego_pose.detach()
        ego = (ego.expand(T, 4, 4) if ego.dim() == 2 else ego).contiguous()
        if ego.shape[0] != T:
            raise ValueError("%d ego poses for %d timestamps" % (ego.shape[0], T))
        table = self.table.tensors(dev)
        if not self.opt_track:
            with torch.no_grad():
                return PoseBatch(*_C.track_poses_forward(table, ts, ego, None, None, None))
        if torch.is_grad_enabled() and (self.opt_trans.requires_grad or self.opt_rots.requires_grad):
            return PoseBatch(*_TrackPoses.apply(table, ts, ego, val, self.opt_trans, self.opt_rots))
        with torch.no_grad():
            return PoseBatch(*_C.track_poses_forward(table, ts, ego, self.opt_trans, self.opt_rots, val))
