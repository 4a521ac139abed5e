"""Closed-loop evaluation session: bind a pose tape once, one call per frame.

The simulator node is started with a pose tape (``cams_tape.json``: render_lite.py:39-87 writes it,
simulator.py:215-307 replays it).  Everything a frame needs except the camera's own ``R``, ``T`` is fixed by the tape
entry: which actors are visible (street_gaussian_model.py:239-262), their tracked world poses under the entry's
``ego_pose`` (:263-283; simulator.py:297-299), each actor's Fourier time (gaussian_model_actor.py:73-75, frame = tape
index, simulator.py:301-303) and, with ``use_mlp`` colour correction, the frame's 3 x 4 matrix.  ``FrameSession``
computes all of it ONCE -- one ``TrackedActorPoses.poses`` launch over the T stamps, the IDFT rows on the host, the
device segment tables of all T frames in one upload and one launch (C ABI ``grpg_frame_tables_bake``,
csrc/frame_table.hip), the tape's own cameras as device rows -- and ``session.frame(k)`` then renders frame ``k`` with
nothing in front of the frame's first launch: no pose launch, no packing, no table upload, no pose gather, and for the
tape's own camera no host-to-device copy at all (C ABI ``grpg_bind_frame_table``).  The bytes are those of the
per-frame route, ``harness.closed_loop_frame(bound=False)``, bit for bit.

``TapePlan`` is the host half -- visible lists, index ranges, Fourier times, IDFT rows, the row lists of the bake --
and needs no device.
"""
import operator
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import harness as hz
from .composed import MAX_FOURIER, ModelParams, _NO_FLIP, _check_models, _idft_rows, _model_lists
from .rasterizer import GaussianRasterizationSettings, _C, _frame_result, _or_empty, _white
from .trajectory import camera_from_tape

CAMERA_ROW = 48     # floats per camera row: view 16, proj 16, campos 3 (+1 spare), ray matrix 9 (+3 spare)
_VIEW, _PROJ, _POS, _RAY = slice(0, 16), slice(16, 32), slice(32, 35), slice(36, 45)


def fourier_time(frame, span) -> float:
    """``get_features_fourier``'s time (gaussian_model_actor.py:74-75) in Python floats: ``fourier_scale * ((frame -
    start_frame) / (end_frame - start_frame))``.  A span of one frame (the reference divides by zero there) gives 0.0;
    ``TapePlan`` accepts it for Fourier dimension 1 only, whose single IDFT weight is cos(0) whatever the time."""
    start, end, scale = span
    if end == start:
        return 0.0
    return float(scale) * ((frame - start) / (end - start))


class TapePlan:
    """The host plan of a tape: per entry the visible actors (``start <= timestamp <= end``, both ends inclusive, and
    ``visibility[a]`` when given; the table's actor order, as ``parse_camera`` lists them), ``graph_gaussian_range``,
    the model and Gaussian counts, the Fourier times and the IDFT rows (``composed._idft_rows``: the float32 bits
    pinned to the reference), and the flat row lists ``grpg_frame_tables_bake`` takes.  Device-free.

    ``start`` / ``end``: the actors' first and last stamps (``TrackTable.start`` / ``.end``); ``counts`` / ``dims``:
    Gaussians and Fourier dimension per actor; ``static_counts``: Gaussians of the static models in front of the
    actors (the background).  ``spans[a] = (start_frame, end_frame, fourier_scale)``."""

    def __init__(self, start, end, counts, dims, tape, spans, visibility=None, static_counts=(0,)):
        A = len(counts)
        if not (len(start) == len(end) == len(dims) == len(spans) == A):
            raise ValueError("one start, end, count, Fourier dimension and span per actor")
        if visibility is not None and len(visibility) != A:
            raise ValueError("visibility: one flag per actor (%d flags, %d actors)" % (len(visibility), A))
        if len(tape) == 0:
            raise ValueError("the tape is empty")
        self.num_actors = A
        self.counts = [int(c) for c in counts]
        self.dims = [int(d) for d in dims]
        self.static_counts = [int(c) for c in static_counts]
        self.spans = [(s[0], s[1], float(s[2])) for s in spans]
        for a, (s, e, _) in enumerate(self.spans):
            if e == s and self.dims[a] > 1:
                raise ValueError("actor %d: end_frame == start_frame with fourier_dim %d: the Fourier time divides by "
                                 "zero (gaussian_model_actor.py:74)" % (a, self.dims[a]))
        n_static, nb = len(self.static_counts), sum(self.static_counts)
        self.stamps = [float(e["timestamp"]) for e in tape]
        self.frames = [e.get("frame", e["id"]) for e in tape]
        self._visible, self._ranges, self._times, self._num = [], [], [], []
        self.frame_first, self.row_model, self.row_pose, idft = [0], [], [], []
        for k, ts in enumerate(self.stamps):
            vis = [a for a in range(A) if start[a] <= ts <= end[a] and (visibility is None or visibility[a])]
            ranges, idx = {}, 0
            if nb:
                ranges["background"] = [0, nb - 1]
                idx = nb
            for a in vis:
                ranges[a] = [idx, idx + self.counts[a] - 1]
                idx += self.counts[a]
            times = [fourier_time(self.frames[k], self.spans[a]) for a in vis]
            self._visible.append(vis)
            self._ranges.append(ranges)
            self._times.append(times)
            self._num.append(idx)
            self.row_model += list(range(n_static)) + [n_static + a for a in vis]
            self.row_pose += [-1] * n_static + [k * A + a for a in vis]
            idft.append(_idft_rows([0.0] * n_static + times, tuple([1] * n_static + [self.dims[a] for a in vis])))
            self.frame_first.append(len(self.row_model))
        self.idft = torch.cat(idft, 0).contiguous()      # [rows, MAX_FOURIER] float32, frame after frame

    def __len__(self):
        return len(self.stamps)

    def check(self, k) -> int:
        k = operator.index(k)
        if k < 0 or k >= len(self.stamps):
            raise IndexError("frame %d is not one of the tape's %d entries" % (k, len(self.stamps)))
        return k

    def visible(self, k) -> List[int]:
        return list(self._visible[self.check(k)])

    def ranges(self, k) -> dict:
        return {key: list(v) for key, v in self._ranges[self.check(k)].items()}

    def fourier_times(self, k) -> List[float]:
        return list(self._times[self.check(k)])

    def num_gaussians(self, k) -> int:
        return self._num[self.check(k)]

    def num_models(self, k) -> int:
        k = self.check(k)
        return self.frame_first[k + 1] - self.frame_first[k]

    def idft_rows(self, k) -> torch.Tensor:
        """[models of frame k, MAX_FOURIER]: the static models' rows first, then the visible actors'"""
        k = self.check(k)
        return self.idft[self.frame_first[k]:self.frame_first[k + 1]]


def default_K(W, H) -> np.ndarray:
    """The intrinsics ``trajectory.camera_from_tape`` renders with: the Waymo FRONT camera scaled to W."""
    s = W / hz.WAYMO_W
    return np.array([[hz.WAYMO_FX * s, 0.0, W / 2.0], [0.0, hz.WAYMO_FY * s, H / 2.0], [0.0, 0.0, 1.0]], dtype=np.float64)


def camera_from_pose(R, T, W, H, device="cpu") -> hz.CameraTensors:
    """``camera_from_tape``'s camera for a pose that is not on the tape: the closed loop's moved camera
    (simulator.py:226-242 -> Camera.__init__)."""
    return camera_from_tape(dict(rotation_matrix=R, position=T), W=W, H=H, device=device)


def _camera_row(cam: hz.CameraTensors, Kinv: Optional[np.ndarray]) -> np.ndarray:
    """One camera as CAMERA_ROW floats; the ray matrix is ``sky.ray_matrix_host``'s arithmetic (float64 ``R^T K^-1``,
    rounded once) on the camera's own world-to-camera matrix."""
    row = np.zeros(CAMERA_ROW, dtype=np.float32)
    view = cam.viewmatrix.detach().numpy()
    row[_VIEW] = view.reshape(-1)
    row[_PROJ] = cam.projmatrix.detach().numpy().reshape(-1)
    row[_POS] = cam.campos.detach().numpy().reshape(-1)
    if Kinv is not None:
        # (the world-to-camera matrix laid out as harness.world2view returns it: the same operands, the same product)
        R64 = np.asarray(np.ascontiguousarray(view.T), dtype=np.float64)[:3, :3]
        row[_RAY] = (R64.T @ Kinv).astype(np.float32).reshape(-1)
    return row


class CameraRow:
    """A camera that already lies on the device: one contiguous float32 ``[CAMERA_ROW]`` row in the layout of the
    session's own cameras (view^T 16, full projection^T 16, centre 3 + 1 spare, ray matrix 9 + 3 spare).
    ``FrameSession.frame(k, camera=row)`` hands its four views straight to the frame call: no staging, no copy, no
    event.  ``closed_loop.EgoLoop.camera`` is one; the kernel that wrote the row and the frame that reads it are
    ordered by the stream they share."""

    def __init__(self, row: torch.Tensor):
        if not (isinstance(row, torch.Tensor) and row.is_cuda and row.dtype == torch.float32
                and tuple(row.shape) == (CAMERA_ROW,) and row.is_contiguous()):
            raise ValueError("a CameraRow is a contiguous float32 [%d] device tensor" % CAMERA_ROW)
        self.row = row.detach()
        self.views = (self.row[_VIEW], self.row[_PROJ], self.row[_POS], self.row[_RAY])

    def tensors(self, H, W, tanfovx, tanfovy) -> hz.CameraTensors:
        """The row read back as CPU ``CameraTensors`` (one device-to-host copy, one host wait): for tests and logs."""
        r = self.row.cpu()
        return hz.CameraTensors(int(H), int(W), tanfovx, tanfovy, r[_VIEW].reshape(4, 4).clone(),
                                r[_PROJ].reshape(4, 4).clone(), r[_POS].clone())


class FrameSession:
    """A scene bound to a pose tape for evaluation: ``session.frame(k)`` is the closed loop's per-frame call.

    ``settings``: a ``GaussianRasterizationSettings``; the session uses its size, ``bg``, ``sh_degree``,
    ``scale_modifier`` and FoV tangents (its camera tensors are not used: the default camera of frame ``k`` is the
    tape's own).  ``background``: one ``ModelParams`` or a list of static models; ``actor_models[a]``: the model of
    actor ``a`` of ``actors.table`` (``actors``: a ``tracks.TrackedActorPoses``).  ``tape``: a list of dicts in
    ``trajectory``'s format (``id``, ``timestamp``, ``rotation_matrix``, ``position``, ``ego_pose``; an optional
    ``frame`` defaults to ``id``).  ``spans[a] = (start_frame, end_frame, fourier_scale)``.  ``visibility``: one flag
    per actor.  ``sky_cube`` / ``K`` / ``sky_fill``: the sky composite of ``forward_frame`` (``K`` defaults to the
    tape camera's intrinsics).  ``affines``: a float32 ``[T,3,4]`` device tensor from any source (``ColorCorrection``
    rows, ``ColorCorrectionMLP.affines``); frame ``k`` uses ``affines[k]`` as a view.  ``object_models`` /
    ``layer_bg``: ``forward_frame``'s, one flag per model of the SCENE (static models, then all actors).  ``ring``:
    staging slots of the moved camera.

    Lifetime: the session keeps references to the parameter tensors whose pointers it baked, to the pose batch and to
    ``affines``.  In-place changes to the parameters are seen by the next frame.  A tensor REPLACED by a new allocation
    (densification, ``load_state_dict`` into new storage, an optimizer step of ``opt_trans`` -- the poses are baked
    values) needs a new session.  Evaluation only: there is no training path and no gradient.  One session renders
    on one stream at a time (the moved camera's device slots are reused in stream order)."""

    def __init__(self, settings: GaussianRasterizationSettings, background, actor_models: Sequence[ModelParams], actors,
                 tape, spans, *, visibility=None, sky_cube=None, K=None, sky_fill=0.0, affines=None,
                 object_models=None, layer_bg=None, ring=8):
        statics = [background] if isinstance(background, ModelParams) else list(background)
        models = statics + list(actor_models)
        _check_models(models)
        table = actors.table
        A = table.shape[2]
        if len(actor_models) != A:
            raise ValueError("one model per actor of the track table (%d models, %d actors)" % (len(actor_models), A))
        lists, dims = _model_lists(models)
        self.plan = TapePlan(list(table.start), list(table.end), [m.xyz.shape[0] for m in actor_models],
                             dims[len(statics):], tape, spans, visibility, [m.xyz.shape[0] for m in statics])
        T = len(self.plan)
        self.settings, self.models, self.ring = settings, models, int(ring)
        if self.ring < 1:
            raise ValueError("ring must be at least 1")
        dev = models[0].xyz.device
        self.device = dev
        H, W = int(settings.image_height), int(settings.image_width)
        if object_models is not None and len(object_models) != len(models):
            raise ValueError("object_models: one flag per model of the scene (%d flags, %d models)"
                             % (len(object_models), len(models)))
        if affines is not None:
            if not (affines.is_cuda and affines.dtype == torch.float32 and tuple(affines.shape) == (T, 3, 4)):
                raise ValueError("affines must be a float32 [%d,3,4] device tensor" % T)
            affines = affines.detach()
            if not affines.is_contiguous():
                affines = affines.contiguous()
        self.affines = affines
        self._affine = [None] * T if affines is None else [affines[k] for k in range(T)]
        self.sky_cube, self.sky_fill = sky_cube, float(sky_fill)
        self._K = default_K(W, H) if K is None else np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K,
                                                                 dtype=np.float64)
        self._Kinv = np.linalg.inv(self._K) if sky_cube is not None else None
        self._layer_bg = layer_bg
        with torch.no_grad():
            # 2. every actor's world pose at every stamp under the entry's ego pose: one launch
            ego = torch.from_numpy(np.asarray([e["ego_pose"] for e in tape], dtype=np.float32).reshape(T, 4, 4)).to(dev)
            self.batch = actors.poses(self.plan.stamps, ego)
            pose_rot = self.batch.rot.detach().reshape(T * A, 4).contiguous()
            pose_trans = self.batch.trans.detach().reshape(T * A, 3).contiguous()
            # 4. the segment tables of all frames: one upload, one launch
            flags = torch.zeros(len(models), 8)
            flags[len(statics):, 0] = 1.0
            no_idft = torch.zeros(len(models), MAX_FOURIER)
            p = self.plan
            bake = lambda cls: _C.bake_frame_tables(*lists, flags, no_idft, p.frame_first, p.row_model, p.row_pose,  # noqa: E731
                                                    p.idft, cls, pose_rot, pose_trans)
            self._tables = bake(torch.empty(0, dtype=torch.uint8))
            # a layered frame with object_models carries their class bit; a plain frame the default one (rigid)
            self._tables_layers = self._tables if object_models is None else bake(
                torch.tensor([1 if object_models[m] else 0 for m in p.row_model], dtype=torch.uint8))
            # 5. the tape's own cameras, made on the host by the function the per-frame route uses
            rows = np.stack([_camera_row(camera_from_tape(e, W=W, H=H, device="cpu"), self._Kinv) for e in tape])
            self._cameras = torch.from_numpy(rows).to(dev)
            self._stage = torch.empty(self.ring, CAMERA_ROW).pin_memory()
            self._stage_np = self._stage.numpy()
            self._slots = torch.empty(self.ring, CAMERA_ROW, device=dev)
        self._tape_views = [self._views(self._cameras[k]) for k in range(T)]
        self._slot_views = [self._views(self._slots[i]) for i in range(self.ring)]
        self._events = [torch.cuda.Event() for _ in range(self.ring)]
        self._used = [False] * self.ring
        self._next = 0
        self._tape = tape
        self._size = (H, W)
        self.num_rendered = 0

    @staticmethod
    def _views(row):
        return row[_VIEW], row[_PROJ], row[_POS], row[_RAY]

    def __len__(self):
        return len(self.plan)

    def visible(self, k):
        return self.plan.visible(k)

    def ranges(self, k):
        return self.plan.ranges(k)

    def num_gaussians(self, k):
        return self.plan.num_gaussians(k)

    def table_rows(self, k, layers=False) -> torch.Tensor:
        """uint8 [models of frame k, 144]: the frame's baked segment rows, a view of the device table"""
        k = self.plan.check(k)
        t = self._tables_layers if layers else self._tables
        first = self.plan.frame_first
        return t.rows.view(-1, 144)[first[k]:first[k + 1]]

    def _stage_camera(self, camera, Kinv):
        """a moved camera: CAMERA_ROW floats into the next pinned slot, one asynchronous copy to its device slot, an
        event behind the copy (the slot comes round again `ring` frames later) -> the slot's views"""
        H, W = self._size
        if not isinstance(camera, hz.CameraTensors):
            R, T = camera
            camera = camera_from_pose(np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64), W, H)
        elif camera.viewmatrix.is_cuda:
            raise ValueError("a moved camera arrives on the host: pass CPU CameraTensors or an (R, T) pair")
        row = _camera_row(camera, Kinv)
        i = self._next
        self._next = (i + 1) % self.ring
        if self._used[i]:
            self._events[i].synchronize()
        self._used[i] = True
        self._stage_np[i] = row
        self._slots[i].copy_(self._stage[i], non_blocking=True)
        self._events[i].record()
        return self._slot_views[i]

    def frame(self, k, camera=None, *, K=None, out=None, planes=False, layers=False, rgb8=True, truncate=True,
              clamp=True) -> dict:
        """Frame ``k`` of the tape -> the dict of ``ComposedRasterizer.forward_frame``.  ``camera=None``: the tape's
        own pose -- no host-to-device copy at all.  ``camera``: CPU ``CameraTensors`` or an ``(R, T)`` pair (the closed
        loop's moved camera); its 35 floats and the ray matrix reach the device in ONE asynchronous copy from a pinned
        ring slot.  ``camera``: a ``CameraRow`` (a float32 ``[48]`` row on the device, ``closed_loop.EgoLoop.camera``):
        its views go to the frame call as they are -- no staging, no copy, no event.  ``K``: other intrinsics for this
        frame's sky rays (then the ray matrix is staged like a moved camera's).  ``k`` outside ``0..T-1`` raises ``IndexError`` before anything is enqueued."""
        k = self.plan.check(k)
        rs = self.settings
        H, W = self._size
        if isinstance(camera, CameraRow):
            if K is not None:
                raise ValueError("a CameraRow carries its own ray matrix: K cannot be given with it")
            if camera.row.device != self.device:
                raise ValueError("the CameraRow is on %s, the session on %s" % (camera.row.device, self.device))
            view, proj, campos, ray = camera.views
        elif camera is None and (K is None or self.sky_cube is None):
            view, proj, campos, ray = self._tape_views[k]
        else:
            Kinv = self._Kinv
            if K is not None and self.sky_cube is not None:
                Kinv = np.linalg.inv(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64))
            if camera is None:
                camera = camera_from_tape(self._tape[k], W=W, H=H, device="cpu")
            view, proj, campos, ray = self._stage_camera(camera, Kinv)
        layer_bg = self._layer_bg
        if layers and layer_bg is None:
            layer_bg = self._layer_bg = _white(self.device)
        layer_bg, sky_cube = _or_empty(layer_bg, self.sky_cube)
        with torch.no_grad():
            ret = _C.rasterize_gaussians_bound_frame(
                self._tables_layers if layers else self._tables, k, rs.bg, layer_bg, bool(layers), rs.scale_modifier,
                view, proj, rs.tanfovx, rs.tanfovy, H, W, rs.sh_degree, campos, rs.debug, sky_cube, ray,
                self.sky_fill, bool(clamp), bool(planes), bool(rgb8), bool(truncate), out, self._affine[k])
        self.num_rendered = ret[0]
        return _frame_result(ret, rgb8, planes, layers)
