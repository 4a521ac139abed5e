"""CPU tests (-m "not gpu") of the device-pose hand-over (``tracks.PoseBatch.rows`` -> ``composed.PoseTable`` -> C ABI
``grpg_bind_device_poses``, csrc/segment_pose.hip): the exports and the ABI version, the life of a binding without a
device, the row index ``rows`` builds, and that ``_pack`` of a ``PoseTable`` never reads the pose tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
OK, NO_DEVICE, INVALID = 0, -2, -1


class Segment(ctypes.Structure):     # grpg_model_segment
    _fields_ = [("xyz", ctypes.c_void_p), ("scaling", ctypes.c_void_p), ("rotation", ctypes.c_void_p),
                ("opacity", ctypes.c_void_p), ("features_dc", ctypes.c_void_p),
                ("features_rest", ctypes.c_void_p), ("count", ctypes.c_int), ("fourier_dim", ctypes.c_int),
                ("rigid", ctypes.c_int), ("obj_rot", ctypes.c_float * 4), ("obj_trans", ctypes.c_float * 3),
                ("idft", ctypes.c_float * 8), ("flip", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the libamdhip64 the library links)
    lib = ctypes.CDLL(LIB)
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_bind_device_poses.restype = ctypes.c_int
    lib.grpg_bind_device_poses.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.grpg_device_poses_bound.restype = ctypes.c_int
    lib.grpg_compose.restype = ctypes.c_int
    lib.grpg_compose.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    return lib


def test_invalid_code_is_the_headers():
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"GRPG_ERR_INVALID_ARGUMENT\s*=?\s*\(?%d\b" % INVALID, header)
    assert re.search(r"GRPG_ERR_NO_DEVICE\s*=?\s*\(?%d\b" % NO_DEVICE, header)


def test_symbols_are_declared_and_exported_and_the_abi_version_stays(lib):
    with open(HEADER) as f:
        header = f.read()
    for s in ("grpg_bind_device_poses", "grpg_device_poses_bound"):
        assert re.search(r"GRPG_API int %s\(" % s, header), s
        assert hasattr(lib, s), s
    assert re.search(r"#define GRPG_ABI_VERSION 7\b", header)
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7
    from gaussianrpg_amd import build
    assert "segment_pose.hip" in build.HIP_UNITS


def _segments():
    host = ctypes.create_string_buffer(4096)            # pointers nobody dereferences: every call ends before that
    segs = (Segment * 2)()
    for s, rigid in zip(segs, (0, 1)):
        for f in ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest"):
            setattr(s, f, ctypes.addressof(host))
        s.count, s.fourier_dim, s.rigid = 32, 1, rigid
    return host, segs


def test_bind_refuses_bad_arguments_and_leaves_no_binding(lib):
    rows = (ctypes.c_int * 2)(-1, 0)
    ptr = ctypes.addressof(ctypes.create_string_buffer(64))
    for args in ((ptr, ptr, None, 2), (ptr, ptr, rows, 0), (ptr, ptr, rows, 1025), (None, ptr, rows, 2),
                 (ptr, None, rows, 2), (ptr, ptr, (ctypes.c_int * 2)(-2, 0), 2)):
        assert lib.grpg_bind_device_poses(ptr, ptr, rows, 2) == OK and lib.grpg_device_poses_bound() == 1
        assert lib.grpg_bind_device_poses(*args) == INVALID, args
        assert b"device poses" in lib.grpg_last_error()
        assert lib.grpg_device_poses_bound() == 0                     # the refused bind replaced the pending one by none
    # nothing bound to the device: the arrays may be NULL
    assert lib.grpg_bind_device_poses(None, None, (ctypes.c_int * 2)(-1, -1), 2) == OK
    assert lib.grpg_device_poses_bound() == 1
    assert lib.grpg_bind_device_poses(ptr, ptr, None, 2) == INVALID and lib.grpg_device_poses_bound() == 0


def test_the_consuming_call_drops_the_binding_without_a_device(lib):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    host, segs = _segments()
    ptr = ctypes.addressof(host)
    rows = (ctypes.c_int * 2)(-1, 0)
    assert lib.grpg_device_poses_bound() == 0
    assert lib.grpg_bind_device_poses(ptr, ptr, rows, 2) == OK          # the bind itself needs no device
    assert lib.grpg_device_poses_bound() == 1
    out = [ptr] * 5
    assert lib.grpg_compose(ctypes.addressof(segs), 2, 1, *out, None) == NO_DEVICE
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_device_poses_bound() == 0                           # consumed by the call that failed
    assert lib.grpg_compose(ctypes.addressof(segs), 2, 1, *out, None) == NO_DEVICE   # ... and not seen by the next
    assert lib.grpg_device_poses_bound() == 0


def test_every_composed_entry_consumes_a_binding(lib):
    """All-NULL calls: each entry fails (no device here, or its first argument check on a GPU machine) -- and takes the
    pending binding with it either way."""
    with open(HEADER) as f:
        header = f.read()
    entries = ["grpg_forward_composed", "grpg_forward_composed_flags", "grpg_forward_composed_layers",
               "grpg_forward_composed_frame", "grpg_forward_composed_features", "grpg_backward_composed",
               "grpg_backward_composed_features", "grpg_backward_composed_objects", "grpg_compose",
               "grpg_compose_features", "grpg_compose_features_backward"]
    rows = (ctypes.c_int * 1)(-1)
    for name in entries:
        m = re.search(r"GRPG_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, header)
        assert m, name
        argtypes = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            ctype = p[:-len(re.search(r"(\w+)$", p).group(1))].strip()
            if ctype == "grpg_alloc_fn" or ctype.endswith("*"):
                argtypes.append(ctypes.c_void_p)
            else:
                argtypes.append({"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float}[ctype])
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, argtypes
        assert lib.grpg_bind_device_poses(None, None, rows, 1) == OK and lib.grpg_device_poses_bound() == 1
        assert fn(*[None if t is ctypes.c_void_p else 0 for t in argtypes]) < 0, name
        assert lib.grpg_device_poses_bound() == 0, name


# ---- PoseBatch.rows ----

def _batch(T=3, A=5, grad=False):
    from gaussianrpg_amd.tracks import PoseBatch
    rot = torch.arange(T * A * 4, dtype=torch.float32).reshape(T, A, 4)
    trans = -torch.arange(T * A * 3, dtype=torch.float32).reshape(T, A, 3)
    if grad:
        rot.requires_grad_(True)
    return PoseBatch(rot, trans, torch.ones(T, A, dtype=torch.uint8))


@pytest.mark.parametrize("static", [0, 1, 2])
def test_rows_builds_the_index_list(static):
    from gaussianrpg_amd.composed import PoseTable
    batch = _batch(grad=True)
    for actors, times in (([3, 0, 4], [0.5, 0.25, 0.125]), ([], []), ([2, 2], [0.1, 0.2]), ([4], None)):
        table = batch.rows(1, actors, times, static=static)
        assert isinstance(table, PoseTable)
        n = len(actors)
        assert list(table.row) == [-1] * static + list(actors)
        assert list(table.posed) == [False] * static + [True] * n
        assert list(table.fourier_time) == [0.0] * static + (list(times) if times is not None else [0.0] * n)
        # the batch's own storage: views, no copy -- and the graph is kept
        assert table.rot.data_ptr() == batch.rot[1].data_ptr() and table.trans.data_ptr() == batch.trans[1].data_ptr()
        assert tuple(table.rot.shape) == (5, 4) and tuple(table.trans.shape) == (5, 3) and table.rot.requires_grad
    with pytest.raises(ValueError, match="one fourier_time per actor"):
        batch.rows(0, [0, 1], [0.0], static=static)
    with pytest.raises(IndexError, match="not one of the batch's 5 actors"):
        batch.rows(0, [5], static=static)
    with pytest.raises(IndexError, match="not one of the batch's 5 actors"):
        batch.rows(0, [-1], static=static)


# ---- _pack of a PoseTable ----

class _Untouchable(torch.Tensor):
    """a pose tensor that must stay where it is: every way to the host raises"""

    @staticmethod
    def _no(*a, **k):
        raise AssertionError("_pack read a pose tensor of a PoseTable")

    cpu = tolist = item = numpy = __array__ = __float__ = __iter__ = _no

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in ("cpu", "tolist", "item", "numpy", "to", "cat", "stack", "__array__"):
            cls._no()
        return super().__torch_function__(func, types, args, kwargs or {})


def _models(dims, n=5):
    from gaussianrpg_amd.composed import ModelParams
    return [ModelParams(torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 4), torch.zeros(n, 1),
                        torch.zeros(n, d, 3), torch.zeros(n, 3, 3)) for d in dims]


def test_pack_of_a_pose_table_never_reads_the_pose_tensors():
    from gaussianrpg_amd.composed import ActorPose, PoseTable, _pack, _posed_flags
    rng = np.random.RandomState(11)
    rot = torch.from_numpy(rng.normal(0, 1, (6, 4)).astype(np.float32)).as_subclass(_Untouchable)
    trans = torch.from_numpy(rng.normal(0, 30, (6, 3)).astype(np.float32)).as_subclass(_Untouchable)
    with pytest.raises(AssertionError, match="read a pose tensor"):      # the guard bites
        rot.cpu()
    with pytest.raises(AssertionError, match="read a pose tensor"):
        torch.cat([rot, rot])
    models = _models([1, 3, 2, 1, 2])
    host = ([0.5, 0.5, -0.5, 0.5], [1.0, -2.0, 3.0])
    table = PoseTable(rot, trans, [-1, 4, 0, -1, 4], [False, True, True, True, True], [0.9, 0.25, 0.5, 0.75, 0.25],
                      [None, None, None, host, None])
    lists, pose_arg, idft = _pack(models, table)
    pose_t, p_rot, p_trans, p_row = pose_arg
    assert p_rot.data_ptr() == rot.data_ptr() and p_trans.data_ptr() == trans.data_ptr()      # handed on as they are
    assert p_row.dtype == torch.int32 and not p_row.is_cuda and p_row.tolist() == [-1, 4, 0, -1, 4]
    assert pose_t.dtype == torch.float32 and tuple(pose_t.shape) == (5, 8) and not pose_t.is_cuda
    want = np.zeros((5, 8), np.float32)
    want[1:, 0] = 1.0                                                    # the posed flag; device rows stay zero
    want[3, 1:5], want[3, 5:8] = host
    assert pose_t.numpy().tobytes() == want.tobytes()
    # the IDFT rows are the host arithmetic of the list form on the same times (a static model's time is ignored)
    listed = [None] + [ActorPose([1.0, 0, 0, 0], [0.0, 0, 0], t) for t in (0.25, 0.5, 0.75, 0.25)]
    assert idft.numpy().tobytes() == _pack(models, listed)[2].numpy().tobytes()
    assert _posed_flags(table) == [False, True, True, True, True]
    assert len(lists) == 7 and lists[0][2] is models[2].xyz


def test_pack_of_a_pose_table_refuses_what_does_not_fit():
    from gaussianrpg_amd.composed import PoseTable, _pack
    rot, trans = torch.zeros(3, 4), torch.zeros(3, 3)
    models = _models([1, 2])
    with pytest.raises(ValueError, match="one row index, posed flag and fourier_time per model"):
        _pack(models, PoseTable(rot, trans, [-1, 0, 1], [False, True, True], [0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="neither -1 nor one of the table's 3 rows"):
        _pack(models, PoseTable(rot, trans, [-1, 3], [False, True], [0.0, 0.0]))
    with pytest.raises(ValueError, match="is static, but names row"):
        _pack(models, PoseTable(rot, trans, [0, 1], [False, True], [0.0, 0.0]))
    with pytest.raises(ValueError, match="neither a table row nor a host pose"):
        _pack(models, PoseTable(rot, trans, [-1, -1], [False, True], [0.0, 0.0]))
    with pytest.raises(ValueError, match=r"rot \[A,4\] and trans \[A,3\]"):
        _pack(models, PoseTable(rot, trans[:2], [-1, 0], [False, True], [0.0, 0.0]))
    with pytest.raises(TypeError, match="must be float32"):
        _pack(models, PoseTable(rot.double(), trans, [-1, 0], [False, True], [0.0, 0.0]))


def test_the_binding_takes_the_tuple_and_still_has_no_cpu_path():
    """the `poses` argument of the composed family: the table alone, or the 4-tuple -- and nothing else"""
    from gaussianrpg_amd.composed import PoseTable, compose
    from gaussianrpg_amd.rasterizer import _C
    models = _models([1, 2])
    table = PoseTable(torch.zeros(3, 4), torch.zeros(3, 3), [-1, 1], [False, True], [0.0, 0.5])
    with pytest.raises(RuntimeError, match="no CPU path"):               # parsed; refused at the device check
        compose(models, table)
    lists = [[m[f] for m in models] for f in range(6)] + [[torch.empty(0, dtype=torch.bool)] * 2]
    with pytest.raises(TypeError):                                       # a 3-tuple is not a pose argument
        _C.compose(*lists, (torch.zeros(2, 8), torch.zeros(3, 4), torch.zeros(3, 3)), torch.zeros(2, 8))


def test_the_pose_gradient_of_a_pose_table_is_what_the_index_select_graph_delivers():
    """dL_dposes [n,8] scattered to the table's shape equals, bit for bit, what autograd makes of the same rows
    through ``PoseBatch.frame``: dense, zero for the actors (and stamps) the frame does not show, summed for an actor
    it shows twice"""
    from gaussianrpg_amd.composed import _pack_table, _scatter_pose_grads
    from gaussianrpg_amd.tracks import PoseBatch
    g = torch.Generator().manual_seed(3)
    rot = torch.randn(3, 6, 4, generator=g).requires_grad_(True)
    trans = torch.randn(3, 6, 3, generator=g).requires_grad_(True)
    batch = PoseBatch(rot, trans, torch.ones(3, 6, dtype=torch.uint8))
    visible, t, static = [4, 1, 4, 0], 1, 2
    g_poses = torch.randn(static + len(visible), 8, generator=g)
    rows = batch.frame(t, visible, static=static)
    ((rows.rot * g_poses[:, 0:4]).sum() + (rows.trans * g_poses[:, 4:7]).sum()).backward()
    pose_arg, _ = _pack_table(static + len(visible), batch.rows(t, visible, static=static))
    g_rot, g_trans = _scatter_pose_grads(pose_arg, g_poses, True, True)
    assert tuple(g_rot.shape) == (6, 4) and tuple(g_trans.shape) == (6, 3)
    assert torch.equal(g_rot, rot.grad[t]) and torch.equal(g_trans, trans.grad[t])
    assert not g_rot[[2, 3, 5]].any() and torch.equal(g_rot[4], g_poses[2, 0:4] + g_poses[4, 0:4])
    assert _scatter_pose_grads(pose_arg, g_poses, False, True)[0] is None
    assert _scatter_pose_grads(pose_arg, g_poses, True, False)[1] is None
