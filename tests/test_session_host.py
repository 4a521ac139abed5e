"""CPU tests (-m "not gpu") of the closed-loop session's host half: ``session.TapePlan`` -- visible lists, index
ranges, Gaussian counts, Fourier times, IDFT rows and the row lists of ``grpg_frame_tables_bake`` --,
``trajectory.extend_tape``, and the three new C entry points through ctypes (size query, loud failure without a
device, exports).  The yardstick of the visible lists and ranges is an inline restatement of the reference's
``parse_camera`` loop (street_gaussian_model.py:239-262)."""
import ctypes
import os
import re

import pytest
import torch

from gaussianrpg_amd.composed import MAX_FOURIER, idft_weights
from gaussianrpg_amd.session import TapePlan, fourier_time
from gaussianrpg_amd.trajectory import extend_tape, make_tape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")

# five actors: first / last stamp, Gaussians, Fourier dimension, (start_frame, end_frame, fourier_scale)
START = [10.0, 10.2, 10.0, 10.4, 10.1]
END = [10.5, 10.6, 10.3, 10.9, 10.1]
COUNTS = [8, 33, 64, 20, 48]
DIMS = [1, 3, 1, 2, 1]
SPANS = [(0, 5, 1.0), (2, 6, 0.5), (0, 3, 1.0), (4, 9, 2.0), (1, 1, 1.0)]   # actor 4: one frame, Fourier dimension 1
NB = 2000
VISIBILITY = [True, True, False, True, True]                                 # actor 2 switched off


def _tape():
    """stamps: before every actor; exactly at starts (10.0, 10.2, 10.4) and ends (10.5, 10.6, 10.9); one repeated
    stamp (10.2 twice); frames that hit time 0 (frame == start_frame) and fourier_scale (frame == end_frame)"""
    stamps = [9.9, 10.0, 10.1, 10.2, 10.2, 10.3, 10.4, 10.5, 10.6, 10.9, 10.45, 11.5]
    frames = [0, 0, 1, 2, 2, 3, 4, 5, 6, 9, 5, 12]
    tape = make_tape(len(stamps))
    for e, t, f in zip(tape, stamps, frames):
        e["timestamp"], e["frame"] = t, f
    return tape


def _reference_parse(timestamp, visibility):
    """street_gaussian_model.py:239-262, restated: graph_obj_list, graph_gaussian_range, num_gaussians"""
    num_gaussians = NB
    graph_obj_list = []
    for i in range(len(COUNTS)):
        start_timestamp, end_timestamp = START[i], END[i]
        if timestamp >= start_timestamp and timestamp <= end_timestamp and (visibility is None or visibility[i]):
            graph_obj_list.append(i)
            num_gaussians += COUNTS[i]
    graph_gaussian_range = dict()
    idx = 0
    graph_gaussian_range["background"] = [idx, idx + NB - 1]
    idx += NB
    for i in graph_obj_list:
        graph_gaussian_range[i] = [idx, idx + COUNTS[i] - 1]
        idx += COUNTS[i]
    return graph_obj_list, graph_gaussian_range, num_gaussians


@pytest.fixture(scope="module")
def tape():
    return _tape()


@pytest.fixture(scope="module", params=[None, VISIBILITY], ids=["all", "actor2_off"])
def plan(request, tape):
    return TapePlan(START, END, COUNTS, DIMS, tape, SPANS, request.param, [NB]), request.param


def test_visible_lists_ranges_and_counts(plan, tape):
    plan, visibility = plan
    assert len(plan) == len(tape) == 12
    for k, e in enumerate(tape):
        vis, ranges, n = _reference_parse(e["timestamp"], visibility)
        assert plan.visible(k) == vis, "frame %d" % k
        assert plan.ranges(k) == ranges
        assert plan.num_gaussians(k) == n
        assert plan.num_models(k) == 1 + len(vis)
    assert plan.visible(0) == [] and plan.visible(11) == []                 # before / after every actor
    assert plan.visible(3) == plan.visible(4)                               # the repeated stamp
    assert 0 in plan.visible(1) and 0 in plan.visible(7)                    # exactly at a start and at an end
    assert 1 in plan.visible(3) and 1 in plan.visible(8) and 3 in plan.visible(9)
    assert plan.visible(2) == ([0, 2, 4] if visibility is None else [0, 4])   # actor 4 lives at one stamp


def test_fourier_times_and_idft_rows(plan, tape):
    plan, _ = plan
    seen = set()
    for k, e in enumerate(tape):
        vis = plan.visible(k)
        times = plan.fourier_times(k)
        rows = plan.idft_rows(k)
        assert tuple(rows.shape) == (1 + len(vis), MAX_FOURIER) and rows.dtype == torch.float32
        assert rows[0].tolist() == [1.0] + [0.0] * (MAX_FOURIER - 1)         # the background: cos(0)
        for i, a in enumerate(vis):
            s, en, scale = SPANS[a]
            want = 0.0 if en == s else scale * ((e["frame"] - s) / (en - s))   # gaussian_model_actor.py:74-75
            assert times[i] == want == fourier_time(e["frame"], SPANS[a])
            w = idft_weights(want, DIMS[a])
            assert rows[1 + i].tolist() == w + [0.0] * (MAX_FOURIER - DIMS[a]), "frame %d actor %d" % (k, a)
            if DIMS[a] > 1:
                seen.add("zero" if want == 0.0 else "scale" if want == scale else "inside")
    assert seen == {"zero", "scale", "inside"}        # times 0 and fourier_scale occur on a Fourier actor


def test_row_lists_of_the_bake(plan):
    plan, _ = plan
    A = len(COUNTS)
    assert plan.frame_first[0] == 0 and len(plan.frame_first) == len(plan) + 1
    assert len(plan.row_model) == len(plan.row_pose) == plan.frame_first[-1] == plan.idft.shape[0]
    for k in range(len(plan)):
        lo, hi = plan.frame_first[k], plan.frame_first[k + 1]
        vis = plan.visible(k)
        assert plan.row_model[lo:hi] == [0] + [1 + a for a in vis]
        assert plan.row_pose[lo:hi] == [-1] + [k * A + a for a in vis]      # rows of the flattened [T,A,*] batch


def test_two_static_models_share_the_background_range(tape):
    plan = TapePlan(START, END, COUNTS, DIMS, tape, SPANS, None, [1500, 500])
    assert plan.ranges(1)["background"] == [0, 1999] and plan.num_models(1) == 2 + len(plan.visible(1))
    lo = plan.frame_first[1]
    assert plan.row_model[lo:lo + 2] == [0, 1] and plan.row_pose[lo:lo + 2] == [-1, -1]


def test_value_and_index_errors(tape):
    with pytest.raises(ValueError, match="end_frame == start_frame"):
        TapePlan(START, END, COUNTS, DIMS, tape, [(0, 5, 1.0), (2, 2, 0.5)] + SPANS[2:], None, [NB])
    with pytest.raises(ValueError, match="visibility"):
        TapePlan(START, END, COUNTS, DIMS, tape, SPANS, [True], [NB])
    with pytest.raises(ValueError, match="empty"):
        TapePlan(START, END, COUNTS, DIMS, [], SPANS, None, [NB])
    plan = TapePlan(START, END, COUNTS, DIMS, tape, SPANS, None, [NB])
    for bad in (-1, 12, 1000):
        for call in (plan.visible, plan.ranges, plan.num_gaussians, plan.idft_rows, plan.check):
            with pytest.raises(IndexError):
                call(bad)
    with pytest.raises(TypeError):
        plan.visible(1.5)


def test_extend_tape():
    tape = make_tape(4)
    more = extend_tape(tape, 3, 0.1)
    assert len(tape) == 4 and len(more) == 7 and more[:4] == tape
    last = tape[-1]
    for i, e in enumerate(more[4:], 1):
        assert e["id"] == last["id"] + i and e["timestamp"] == last["timestamp"] + i * 0.1
        assert e["rotation_matrix"] == last["rotation_matrix"] and e["position"] == last["position"]
        assert e["ego_pose"] == last["ego_pose"] and "frame" not in e
    assert extend_tape(tape, 0, 0.1) == tape
    framed = extend_tape([dict(last, frame=40)], 2, 0.5)
    assert [e["frame"] for e in framed] == [40, 41, 42]
    with pytest.raises(ValueError):
        extend_tape([], 1, 0.1)
    with pytest.raises(ValueError):
        extend_tape(tape, -1, 0.1)


# ---- the C entry points, through ctypes ----

NEW_SYMBOLS = ("grpg_frame_tables_bytes", "grpg_frame_tables_bake", "grpg_bind_frame_table", "grpg_frame_tables_bound")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    lib = ctypes.CDLL(LIB)
    lib.grpg_frame_tables_bytes.restype = ctypes.c_size_t
    lib.grpg_frame_tables_bytes.argtypes = [ctypes.c_longlong]
    lib.grpg_bind_frame_table.restype = ctypes.c_int
    lib.grpg_bind_frame_table.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.grpg_frame_tables_bake.restype = ctypes.c_int
    lib.grpg_frame_tables_bake.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + \
        [ctypes.c_void_p] * 6 + [ctypes.c_longlong, ctypes.c_void_p]
    lib.grpg_frame_tables_bound.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    return lib


def test_new_symbols_are_declared_and_exported(lib):
    declared = set(re.findall(r"GRPG_API\s+[\w\s\*]+?\b(grpg_\w+)\s*\(", open(HEADER).read()))
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in the header" % name
        assert hasattr(lib, name), "libgrpg_rasterizer.so does not export %s" % name
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7          # additive: the version stays


def test_size_query_needs_no_device(lib):
    assert lib.grpg_frame_tables_bytes(0) == 0 and lib.grpg_frame_tables_bytes(-3) == 0
    assert lib.grpg_frame_tables_bytes(1) == 144                  # one SegmentDev row
    assert lib.grpg_frame_tables_bytes(200 * 51) == 144 * 200 * 51


def test_bake_and_bind_without_a_device(lib):
    """On a machine without a GPU both fail with GRPG_ERR_NO_DEVICE and leave no binding; with one, the same
    argument-free calls are refused as invalid arguments -- either way nothing is enqueued."""
    expect = -1 if torch.cuda.is_available() else -2
    assert lib.grpg_frame_tables_bound() == 0
    assert lib.grpg_bind_frame_table(None, 3, 100) == expect
    assert lib.grpg_frame_tables_bound() == 0
    assert lib.grpg_frame_tables_bake(None, None, 0, None, 0, None, None, None, None, None, None, 0, None) == expect
    if expect == -2:
        assert b"no usable HIP device" in lib.grpg_last_error()
        rows = (ctypes.c_char * 4096)()
        aligned = (ctypes.addressof(rows) + 15) & ~15
        assert lib.grpg_bind_frame_table(aligned, 3, 100) == -2      # well-formed arguments: still no device
        assert lib.grpg_frame_tables_bound() == 0
