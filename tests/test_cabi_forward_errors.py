"""The nine forward entry points of the C ABI answer bad arguments with the same (return code,
grpg_last_error() text) pairs as the library did before the forward path of csrc/api.hip was split
into stages: which check fires first is part of the contract of every entry.

Every case is a call that returns before anything is enqueued.  The allocator callbacks handed to
the library return NULL, so even a call whose arguments pass every check ends at "allocation failed"
-- no kernel is launched and no copy is queued, on a machine without a device (where nearly every
case ends at GRPG_ERR_NO_DEVICE, except the checks an entry makes before it looks for a device) and
on one with a device (where the argument checks themselves answer).

The expected pairs (tests/golden/cabi_forward_errors.json) were recorded from a build of the commit
BEFORE the split, with this file run as a script:
    python tests/test_cabi_forward_errors.py <libgrpg_rasterizer.so of that commit> <json>
once without a device ("no_device") and once on an MI355X ("device").
"""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cabi_forward_errors.json")

ENTRIES = ["grpg_forward", "grpg_forward_flags", "grpg_forward_layers", "grpg_forward_deferred",
           "grpg_forward_frame", "grpg_forward_composed", "grpg_forward_composed_flags",
           "grpg_forward_composed_layers", "grpg_forward_composed_frame"]

ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
ALLOC_CALLS = []


def _alloc_null(nbytes, user):
    ALLOC_CALLS.append(nbytes)
    return None      # NULL: the forward stops at "allocation failed", before its first launch


ALLOC_NULL = ALLOC_FN(_alloc_null)


class Segment(ctypes.Structure):     # grpg_model_segment
    _fields_ = [("xyz", ctypes.c_void_p), ("scaling", ctypes.c_void_p), ("rotation", ctypes.c_void_p),
                ("opacity", ctypes.c_void_p), ("features_dc", ctypes.c_void_p),
                ("features_rest", ctypes.c_void_p), ("count", ctypes.c_int), ("fourier_dim", ctypes.c_int),
                ("rigid", ctypes.c_int), ("obj_rot", ctypes.c_float * 4), ("obj_trans", ctypes.c_float * 3),
                ("idft", ctypes.c_float * 8), ("flip", ctypes.c_void_p)]


class Epilogue(ctypes.Structure):    # grpg_frame_epilogue
    _fields_ = [("sky_cube", ctypes.c_void_p), ("sky_res", ctypes.c_int), ("ray_matrix", ctypes.c_void_p),
                ("ray_matrix_on_device", ctypes.c_int), ("sky_fill", ctypes.c_float), ("clamp", ctypes.c_int),
                ("out_rgb8", ctypes.c_void_p), ("truncate", ctypes.c_int), ("out_rgb8_on_host", ctypes.c_int)]


def _signatures():
    """entry -> [(parameter name, ctypes type)], read from the header's declarations."""
    text = open(HEADER).read()
    sigs = {}
    for name in ENTRIES:
        m = re.search(r"GRPG_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, "no declaration of %s in the header" % name
        params = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            pname = re.search(r"(\w+)$", p).group(1)
            ctype = p[:-len(pname)].strip()
            if ctype == "grpg_alloc_fn":
                t = ALLOC_FN
            elif ctype.endswith("*"):
                t = ctypes.c_void_p
            else:
                t = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float}[ctype]
            params.append((pname, t))
        sigs[name] = params
    return sigs


HOST = ctypes.create_string_buffer(4096)      # "valid-looking" pointers: host memory nobody dereferences
PTR = ctypes.addressof(HOST)
TICKET = ctypes.c_int(0)
ALLOCS = ("geometry_alloc", "binning_alloc", "image_alloc")
PLANES = ("out_color_bg", "out_alpha_bg", "out_color_obj", "out_alpha_obj")


def _base():
    """Arguments that look like a real call: every check passes and the forward asks for its blobs."""
    v = {n: ALLOC_NULL for n in ALLOCS}
    v.update(geometry_user=None, binning_user=None, image_user=None, hip_stream=None, epilogue=None,
             colors_precomp=None, cov3D_precomp=None, semantics=None, out_semantic=None, segment_class=None,
             P=64, D=1, M=4, S=0, width=64, height=48, scale_modifier=1.0, tan_fovx=0.5, tan_fovy=0.5,
             prefiltered=0, debug=0, flags=0, num_segments=2, ticket=ctypes.addressof(TICKET),
             seg=[dict(count=32), dict(count=32, rigid=1)])
    return v


CASES = {
    "all_null": None,                                   # every argument zero / NULL
    "valid_looking": {},
    "negative_P": dict(P=-1),
    "negative_width": dict(width=-1),
    "zero_height": dict(height=0),
    "negative_S": dict(S=-1),
    "negative_M": dict(M=-1),
    "null_allocators": {n: None for n in ALLOCS},
    "null_binning_allocator": dict(binning_alloc=None),
    "null_background": dict(background=None),
    "null_viewmatrix": dict(viewmatrix=None),
    "null_out_depth": dict(out_depth=None),
    "P_2_28": dict(P=1 << 28, seg=[dict(count=1 << 27), dict(count=1 << 27)]),
    "P_2_27": dict(P=1 << 27, seg=[dict(count=1 << 26), dict(count=1 << 26)]),
    "three_of_four_planes": dict(out_alpha_obj=None),
    "one_of_four_planes": dict(out_color_bg=None, out_alpha_bg=None, out_color_obj=None),
    "no_layer_planes": {n: None for n in PLANES},
    "null_layer_background": dict(layer_background=None),
    "null_layer_class": dict(layer_class=None),
    "three_planes_P_2_27": dict(out_alpha_obj=None, P=1 << 27, seg=[dict(count=1 << 26), dict(count=1 << 26)]),
    "sh_degree_4": dict(D=4, M=25),
    "sh_degree_negative": dict(D=-1),
    "sh_degree_beyond_M": dict(D=3, M=4),
    "M_17": dict(M=17),
    "M_0": dict(M=0),
    "null_means3D": dict(means3D=None),
    "null_scales": dict(scales=None),
    "null_shs": dict(shs=None),
    "semantic_without_planes": dict(S=3),
    "segment_count_zero": dict(seg=[dict(count=32), dict(count=0)]),
    "segment_count_negative": dict(seg=[dict(count=-5), dict(count=32)]),
    "segment_null_array": dict(seg=[dict(count=32), dict(count=32, opacity=None)]),
    "segment_fourier_dim_0": dict(seg=[dict(count=32, fourier_dim=0)], num_segments=1),
    "segment_fourier_dim_9": dict(seg=[dict(count=32, fourier_dim=9)], num_segments=1),
    "null_segments": dict(segments=None),
    "zero_segments": dict(num_segments=0),
    "too_many_segments": dict(num_segments=1025),
    "null_ticket": dict(ticket=None),
    "epilogue_sky_without_res": dict(epi=dict(sky_cube=PTR, sky_res=0)),
    "epilogue_bytes_without_planes": dict(epi=dict(out_rgb8=PTR), out_color=None, out_depth=None, out_alpha=None),
    "epilogue_no_bytes_no_planes": dict(epi=dict(clamp=1), out_color=None),
}


def _call(lib, name, params, case):
    keep = []                                           # ctypes objects the call points into
    if case is None:
        vals = {}
    else:
        vals = _base()
        vals.update(case)
        segs = (Segment * max(len(vals["seg"]), 1))()
        for s, spec in zip(segs, vals["seg"]):
            for f in ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest"):
                setattr(s, f, PTR)
            s.fourier_dim = 1
            for k, x in spec.items():
                setattr(s, k, x)
        keep.append(segs)
        vals.setdefault("segments", ctypes.addressof(segs))
        if "epi" in vals:
            e = Epilogue(**vals["epi"])
            keep.append(e)
            vals["epilogue"] = ctypes.addressof(e)
    args = []
    for pname, t in params:
        if case is None:
            x = t() if t is ALLOC_FN else (None if t is ctypes.c_void_p else 0)
        else:
            x = vals.get(pname, PTR if t is ctypes.c_void_p else None)
            assert x is not None or t is ctypes.c_void_p or t is ALLOC_FN, (name, pname)
            if x is None and t is ALLOC_FN:
                x = ALLOC_FN()
        args.append(x)
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [t for _, t in params]
    lib.grpg_last_error.restype = ctypes.c_char_p
    rc = fn(*args)
    return [rc, lib.grpg_last_error().decode()]


def run_all(lib_path):
    import torch  # noqa: F401  (loads the libamdhip64 the library links against, as test_cabi_exports does)
    lib = ctypes.CDLL(lib_path)
    sigs = _signatures()
    return {name: {cid: _call(lib, name, sigs[name], case) for cid, case in CASES.items()} for name in ENTRIES}


def _mode():
    import torch
    return "device" if torch.cuda.is_available() else "no_device"


def _check(mode):
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    want = json.load(open(GOLDEN))[mode]
    got = run_all(LIB)
    assert sorted(got) == sorted(want) == sorted(ENTRIES)
    bad = []
    for name in ENTRIES:
        assert sorted(got[name]) == sorted(want[name]) == sorted(CASES), name
        for cid in CASES:
            if got[name][cid] != want[name][cid]:
                bad.append((name, cid, got[name][cid], want[name][cid]))
    assert not bad, "(entry, case, got, recorded before the split):\n" + "\n".join(map(repr, bad))
    for name in ENTRIES:                                # every case is an error return: nothing was enqueued
        for cid, (rc, msg) in got[name].items():
            assert rc < 0 and msg, (name, cid, rc, msg)


def test_forward_entries_report_the_recorded_errors():
    """Without a device: the "no_device" pairs; with one: the "device" pairs."""
    _check(_mode())


@pytest.mark.gpu
def test_forward_entries_validate_arguments_on_device():
    """The argument checks proper (negative sizes, NULL allocators, P >= 2^28, three of four layer
    planes, a bad SH degree, a segment with count <= 0, ...) -- reached only behind ensure_device."""
    _check("device")


if __name__ == "__main__":      # recorder: <library> <json>; merges this machine's mode into the file
    lib_path, out = sys.argv[1], sys.argv[2]
    table = json.load(open(out)) if os.path.exists(out) else {}
    table[_mode()] = run_all(os.path.abspath(lib_path))
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %s: %d entries x %d cases, %d allocator calls" % (_mode(), len(ENTRIES), len(CASES), len(ALLOC_CALLS)))
