"""CPU tests (-m "not gpu") of the colour correction inside the one-call frame's epilogue (C ABI
``grpg_bind_frame_correction``; csrc/render_fwd.hip ``frame_finish``, csrc/color_math.h): the exports and the ABI
version, the life of a binding without a device, the register budget of the render instantiations that carry the
epilogue, and that the input tests/test_gpu_frame_corrected.py uses can see a clamp in the wrong place."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import color_correction_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
OK, NO_DEVICE, INVALID = 0, -2, -1


class Epilogue(ctypes.Structure):     # grpg_frame_epilogue
    _fields_ = [("sky_cube", ctypes.c_void_p), ("sky_res", ctypes.c_int), ("ray_matrix", ctypes.c_void_p),
                ("ray_matrix_on_device", ctypes.c_int), ("sky_fill", ctypes.c_float), ("clamp", ctypes.c_int),
                ("out_rgb8", ctypes.c_void_p), ("truncate", ctypes.c_int), ("out_rgb8_on_host", ctypes.c_int)]


def _header():
    with open(HEADER) as f:
        return f.read()


def _declare(lib, name):
    """restype / argtypes of an entry point from its declaration in the header"""
    m = re.search(r"GRPG_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, _header())
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
    return fn


def _nulls(fn, **put):
    """all-NULL / all-zero arguments; put: position -> value"""
    args = [None if t is ctypes.c_void_p else 0 for t in fn.argtypes]
    for k, v in put.items():
        args[int(k)] = v
    return args


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the libamdhip64 the library links)
    lib = ctypes.CDLL(LIB)
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_bind_frame_correction.restype = ctypes.c_int
    lib.grpg_bind_frame_correction.argtypes = [ctypes.c_void_p]
    lib.grpg_frame_correction_bound.restype = ctypes.c_int
    lib.grpg_frame_correction_bound.argtypes = []
    return lib


def test_symbols_are_declared_and_exported_and_the_abi_version_stays(lib):
    header = _header()
    for s in ("grpg_bind_frame_correction", "grpg_frame_correction_bound"):
        assert re.search(r"GRPG_API int %s\(" % s, header), s
        assert hasattr(lib, s), s
    assert re.search(r"#define GRPG_ABI_VERSION 7\b", header)
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7
    assert re.search(r"GRPG_ERR_INVALID_ARGUMENT\s*=?\s*\(?%d\b" % INVALID, header)
    assert re.search(r"GRPG_ERR_NO_DEVICE\s*=?\s*\(?%d\b" % NO_DEVICE, header)
    # the struct the existing ctypes callers lay out did not grow
    m = re.search(r"typedef struct grpg_frame_epilogue \{(.*?)\} grpg_frame_epilogue;", header, re.S)
    assert [f.split()[-1].lstrip("*") for f in m.group(1).strip().rstrip(";").split(";")] == [n for n, _ in Epilogue._fields_]


def test_the_life_of_a_binding_without_a_device(lib):
    buf = ctypes.create_string_buffer(64)            # a pointer nobody dereferences: every call ends before that
    other = ctypes.create_string_buffer(64)
    ptr, ptr2 = ctypes.addressof(buf), ctypes.addressof(other)
    frame = _declare(lib, "grpg_forward_frame")
    composed = _declare(lib, "grpg_forward_composed_frame")
    epi = Epilogue()
    last = len(frame.argtypes) - 1
    failed = (lambda rc: rc < 0) if torch.cuda.is_available() else (lambda rc: rc == NO_DEVICE)

    assert lib.grpg_frame_correction_bound() == 0
    # NULL is refused and leaves nothing bound -- not even what was pending
    assert lib.grpg_bind_frame_correction(None) == INVALID and b"frame correction" in lib.grpg_last_error()
    assert lib.grpg_frame_correction_bound() == 0
    assert lib.grpg_bind_frame_correction(ptr) == OK and lib.grpg_frame_correction_bound() == 1
    assert lib.grpg_bind_frame_correction(None) == INVALID and lib.grpg_frame_correction_bound() == 0
    # bound; the query is pure
    assert lib.grpg_bind_frame_correction(ptr) == OK
    assert lib.grpg_frame_correction_bound() == 1 and lib.grpg_frame_correction_bound() == 1
    # the frame call takes it, although it fails (here: no device; on a GPU machine: its first argument check)
    assert failed(frame(*_nulls(frame, **{str(last): ctypes.addressof(epi)})))
    if not torch.cuda.is_available():
        assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_frame_correction_bound() == 0
    # ... and so does the composed frame call
    assert lib.grpg_bind_frame_correction(ptr) == OK and lib.grpg_frame_correction_bound() == 1
    assert composed(*_nulls(composed, **{str(len(composed.argtypes) - 1): ctypes.addressof(epi)})) < 0
    assert lib.grpg_frame_correction_bound() == 0
    # a correction needs an epilogue to run in: refused with a message before a device is looked for, and taken
    assert lib.grpg_bind_frame_correction(ptr) == OK
    assert frame(*_nulls(frame)) == INVALID and b"no epilogue" in lib.grpg_last_error()
    assert lib.grpg_frame_correction_bound() == 0
    assert failed(frame(*_nulls(frame)))                      # nothing bound any more: the plain call's own failure
    assert b"no epilogue" not in lib.grpg_last_error()
    # a rebind replaces the pending binding (still one binding, and one frame call clears it)
    assert lib.grpg_bind_frame_correction(ptr) == OK and lib.grpg_bind_frame_correction(ptr2) == OK
    assert lib.grpg_frame_correction_bound() == 1
    # calls that are not frame calls leave it bound
    for name in ("grpg_forward", "grpg_forward_layers", "grpg_forward_composed", "grpg_forward_composed_layers",
                 "grpg_color_correct_forward", "grpg_compose"):
        fn = _declare(lib, name)
        assert fn(*_nulls(fn)) < 0, name
        assert lib.grpg_frame_correction_bound() == 1, name
    rows = (ctypes.c_int * 1)(-1)
    lib.grpg_bind_device_poses.restype = ctypes.c_int
    lib.grpg_bind_device_poses.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert lib.grpg_bind_device_poses(None, None, rows, 1) == OK        # the other binding lives beside it
    assert lib.grpg_frame_correction_bound() == 1 and lib.grpg_device_poses_bound() == 1
    assert composed(*_nulls(composed, **{str(len(composed.argtypes) - 1): ctypes.addressof(epi)})) < 0
    assert lib.grpg_frame_correction_bound() == 0 and lib.grpg_device_poses_bound() == 0     # both rode on that call


def test_the_epilogue_instantiations_keep_their_register_budget():
    """The correction is a run-time branch of the EXISTING instantiations of render_forward_kernel (EPI, the last
    template argument): four waves per SIMD and no scratch, as before; the plain evaluation kernel keeps its 96."""
    from gaussianrpg_amd import build
    res = {k: v for k, v in build.kernel_resources("render_fwd.hip").items() if "render_forward_kernel" in k}
    assert len(res) == 7, sorted(res)
    epi = {k: v for k, v in res.items() if re.search(r"render_forward_kernelIL.*Lb1EEEv", k)}
    assert len(epi) == 2, sorted(res)
    for k, v in epi.items():
        print(k[:64], v)
        assert v["occupancy"] == 4 and v["scratch"] == 0 and v["vgprs"] <= 128, (k, v)
    plain = [v for k, v in res.items() if "ILb0ELi1ELi0ELb0ELb0EE" in k]
    assert len(plain) == 1 and plain[0]["vgprs"] <= 96 and plain[0]["occupancy"] == 5 and plain[0]["scratch"] == 0


def test_a_misplaced_clamp_is_visible_on_the_telling_input():
    """The epilogue clamps the composite only BEHIND the map.  On values outside [0,1] -- what the uncorrected
    colour plus a clamped sky sample reaches -- clamp-then-map and map-then-clamp differ after the final clamp, in
    planes and in bytes, for the matrices the GPU test uses."""
    rng = np.random.RandomState(5)
    x = rng.uniform(0.0, 2.0, (3, 40, 50)).astype(np.float32)      # rgb in [0,1] + sky (1 - acc) in [0,1]
    assert (x > 1.0).mean() > 0.2
    for kind, seed in (("near", 9), ("wide", 1)):
        A = T.build_affine(kind, seed=seed)
        right = np.clip(T.forward32(A, x), 0.0, 1.0)
        wrong = np.clip(T.forward32(A, np.clip(x, 0.0, 1.0)), 0.0, 1.0)
        b_right, b_wrong = (right * 255.0).astype(np.uint8), (wrong * 255.0).astype(np.uint8)
        share = float((b_right != b_wrong).mean())
        print(kind, "bytes that see the order: %.3f" % share)
        assert share > 0.05, (kind, share)
    # the identity cannot tell them apart after the final clamp: the GPU test's identity case checks something else
    eye = T.build_affine("identity")
    assert np.array_equal(np.clip(T.forward32(eye, x), 0, 1), np.clip(T.forward32(eye, np.clip(x, 0, 1)), 0, 1))
