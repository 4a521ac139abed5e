"""CPU test (-m "not gpu"): the C-ABI library loads and exports every symbol that
include/grpg_rasterizer.h declares (no compute calls: there is no GPU here), and the entry points
fail loudly -- not silently fall back -- when no HIP device is usable."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")


def _declared():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"GRPG_API\s+[\w\s\*]+?\b(grpg_\w+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    import torch  # noqa: F401  (loads the same libamdhip64 the extension will use)
    return ctypes.CDLL(LIB)


def test_header_declares_the_reference_entry_points():
    names = _declared()
    for required in ("grpg_forward", "grpg_backward", "grpg_mark_visible", "grpg_visible_filter"):
        assert required in names
    assert len(names) >= 9


def test_every_declared_symbol_is_exported(lib):
    for name in _declared():
        assert hasattr(lib, name), "libgrpg_rasterizer.so does not export %s" % name


def test_abi_version_and_loud_failure_without_gpu(lib):
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib.grpg_mark_visible.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    rc = lib.grpg_mark_visible(0, None, None, None, None, None)
    assert rc == -2, "expected GRPG_ERR_NO_DEVICE, got %d" % rc      # no CPU fallback
    assert b"no usable HIP device" in lib.grpg_last_error()
    # the "next rows" entry points fail the same way: distCUDA2 and the rgb8 frame pack
    lib.grpg_knn_mean_dist2.restype = ctypes.c_int
    assert lib.grpg_knn_mean_dist2(4, None, None, None, None, None) == -2
    lib.grpg_pack_rgb_u8_hwc.restype = ctypes.c_int
    assert lib.grpg_pack_rgb_u8_hwc(None, None, 4, 4, 1, None) == -2
    lib.grpg_knn_workspace_bytes.restype = ctypes.c_size_t
    assert lib.grpg_knn_workspace_bytes(1000) > 1000 * 24   # pure size query, no device needed


def test_default_binning_algorithm_of_a_fresh_process(lib):
    """Without GRPG_BINNING a fresh process bins hierarchically (include/grpg_rasterizer.h): the default comes from a
    namespace-scope initializer of csrc/api.hip, which a size query cannot see going wrong."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "GRPG_BINNING"}
    out = subprocess.run([sys.executable, "-c", "import ctypes, sys; "
                          "print(ctypes.CDLL(sys.argv[1]).grpg_get_binning_algorithm())", LIB],
                         env=env, capture_output=True, text=True, check=True).stdout.strip()
    assert out == re.search(r"#define\s+GRPG_BINNING_ALG_HIER\s+(\d+)", open(HEADER).read()).group(1)


def test_python_api_rejects_cpu_tensors():
    import torch
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4),
                                       0, torch.zeros(3), False, False)
    r = GaussianRasterizer(rs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(torch.zeros(2, 3), None, torch.ones(2, 1), colors_precomp=torch.ones(2, 3),
          scales=torch.ones(2, 3), rotations=torch.ones(2, 4))
    # the reference's two validation messages (diff_gaussian_rasterization/__init__.py:202,205)
    with pytest.raises(Exception, match="excatly one of either SHs"):
        r(torch.zeros(2, 3), None, torch.ones(2, 1), scales=torch.ones(2, 3), rotations=torch.ones(2, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(torch.zeros(2, 3), None, torch.ones(2, 1), colors_precomp=torch.ones(2, 3))


def test_extension_is_importable_under_the_reference_dotted_names():
    """DGR/setup.py:22 builds ``diff_gaussian_rasterization._C`` and the package imports it with
    ``from . import _C`` (DGR/diff_gaussian_rasterization/__init__.py:14); simple-knn's is
    ``simple_knn._C``.  All spellings must resolve to the gfx950 extension."""
    import importlib
    import subprocess
    import sys
    code = ("import diff_gaussian_rasterization._C as a; import importlib;"
            "b = importlib.import_module('diff_gaussian_rasterization._C');"
            "from diff_gaussian_rasterization import _C as c; assert a is b is c;"
            "assert hasattr(a, 'rasterize_gaussians') and hasattr(a, 'rasterize_gaussians_backward');"
            "from simple_knn._C import distCUDA2; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr
    importlib.import_module("diff_gaussian_rasterization._C")
