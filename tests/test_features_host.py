"""CPU tests of the feature planes of a composed frame: the float64 truth against the reference-derived quaternion
fixture, the argument refusals of the four C entries through ctypes (without a GPU: GRPG_ERR_NO_DEVICE, no fallback),
and the Python refusals of gaussianrpg_amd.composed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import feature_truth as ft
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
ENTRIES = ("grpg_compose_features", "grpg_compose_features_backward", "grpg_forward_composed_features",
           "grpg_backward_composed_features")


def test_truth_normal_is_a_column_of_the_reference_matrix():
    """tests/golden/ref_quat.npz holds the reference's quaternion_to_matrix_numpy (general_utils.py:103-122) of 64
    quaternions: for each and each choice of the smallest scale k the truth's normal is +-R_ref[:, k] -- the
    (r, x, y, z) convention and column-not-row."""
    z = np.load(os.path.join(GOLDEN, "ref_quat.npz"))
    q, R = torch.from_numpy(z["q"]), z["R"]
    n = q.shape[0]
    means = torch.randn(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 5
    campos = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    for k in range(3):
        scales = torch.ones(n, 3, dtype=torch.float64)
        scales[:, k] = 0.5
        got, kk, dot = ft.normals_of(means, scales, q, campos, with_details=True)
        assert bool((kk == k).all())
        col = R[:, :, k]
        sign = np.where(dot.numpy() >= 0, 1.0, -1.0)[:, None]
        np.testing.assert_allclose(got.numpy(), sign * col, rtol=0, atol=1e-12)
        # a row would differ: the fixture's rotations are not symmetric
        assert np.abs(np.abs(got.numpy()) - np.abs(R[:, k, :])).max() > 1e-2
        # the normal faces the camera
        d = (means - campos).numpy()
        assert (np.sum(-d * got.numpy(), axis=1) >= 0).all()


def test_truth_feature_order_and_null_semantics():
    from gaussianrpg_amd.composed import ModelParams
    g = torch.Generator().manual_seed(2)
    mk = lambda n: ModelParams(torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g),   # noqa: E731
                               torch.randn(n, 4, generator=g), torch.randn(n, 1, generator=g),
                               torch.randn(n, 1, 3, generator=g), torch.randn(n, 0, 3, generator=g))
    models = [mk(5), mk(3)]
    poses = [None, ([0.9, 0.1, -0.3, 0.2], [1.0, 2.0, 3.0], 0.0)]
    sem = [None, torch.randn(3, 4, generator=g)]
    f = ft.features(models, poses, sem, True, torch.zeros(3))
    assert f.shape == (8, 7) and f.dtype == torch.float64
    torch.testing.assert_close(f[:, :3].norm(dim=1), torch.ones(8, dtype=torch.float64))
    assert not f[:5, 3:].any() and torch.equal(f[5:, 3:], sem[1].double())
    assert ft.features(models, poses, None, False).shape == (8, 0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    import torch  # noqa: F401
    l = ctypes.CDLL(LIB)
    for e in ENTRIES:
        getattr(l, e).restype = ctypes.c_int
    l.grpg_last_error.restype = ctypes.c_char_p
    return l


class _Segment(ctypes.Structure):   # grpg_model_segment
    _fields_ = [("xyz", ctypes.c_void_p), ("scaling", ctypes.c_void_p), ("rotation", ctypes.c_void_p),
                ("opacity", ctypes.c_void_p), ("features_dc", ctypes.c_void_p), ("features_rest", ctypes.c_void_p),
                ("count", ctypes.c_int), ("fourier_dim", ctypes.c_int), ("rigid", ctypes.c_int),
                ("obj_rot", ctypes.c_float * 4), ("obj_trans", ctypes.c_float * 3), ("idft", ctypes.c_float * 8),
                ("flip", ctypes.c_void_p)]


def _segment(count=4):
    d = 0x1000   # never dereferenced: every call below is refused before a launch
    return _Segment(d, d, d, d, d, d, count, 1, 0, (ctypes.c_float * 4)(1, 0, 0, 0), (ctypes.c_float * 3)(),
                    (ctypes.c_float * 8)(1), None)


def _calls(lib, seg, nseg, S, normals, campos=None, feats=None):
    """the four entries with the given size arguments; everything else plausible or NULL"""
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ps = ctypes.byref(seg) if seg is not None else None
    return {
        "grpg_compose_features": lambda: lib.grpg_compose_features(ps, I(nseg), None, I(S), I(normals), V(campos), V(feats), None),
        "grpg_compose_features_backward": lambda: lib.grpg_compose_features_backward(
            ps, I(nseg), I(S), I(normals), V(campos), V(feats), None, None, None, None),
        "grpg_forward_composed_features": lambda: lib.grpg_forward_composed_features(
            None, None, None, None, None, None, None, None, ps, I(nseg), None, I(S), I(normals), I(0), I(1), None, I(8),
            I(8), F(1.0), None, None, V(campos), F(1.0), F(1.0), None, None, None, None, None, I(0), None,
            ctypes.c_uint(0)),
        "grpg_backward_composed_features": lambda: lib.grpg_backward_composed_features(
            ps, None, I(nseg), None, I(S), I(normals), I(0), I(1), I(0), None, I(8), I(8), F(1.0), None, None,
            V(campos), F(1.0), F(1.0), None, None, None, None, None, None, None, None, None, None, None, None, None,
            I(0), None),
    }


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_fail_loudly_without_a_device(lib, entry):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    rc = _calls(lib, _segment(), 1, 3, 0)[entry]()
    assert rc == -2, "expected GRPG_ERR_NO_DEVICE, got %d" % rc
    assert b"no usable HIP device" in lib.grpg_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_bad_sizes_and_arguments(lib, entry):
    """every refusal comes before the first launch: the pointers are never read"""
    bad = [
        (_calls(lib, None, 1, 3, 0), b"segments"),                      # no segment table
        (_calls(lib, _segment(), 0, 3, 0), b"segments"),                # no segments
        (_calls(lib, _segment(0), 1, 3, 0), b"count <= 0"),             # an empty segment
        (_calls(lib, _segment(), 1, -1, 0), b"S must be >= 0"),
        (_calls(lib, _segment(), 1, 3, 2), b"normals 0 or 1"),
    ]
    if entry == "grpg_backward_composed_features":
        bad = bad[3:] + [(_calls(lib, _segment(), 1, 33, 0), b"at most 32 semantic channels"),
                         (_calls(lib, _segment(), 1, 30, 1), b"at most 32 semantic channels")]
    if entry in ("grpg_compose_features", "grpg_compose_features_backward"):
        bad.append((_calls(lib, _segment(), 1, 0, 1), b"cam_pos"))      # normals without a camera centre
        bad.append((_calls(lib, _segment(), 1, 3, 0), b"NULL"))         # no feature / gradient array
    for calls, text in bad:
        rc = calls[entry]()
        assert rc == -1, (entry, text, rc, lib.grpg_last_error())
        assert text in lib.grpg_last_error(), (entry, text, lib.grpg_last_error())


def _cpu_models(n=4, dtype=torch.float32):
    from gaussianrpg_amd.composed import ModelParams
    return [ModelParams(torch.zeros(n, 3, dtype=dtype), torch.zeros(n, 3, dtype=dtype), torch.ones(n, 4, dtype=dtype),
                        torch.zeros(n, 1, dtype=dtype), torch.zeros(n, 1, 3, dtype=dtype),
                        torch.zeros(n, 0, 3, dtype=dtype))]


def test_python_api_refuses_cpu_tensors():
    from gaussianrpg_amd.composed import ComposedRasterizer, compose_features, gaussian_normals
    from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                       torch.zeros(3), False, False)
    m = _cpu_models()
    with pytest.raises(RuntimeError, match="no CPU path"):
        compose_features(m, [None], [torch.zeros(4, 3)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ComposedRasterizer(rs).forward_features(m, [None], [torch.zeros(4, 3)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        gaussian_normals(m[0].scaling, m[0].rotation, m[0].xyz, torch.zeros(3))


def test_python_api_refuses_what_it_cannot_run():
    """the checks that come before the device check: they hold on any machine"""
    from gaussianrpg_amd import composed
    assert callable(composed.compose_features) and callable(composed.gaussian_normals)
    assert callable(composed.ComposedRasterizer.forward_features)

    class Dev(torch.Tensor):   # a CPU tensor that claims to live on the device: reaches the later checks
        is_cuda = True

    as_dev = lambda t: t.as_subclass(Dev)   # noqa: E731
    M = composed.ModelParams
    m32 = [M(*(as_dev(t) for t in mm[:6])) for mm in _cpu_models() + _cpu_models(3)]
    m64 = [M(*(as_dev(t) for t in mm[:6])) for mm in _cpu_models(dtype=torch.float64)]
    with pytest.raises(TypeError, match="float32"):
        composed.compose_features(m64, [None])
    with pytest.raises(TypeError, match="float32"):
        composed.compose_features(m32, [None, None], [as_dev(torch.zeros(4, 3, dtype=torch.float16)), None])
    with pytest.raises(ValueError, match="same number of semantic channels"):
        composed.compose_features(m32, [None, None], [as_dev(torch.zeros(4, 3)), as_dev(torch.zeros(3, 5))])
    with pytest.raises(ValueError, match="per model"):
        composed.compose_features(m32, [None, None], [as_dev(torch.zeros(4, 3))])
    with pytest.raises(ValueError, match="needs campos"):
        composed.compose_features(m32, [None, None], None, normals=True)
