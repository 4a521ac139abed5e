"""CPU tests (-m "not gpu") of the fused SSIM + L1 loss (gaussianrpg_amd/loss.py, csrc/ssim.hip):
the tests' float64 statement of loss_utils (tests/ssim_truth.py) reproduces the reference's own
float64 run pinned in tests/golden/ref_ssim.npz, the module and the C entries exist and fail loudly
without a device, and the wrapper rejects what it does not support."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ssim_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_ssim.npz"))
    return {k: z[k] for k in z.files}


def _case(g, name):
    a = torch.from_numpy(g[name + "/img1"])
    b = torch.from_numpy(g[name + "/img2"])
    m = torch.from_numpy(g[name + "/mask"]) if name + "/mask" in g else None
    return a, b, m


def _rel(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def test_truth_reproduces_the_reference_values(golden):
    for name in golden["names"]:
        a, b, m = _case(golden, str(name))
        assert abs(float(ssim_truth.ssim(a, b, mask=m)) - float(golden[name + "/ssim"])) < 1e-12, name
        if name + "/ssim_per_image" in golden:
            np.testing.assert_allclose(ssim_truth.ssim(a, b, size_average=False, mask=m).numpy(),
                                       golden[name + "/ssim_per_image"], rtol=0, atol=1e-12)
        if name + "/l1" in golden:
            assert abs(float(ssim_truth.l1(a, b, m)) - float(golden[name + "/l1"])) < 1e-12, name
            assert abs(float(ssim_truth.mix(a, b, m)) - float(golden[name + "/mix"])) < 1e-12, name


def test_truth_reproduces_the_reference_gradients(golden):
    for name in golden["names"]:
        a, b, m = _case(golden, str(name))
        t = a.clone().requires_grad_(True)
        ssim_truth.ssim(t, b, mask=m).backward()
        assert _rel(t.grad.numpy(), golden[name + "/grad_ssim"]) < 1e-10, name
        if name + "/grad_l1" in golden:
            t = a.clone().requires_grad_(True)
            ssim_truth.l1(t, b, m).backward()
            assert _rel(t.grad.numpy(), golden[name + "/grad_l1"]) < 1e-10, name
            t = a.clone().requires_grad_(True)
            ssim_truth.mix(t, b, m).backward()
            assert _rel(t.grad.numpy(), golden[name + "/grad_mix"]) < 1e-10, name


def test_golden_covers_the_required_shapes(golden):
    shapes = {tuple(golden[str(n) + "/img1"].shape) for n in golden["names"]}
    assert {(3, 37, 53), (3, 5, 7), (2, 3, 20, 30), (3, 1, 1)} <= shapes
    assert any(str(n) + "/mask" in golden for n in golden["names"])


def test_loss_module_imports():
    from gaussianrpg_amd import loss
    for name in ("ssim", "l1_loss", "l1_ssim_loss"):
        assert callable(getattr(loss, name))
    from gaussianrpg_amd.rasterizer import _C
    assert hasattr(_C, "ssim_forward") and hasattr(_C, "ssim_backward")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    return ctypes.CDLL(LIB)


def test_c_entries_fail_loudly_without_a_device(lib):
    lib.grpg_ssim_workspace_bytes.restype = ctypes.c_size_t
    assert lib.grpg_ssim_workspace_bytes(1, 3, 1280, 1920) >= 3 * 8 * 3 * 40 * 80   # pure size query
    assert lib.grpg_ssim_workspace_bytes(1, 3, 0, 1920) == 0
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib.grpg_ssim_forward.restype = ctypes.c_int
    lib.grpg_ssim_backward.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    f = ctypes.c_float
    assert lib.grpg_ssim_forward(1, 3, 8, 8, None, None, None, 1, 1, f(0.8), f(0.2), None, None, None,
                                 None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_ssim_backward(1, 3, 8, 8, None, None, None, 1, 1, f(0.8), f(0.2), None, None, None,
                                  None, None) == -2


def test_wrapper_rejects_unsupported_inputs():
    from gaussianrpg_amd import loss
    a = torch.rand(3, 8, 9)
    b = torch.rand(3, 8, 9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.ssim(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.l1_loss(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.l1_ssim_loss(a, b)
    with pytest.raises(TypeError, match="float32"):
        loss.ssim(a.double(), b.double())
    with pytest.raises(TypeError, match="float32"):
        loss.l1_ssim_loss(a, b.double())
    with pytest.raises(ValueError, match="window_size == 11"):
        loss.ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="gt requires a gradient"):
        loss.l1_ssim_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="img2 requires a gradient"):
        loss.ssim(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="same shape"):
        loss.ssim(a, torch.rand(3, 8, 10))
    with pytest.raises(ValueError, match="same shape"):
        loss.l1_loss(a, torch.rand(1, 3, 8, 9))
