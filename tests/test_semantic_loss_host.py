"""CPU tests (-m "not gpu") of the fused semantic cross-entropy loss: the Python surface rejects what it cannot
run (there is no CPU or PyTorch fallback), the float64 statement the GPU tests compare against
(tests/semantic_loss_truth.py) is F.cross_entropy(..., ignore_index=-1) behind the reference's guard, and the C ABI
answers its size query and fails loudly without a device."""
import ctypes
import inspect
import os

import pytest
import torch

import semantic_loss_truth as truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")


def _inputs(S=5, H=7, W=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    sem = torch.randn(S, H, W, generator=g)
    gt = torch.randint(0, S, (H, W), generator=g)
    gt[torch.rand(H, W, generator=g) < 0.2] = -1
    return sem, gt


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    return ctypes.CDLL(LIB)


def test_semantic_loss_rejects_what_it_cannot_run():
    from gaussianrpg_amd import loss
    assert "semantic_loss" in loss.__all__ and "semantic_loss_stats" in loss.__all__
    sem, gt = _inputs()
    for fn in (loss.semantic_loss, loss.semantic_loss_stats):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(sem, gt)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(sem[None], gt[None].int(), mode="probabilities")
        with pytest.raises(TypeError, match="float32"):
            fn(sem.double(), gt)
        with pytest.raises(TypeError, match="int64 or int32"):
            fn(sem, gt.float())
        with pytest.raises(TypeError, match="int64 or int32"):
            fn(sem, gt.to(torch.int16))
        with pytest.raises(ValueError):
            fn(sem, gt[:, :-1])                      # mismatched H x W
        with pytest.raises(ValueError):
            fn(sem, gt.t().contiguous())
        with pytest.raises(ValueError, match="mode"):
            fn(sem, gt, mode="softmax")
        with pytest.raises(ValueError, match="ignore_index"):
            fn(sem, gt, ignore_index=255)
        with pytest.raises(ValueError):
            fn(sem[0], gt)                           # [H,W] planes: no channel axis


@pytest.mark.parametrize("mode", ["logits", "probabilities"])
def test_truth_is_cross_entropy_with_ignore_index(mode):
    sem, gt = _inputs(S=6, H=11, W=13, seed=3)
    if mode == "probabilities":
        sem = sem.abs() + 0.01
    x = sem.double().clone().requires_grad_(True)
    v = truth.loss64(x, gt, mode)
    v.backward()
    y = sem.double().clone().requires_grad_(True)
    inp = y if mode == "logits" else torch.log(y / (y.sum(0, keepdim=True) + 1e-8) + 1e-8)
    ref = torch.nn.functional.cross_entropy(inp[None], gt[None], ignore_index=-1, reduction="mean")
    ref.backward()
    assert v.dtype == torch.float64 and float(v.detach()) == float(ref.detach())
    assert torch.equal(x.grad, y.grad)
    # the definition, written out: mean over the valid pixels of logsumexp - x_target
    ref = ref.detach()
    assert abs(float(truth.manual64(sem, gt, mode)) - float(ref)) <= 1e-13 * abs(float(ref))
    # [1,S,H,W] planes with [1,H,W] labels, int32 labels
    assert float(truth.loss64(sem[None], gt[None].int(), mode)) == float(ref)
    # float32: the reference's own arithmetic, a few ulp from float64
    assert abs(float(truth.loss32(sem, gt, mode)) - float(ref)) <= 1e-6 * abs(float(ref))


def test_truth_guard_and_bad_labels():
    sem, gt = _inputs()
    x = sem.double().requires_grad_(True)
    v = truth.loss64(x, torch.full_like(gt, -1))
    v.backward()
    assert float(v.detach()) == 0.0 and float(x.grad.abs().max()) == 0.0 # exactly 0, zero gradient
    assert float(truth.loss32(sem, torch.full_like(gt, -1), "probabilities")) == 0.0
    # labels outside [-1, S) are ignored like -1
    bad = gt.clone()
    bad[0, 0], bad[1, 2] = -7, sem.shape[0] + 3
    ign = gt.clone()
    ign[0, 0], ign[1, 2] = -1, -1
    assert float(truth.loss64(sem, bad)) == float(truth.loss64(sem, ign))
    n_valid, n_bad, n_correct, labels = truth.counts(sem, bad)
    assert n_bad == 2 and n_valid == int((ign >= 0).sum())
    assert n_correct == int(((sem.argmax(0) == ign) & (ign >= 0)).sum()) and labels.shape == gt.shape


def test_workspace_size_query_needs_no_device(lib):
    lib.grpg_semantic_ce_workspace_bytes.restype = ctypes.c_size_t
    lib.grpg_semantic_ce_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    n = lib.grpg_semantic_ce_workspace_bytes(37, 53)
    assert n >= 4 * 37 * 53                                              # the per-pixel logsumexp plane
    assert n < 4 * 37 * 53 + (1 << 16)                                   # plus a bounded header
    assert lib.grpg_semantic_ce_workspace_bytes(0, 53) == 0
    assert lib.grpg_semantic_ce_workspace_bytes(1280, 1920) >= 4 * 1280 * 1920


def test_entry_points_fail_loudly_without_a_device(lib):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    lib.grpg_last_error.restype = ctypes.c_char_p
    lib.grpg_semantic_ce_forward.restype = ctypes.c_int
    lib.grpg_semantic_ce_backward.restype = ctypes.c_int
    assert lib.grpg_semantic_ce_forward(3, 4, 4, None, None, 8, 0, None, None, None, None) == -2
    assert b"no usable HIP device" in lib.grpg_last_error()
    assert lib.grpg_semantic_ce_backward(3, 4, 4, None, None, 8, 0, None, None, None, None) == -2


def test_binding_exposes_the_entry_points():
    from gaussianrpg_amd.rasterizer import _C
    assert hasattr(_C, "semantic_ce_forward") and hasattr(_C, "semantic_ce_backward")
    sem, gt = _inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.semantic_ce_forward(sem, gt, 0, False)


def test_train_loss_accepts_the_semantic_keywords():
    from gaussianrpg_amd import harness as hz
    p = inspect.signature(hz.train_loss).parameters
    assert p["gt_semantic"].default is None
    assert p["lambda_semantic"].default == 0.0
    assert p["semantic_mode"].default == "logits"
    assert "SSIM, semantic and the regularisers" not in hz.train_loss.__doc__       # no longer listed as not fused
    # the defaults, and a lambda of 0, leave the result as it is (CPU tensors: the PyTorch terms only)
    g = torch.Generator().manual_seed(1)
    pkg = {"rgb": torch.rand(3, 6, 8, generator=g), "acc": torch.rand(1, 6, 8, generator=g) * 0.9 + 0.05,
           "depth": torch.rand(1, 6, 8, generator=g) * 10, "semantic": torch.rand(4, 6, 8, generator=g)}
    gt_img = torch.rand(3, 6, 8, generator=g)
    sky = torch.rand(1, 6, 8, generator=g) < 0.3
    gt_sem = torch.randint(-1, 4, (1, 6, 8), generator=g)
    base = hz.train_loss(pkg, gt_img, sky_mask=sky)
    assert torch.equal(base, hz.train_loss(pkg, gt_img, sky_mask=sky, gt_semantic=gt_sem, lambda_semantic=0.0))
    assert torch.equal(base, hz.train_loss(pkg, gt_img, sky_mask=sky, lambda_semantic=0.1))          # no labels
    with pytest.raises(RuntimeError, match="no CPU path"):                                           # no fallback
        hz.train_loss(pkg, gt_img, sky_mask=sky, gt_semantic=gt_sem, lambda_semantic=0.1)
