"""GPU tests of the fused semantic cross-entropy loss (gaussianrpg_amd/loss.py, csrc/semantic_loss.hip) against the
float64 statement of train.py:129-143 (tests/semantic_loss_truth.py) and against the same code run in float32
PyTorch on the device (the reference's own arithmetic).

Bars (those of tests/test_gpu_aux_loss.py): the value within 1e-6 relative of float64 and no further from it than
twice the float32 PyTorch path plus 3e-7 relative; the gradient within relative L2 1e-5 of float64 autograd; the
counts and the label plane exact.  Float32 PyTorch itself sits at <= 1.2e-7 (value) and <= 9e-8 (gradient) from
float64 on these shapes."""
import ctypes
import math
import os

import pytest
import torch

import semantic_loss_truth as truth
from gaussianrpg_amd import harness as hz

pytestmark = pytest.mark.gpu

VAL_REL = 1e-6
VAL_FLOOR = 3e-7      # relative: a few ulp of a float32
GRAD_REL = 1e-5
MODES = ["logits", "probabilities"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _inputs(S, H, W, mode, dev, seed=0, ignored=0.2, scale=1.0):
    """Planes without exact ties (continuous random values) and labels with 20 % of -1."""
    g = torch.Generator().manual_seed(1000 * S + H + seed)
    if mode == "logits":
        sem = torch.randn(S, H, W, generator=g) * scale
    else:
        sem = (torch.rand(S, H, W, generator=g) * 0.98 + 0.01) * scale     # rendered probabilities: positive
    gt = torch.randint(0, S, (H, W), generator=g)
    gt[torch.rand(H, W, generator=g) < ignored] = -1
    return sem.to(dev), gt.to(dev)


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def _val_ok(v, v64, v32, what):
    v, v64, v32 = float(v), float(v64), float(v32)
    e, e32 = abs(v - v64), abs(v32 - v64)
    scale = max(abs(v64), 1e-30)
    print("%s: value %.9g float64 %.9g rel err %.3g (float32 torch %.3g)" % (what, v, v64, e / scale, e32 / scale))
    assert math.isfinite(v), (what, v)
    assert e <= VAL_REL * scale, (what, v, v64)
    assert e <= 2 * e32 + VAL_FLOOR * scale, (what, e, e32)


def _grad_ok(g, g64, what):
    assert bool(torch.isfinite(g).all()), what
    if float(g64.double().abs().max()) == 0.0:
        assert float(g.abs().max()) == 0.0, what
    else:
        print("%s: gradient rel L2 %.3g" % (what, _rel(g, g64)))
        assert _rel(g, g64) < GRAD_REL, (what, _rel(g, g64))


def _fused(sem, gt, mode):
    from gaussianrpg_amd import loss
    x = sem.clone().requires_grad_(True)
    v = loss.semantic_loss(x, gt, mode=mode)
    v.backward()
    return v.detach(), x.grad


def _check(sem, gt, mode, what):
    v, g = _fused(sem, gt, mode)
    x64 = sem.double().requires_grad_(True)
    v64 = truth.loss64(x64, gt, mode)
    v64.backward()
    v32 = truth.loss32(sem, gt, mode)
    assert v.shape == () and v.dtype == torch.float32 and g.shape == sem.shape
    _val_ok(v, v64.detach(), v32, what)
    _grad_ok(g, x64.grad, what)
    return v, g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [1, 3, 19, 32, 40])
def test_value_and_gradient_37x53(dev, S, mode):
    """H*W odd, a partial last wave and a partial last workgroup; S on each register path and past it."""
    sem, gt = _inputs(S, 37, 53, mode, dev)
    v, g = _check(sem, gt, mode, "S=%d %s" % (S, mode))
    if S == 1:
        assert float(v) == 0.0 and float(g.abs().max()) == 0.0
    assert float(g[:, gt == -1].abs().max()) == 0.0          # ignored pixels: exactly 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,H,W", [(19, 64, 64), (8, 96, 200), (15, 96, 200)])
def test_value_and_gradient_other_shapes(dev, S, H, W, mode):
    """64x64: whole workgroups only; 96x200: 75 workgroups of partial sums."""
    sem, gt = _inputs(S, H, W, mode, dev, seed=5)
    _check(sem, gt, mode, "S=%d %dx%d %s" % (S, H, W, mode))


@pytest.mark.parametrize("mode", MODES)
def test_every_target_ignored(dev, mode):
    from gaussianrpg_amd import loss
    sem, gt = _inputs(19, 37, 53, mode, dev)
    gt = torch.full_like(gt, -1)
    v, g = _fused(sem, gt, mode)
    assert float(v) == 0.0 and float(g.abs().max()) == 0.0 and not bool(torch.isnan(g).any())
    s = loss.semantic_loss_stats(sem, gt, mode=mode)
    assert int(s["n_valid"]) == 0 and int(s["n_bad"]) == 0 and int(s["n_correct"]) == 0 and float(s["loss"]) == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_single_valid_pixel(dev, mode):
    sem, gt = _inputs(19, 37, 53, mode, dev)
    one = torch.full_like(gt, -1)
    one[20, 31] = 7
    v, g = _check(sem, one, mode, "single pixel %s" % mode)
    keep = torch.zeros_like(one, dtype=torch.bool)
    keep[20, 31] = True
    assert float(g[:, ~keep].abs().max()) == 0.0 and float(g[:, keep].abs().max()) > 0.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,H,W", [(3, 37, 53), (19, 37, 53), (40, 37, 53), (15, 96, 200), (3, 520, 520)])
def test_counts_and_labels_are_exact(dev, S, H, W, mode):
    """520x520: 1057 workgroups, so the first threads of the one-workgroup reduce add two slots each."""
    from gaussianrpg_amd import loss
    sem, gt = _inputs(S, H, W, mode, dev, seed=9)
    gt[3, 4], gt[H - 1, W - 1], gt[0, 0] = -7, S + 3, -(2 ** 40)       # bad labels: counted, ignored, no fault
    s = loss.semantic_loss_stats(sem, gt, mode=mode)
    n_valid, n_bad, n_correct, labels = truth.counts(sem, gt)
    assert n_bad == 3
    assert (int(s["n_valid"]), int(s["n_bad"]), int(s["n_correct"])) == (n_valid, n_bad, n_correct)
    assert s["n_valid"].dtype == torch.int64
    assert s["labels"].dtype == torch.uint8 and s["labels"].shape == (H, W)
    assert torch.equal(s["labels"].long(), labels)
    assert not s["loss"].requires_grad
    # the bad labels are ignored: the value and the gradient of the sanitized labels
    v, g = _check(sem, gt, mode, "bad labels S=%d %s" % (S, mode))
    assert float(s["loss"]) == float(v)
    for y, x in ((3, 4), (H - 1, W - 1), (0, 0)):
        assert float(g[:, y, x].abs().max()) == 0.0


def test_constructed_tie_goes_to_the_lowest_channel(dev):
    from gaussianrpg_amd import loss
    sem, gt = _inputs(19, 37, 53, "logits", dev, seed=2)
    sem[4, 10, 10] = sem[11, 10, 10] = sem[17, 10, 10] = float(sem[:, 10, 10].max()) + 1.0
    gt[10, 10] = 4
    sem[:, 11, 11] = 0.25                                    # every channel ties: channel 0
    gt[11, 11] = 0
    s = loss.semantic_loss_stats(sem, gt)
    n_valid, n_bad, n_correct, labels = truth.counts(sem, gt)
    assert int(labels[10, 10]) == 4 and int(labels[11, 11]) == 0          # torch.argmax on these inputs
    assert torch.equal(s["labels"].long(), labels) and int(s["n_correct"]) == n_correct


def test_no_label_plane_past_256_channels(dev):
    from gaussianrpg_amd import loss
    sem, gt = _inputs(300, 8, 9, "logits", dev)
    s = loss.semantic_loss_stats(sem, gt)
    assert "labels" not in s
    n_valid, n_bad, n_correct, _ = truth.counts(sem, gt)
    assert (int(s["n_valid"]), int(s["n_bad"]), int(s["n_correct"])) == (n_valid, n_bad, n_correct)
    _check(sem, gt, "logits", "S=300")


@pytest.mark.parametrize("S", [19, 40])
def test_large_logits_do_not_overflow(dev, S):
    sem, gt = _inputs(S, 37, 53, "logits", dev, seed=4, scale=30.0)
    sem[:, 5, 6] = 0.0
    sem[2, 5, 6], sem[S - 1, 5, 6] = 1e4, -1e4
    gt[5, 6] = S - 1                                          # a loss of 2e4 at this pixel
    sem[:, 7, 8] = 0.0
    sem[S - 2, 7, 8], sem[0, 7, 8] = 1e4, -1e4
    gt[7, 8] = S - 2                                          # and one of 0
    _check(sem, gt, "logits", "30x logits S=%d" % S)


NINF = float("-inf")
MINUS_INF_PIXELS = {"ninf_ninf_0": (NINF, NINF, 0.0), "ninf_0_ninf": (NINF, 0.0, NINF), "0_ninf_ninf": (0.0, NINF, NINF),
                    "all_ninf": (NINF, NINF, NINF)}


@pytest.mark.parametrize("name", list(MINUS_INF_PIXELS))
@pytest.mark.parametrize("S", [3, 40])
def test_minus_inf_logits(dev, S, name):
    """A channel at -inf has probability 0: the log-sum-exp of (-inf, -inf, 0) is 0, not exp(-inf - -inf) = NaN.
    One pixel at a time (every other label -1), each target 0..2, in the register form (S = 3) and the memory form
    (S = 40, the further channels -inf): the loss is finite and inside the file's bars where float64 F.cross_entropy
    is finite, +inf where it is +inf (the target itself at -inf), NaN where it is NaN (every channel -inf); the
    gradient is exactly 0 at every -inf channel where the truth's is."""
    H, W = 3, 5
    sem = torch.full((S, H, W), NINF, device=dev)
    sem[:3] = torch.randn(3, H, W, generator=torch.Generator().manual_seed(S)).to(dev)
    sem[:3, 1, 2] = torch.tensor(MINUS_INF_PIXELS[name], device=dev)
    for t in range(3):
        what = "%s target %d S=%d" % (name, t, S)
        gt = torch.full((H, W), -1, dtype=torch.int64, device=dev)
        gt[1, 2] = t
        v, g = _fused(sem, gt, "logits")
        x64 = sem.double().requires_grad_(True)
        v64 = truth.loss64(x64, gt, "logits")
        v64.backward()
        v64, g64 = float(v64.detach()), x64.grad
        print("%s: value %r float64 %r" % (what, float(v), v64))
        if math.isfinite(v64):
            _val_ok(v, v64, truth.loss32(sem, gt, "logits"), what)
        elif math.isnan(v64):
            assert math.isnan(float(v)), (what, float(v))
        else:
            assert float(v) == v64, (what, float(v), v64)
        assert torch.equal(torch.isnan(g).cpu(), torch.isnan(g64).cpu()), what
        zero = (sem == NINF) & (g64 == 0)
        assert bool((g[zero] == 0).all()), what
        if bool(torch.isfinite(g64).all()):
            _grad_ok(g, g64, what)
    # among ordinary pixels: the three patterns whose target holds the 0 join a mean of finite losses
    if name != "all_ninf":
        gt = torch.randint(0, 3, (H, W), generator=torch.Generator().manual_seed(S + 1)).to(dev)
        gt[1, 2] = MINUS_INF_PIXELS[name].index(0.0)
        _check(sem, gt, "logits", "%s among finite pixels S=%d" % (name, S))


@pytest.mark.parametrize("S", [3, 19, 40])
def test_probabilities_edge_inputs_stay_finite(dev, S):
    from gaussianrpg_amd import loss
    sem, gt = _inputs(S, 37, 53, "probabilities", dev, seed=6)
    sem[:, 9, 9] = 0.0                                        # nothing rendered here: a uniform prediction
    gt[9, 9] = S - 1
    only = torch.full_like(gt, -1)
    only[9, 9] = S - 1
    v, g = _fused(sem, only, "probabilities")
    assert bool(torch.isfinite(g).all())
    assert abs(float(v) - math.log(S)) <= 1e-6 * max(math.log(S), 1.0)
    _check(sem, gt, "probabilities", "zero pixel S=%d" % S)
    small, gt2 = _inputs(S, 37, 53, "probabilities", dev, seed=7, scale=1e-3)
    _check(small, gt2, "probabilities", "1e-3 planes S=%d" % S)
    assert math.isfinite(float(loss.semantic_loss_stats(small, gt2, mode="probabilities")["loss"]))


@pytest.mark.parametrize("mode", MODES)
def test_layouts(dev, mode):
    sem, gt = _inputs(19, 37, 53, mode, dev, seed=8)
    v, g = _fused(sem, gt, mode)
    # [1,S,H,W] planes with [1,H,W] labels
    v4, g4 = _fused(sem[None], gt[None], mode)
    assert g4.shape == (1, 19, 37, 53) and torch.equal(v4, v) and torch.equal(g4[0], g)
    # a permuted view ([H,W,S] memory)
    hwc = sem.permute(1, 2, 0).contiguous()
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous()
    vp, gp = _fused(view, gt, mode)
    assert torch.equal(vp, v) and torch.equal(gp, g)
    # int32 labels
    vi, gi = _fused(sem, gt.int(), mode)
    assert torch.equal(vi, v) and torch.equal(gi, g)
    # planes one float off their allocation: the bits of the aligned copy
    buf = torch.empty(sem.numel() + 1, device=dev)
    off = buf[1:].view(sem.shape)
    off.copy_(sem)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    vo, go = _fused(off, gt, mode)
    assert torch.equal(vo, v) and torch.equal(go, g)


@pytest.mark.parametrize("mode", MODES)
def test_identical_calls_give_identical_bits(dev, mode):
    from gaussianrpg_amd import loss
    sem, gt = _inputs(15, 96, 200, mode, dev, seed=3)
    v1, g1 = _fused(sem, gt, mode)
    v2, g2 = _fused(sem, gt, mode)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    # one forward, its backward twice
    x = sem.clone().requires_grad_(True)
    v = loss.semantic_loss(x, gt, mode=mode)
    (ga,) = torch.autograd.grad(v, x, retain_graph=True)
    (gb,) = torch.autograd.grad(v, x)
    assert torch.equal(ga, gb) and torch.equal(ga, g1)
    # an upstream factor arrives on the device
    x = sem.clone().requires_grad_(True)
    (0.25 * loss.semantic_loss(x, gt, mode=mode)).backward()
    assert _rel(x.grad, 0.25 * g1.double()) < 1e-6


@pytest.mark.parametrize("mode", [0, 1])
def test_backward_overwrites_a_poisoned_buffer(dev, mode):
    from gaussianrpg_amd.rasterizer import _C
    name = MODES[mode]
    sem, gt = _inputs(19, 37, 53, name, dev, seed=1)
    gt[2, 2] = 25                                             # a bad pixel among the valid and the ignored
    _, ref = _fused(sem, gt, name)
    stats, ws, _ = _C.semantic_ce_forward(sem, gt, mode, False)
    out = torch.full_like(sem, float("nan"))
    g = _C.semantic_ce_backward(sem, gt, mode, torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev), ws, out)
    assert g.data_ptr() == out.data_ptr()
    assert not bool(torch.isnan(out).any()) and torch.equal(out, ref)
    # all ignored: a poisoned buffer becomes exactly 0
    none = torch.full_like(gt, -1)
    stats, ws, _ = _C.semantic_ce_forward(sem, none, mode, False)
    out = torch.full_like(sem, float("nan"))
    _C.semantic_ce_backward(sem, none, mode, torch.ones(4, device=dev), ws, out)
    assert float(out.abs().max()) == 0.0


def test_c_abi_rejects_bad_arguments(dev):
    torch.zeros(1, device=dev)                                # the device is up
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so"))
    fwd = lib.grpg_semantic_ce_forward
    fwd.restype = ctypes.c_int
    fwd.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 4
    sem, gt = _inputs(3, 8, 8, "logits", dev)
    stats = torch.zeros(4, device=dev)
    lib.grpg_semantic_ce_workspace_bytes.restype = ctypes.c_size_t
    ws = torch.zeros(lib.grpg_semantic_ce_workspace_bytes(8, 8), dtype=torch.uint8, device=dev)
    ok = (3, 8, 8, sem.data_ptr(), gt.data_ptr(), 8, 0, stats.data_ptr(), None, ws.data_ptr(), None)
    for i, bad in ((0, 0), (3, None), (4, None), (5, 2), (6, 2)):      # S < 1, NULL sem / target, width, mode
        args = list(ok)
        args[i] = bad
        assert fwd(*args) == -1, i
    torch.cuda.synchronize()


def test_end_to_end_through_the_rasterizer(dev):
    """The per-Gaussian semantic gradients of a small scene: fused loss against F.cross_entropy on the same planes."""
    from gaussianrpg_amd import loss
    P, S = 2000, 3
    sc = hz.toy_scene(P=P, seed=3).to(dev)
    cam = hz.trajectory_camera(0, W=64, H=48, device=dev)
    g = torch.Generator().manual_seed(11)
    sem_p = torch.randn(P, S, generator=g).to(dev)
    gt = torch.randint(0, S, (48, 64), generator=g)
    gt[torch.rand(48, 64, generator=g) < 0.2] = -1
    gt = gt.to(dev)
    grads = []
    for fn in (lambda planes: loss.semantic_loss(planes, gt[None]),
               lambda planes: torch.nn.functional.cross_entropy(planes[None], gt[None], ignore_index=-1)):
        leaf = sem_p.clone().requires_grad_(True)
        pkg = hz.render_kernel(sc, cam, mode="train", semantics=leaf)
        assert pkg["semantic"].shape == (S, 48, 64)
        fn(pkg["semantic"]).backward()
        grads.append(leaf.grad.clone())
    assert float(grads[1].abs().max()) > 0.0
    print("end to end: per-Gaussian semantic gradient rel L2 %.3g" % _rel(grads[0], grads[1]))
    assert _rel(grads[0], grads[1]) < GRAD_REL


def test_train_loss_with_and_without_the_semantic_term(dev):
    from gaussianrpg_amd import loss
    g = torch.Generator().manual_seed(2)
    H, W, S = 37, 53, 5
    pkg = {"rgb": torch.rand(3, H, W, generator=g).to(dev), "acc": (torch.rand(1, H, W, generator=g) * 0.9 + 0.05).to(dev),
           "depth": (torch.rand(1, H, W, generator=g) * 20).to(dev), "semantic": torch.randn(S, H, W, generator=g).to(dev)}
    gt_img = torch.rand(3, H, W, generator=g).to(dev)
    sky = (torch.rand(1, H, W, generator=g) < 0.3).to(dev)
    lidar = (torch.rand(1, H, W, generator=g) * 30).to(dev)
    gt_sem = torch.randint(-1, S, (1, H, W), generator=g).to(dev)
    for kw in (dict(), dict(fused_aux=True), dict(lambda_dssim=0.2)):
        base = hz.train_loss(pkg, gt_img, lidar, sky, **kw)
        same = hz.train_loss(pkg, gt_img, lidar, sky, gt_semantic=gt_sem, lambda_semantic=0, **kw)
        assert torch.equal(base, same)                        # bit-identical
        full = hz.train_loss(pkg, gt_img, lidar, sky, gt_semantic=gt_sem, lambda_semantic=0.1, **kw)
        assert torch.equal(full, base + 0.1 * loss.semantic_loss(pkg["semantic"], gt_sem))
    p = dict(pkg, semantic=pkg["semantic"].abs() + 0.01)
    full = hz.train_loss(p, gt_img, lidar, sky, gt_semantic=gt_sem, lambda_semantic=0.1, semantic_mode="probabilities")
    assert torch.equal(full, hz.train_loss(p, gt_img, lidar, sky)
                       + 0.1 * loss.semantic_loss(p["semantic"], gt_sem, mode="probabilities"))
