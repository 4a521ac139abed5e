"""CPU tests (-m "not gpu") of the object-alpha plane of a training frame: the header declares and the library exports
the three entry points, the size query answers without a device and the calls fail loudly without one, the Python
surface checks its arguments before it touches the device, and -- in float64, on oracle/torch_splat.py -- the formula
the backward kernel implements (csrc/object_alpha.hip),
    dL/dalpha_i = g T_final / (1 - alpha_i),   dL/dG = opacity dL/dalpha,   dL/dopacity = G dL/dalpha,
    dL/dconic and dL/dmean2D as render_bwd.hip forms them (0.5 W / 0.5 H, the xy moment stored at half weight),
equals autograd of the alpha plane."""
import ctypes
import os
import re

import pytest
import torch

from gaussianrpg_amd import harness as hz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussianrpg_amd", "libgrpg_rasterizer.so")
HEADER = os.path.join(ROOT, "include", "grpg_rasterizer.h")
SYMBOLS = ("grpg_object_alpha_workspace_bytes", "grpg_object_alpha_forward", "grpg_backward_composed_objects")
GRPG_ERR_NO_DEVICE = -2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from gaussianrpg_amd import build
        build.build_native()
    lb = ctypes.CDLL(LIB)
    lb.grpg_object_alpha_workspace_bytes.restype = ctypes.c_size_t
    lb.grpg_object_alpha_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    return lb


def test_header_declares_and_library_exports(lib):
    text = open(HEADER).read()
    for s in SYMBOLS:
        assert re.search(r"GRPG_API\s+(int|size_t)\s+%s\(" % s, text), s
        assert hasattr(lib, s), s
    assert re.search(r"#define GRPG_ABI_VERSION 7\b", text)
    lib.grpg_abi_version.restype = ctypes.c_int
    assert lib.grpg_abi_version() == 7


def test_size_query_needs_no_device(lib):
    for W, H in ((160, 96), (200, 136), (1920, 1280), (1, 1)):
        T = ((W + 15) // 16) * ((H + 15) // 16)
        n = lib.grpg_object_alpha_workspace_bytes(W, H)
        assert n >= 4 * W * H + T and n % 256 == 0, (W, H, n)      # n_contrib [N] u32 + one flag byte per tile
        assert n <= 4 * W * H + T + 512
    for W, H in ((0, 96), (160, 0), (-1, 96), (160, -5)):
        assert lib.grpg_object_alpha_workspace_bytes(W, H) == 0


def test_entry_points_fail_without_a_device(lib):
    if torch.cuda.is_available():
        pytest.skip("a device is visible: the no-device answer cannot be observed")
    lib.grpg_object_alpha_forward.restype = ctypes.c_int
    lib.grpg_backward_composed_objects.restype = ctypes.c_int
    lib.grpg_last_error.restype = ctypes.c_char_p
    assert lib.grpg_object_alpha_forward(10, 16, 16, None, None, None, None, None, None, None) == GRPG_ERR_NO_DEVICE
    assert b"no usable HIP device" in lib.grpg_last_error()
    f = ctypes.c_float(1.0)
    rc = lib.grpg_backward_composed_objects(
        None, None, 0, None, 0, 0, 1, 4, 0, None, 16, 16, f, None, None, None, f, f, None, None, None, None, None,
        None, None, None, None, None, None, None, None, None, None, None, 0, None)
    assert rc == GRPG_ERR_NO_DEVICE


def test_forward_objects_checks_object_models_before_the_device():
    from gaussianrpg_amd.composed import ComposedRasterizer, ModelParams
    from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
    cam = hz.trajectory_camera(0, W=48, H=32)
    rast = ComposedRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1)))
    z = lambda *s: torch.zeros(*s)   # noqa: E731
    m = ModelParams(z(5, 3), z(5, 3), z(5, 4), z(5, 1), z(5, 1, 3), z(5, 3, 3))   # CPU tensors: never reach the device
    with pytest.raises(ValueError, match="one flag per model"):
        rast.forward_objects([m, m], [None, None], object_models=[True])
    with pytest.raises(ValueError, match="one flag per model"):
        rast.forward_objects([m], [None], object_models=[True, False, True])
    with pytest.raises(RuntimeError, match="no CPU path"):       # the right length: the models are looked at next
        rast.forward_objects([m, m], [None, None], object_models=[True, False])


def test_formula_equals_autograd_in_float64():
    """48x32, three tiles by two: per pixel and contributing splat, T_final / (1 - alpha_i) times the chain of
    render_bwd.hip, summed per Gaussian, against autograd of sum(g * alpha plane) through oracle/torch_splat.py.
    Opacities stay below 0.99: the clamp never binds, on which the reference's backward and autograd would differ (the
    reference carries no clamp mask, backward.cu:596)."""
    from oracle import torch_splat as ts
    from helpers import oracle_kwargs
    W, H = 48, 32
    sc = hz.toy_scene(400, seed=6, sh_degree=1, depth=6.0, spread=1.2, scale=0.12)
    cam = hz.trajectory_camera(0, W=W, H=H)
    kw = oracle_kwargs(cam, 1, bg=torch.zeros(3))
    kw = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in kw.items()}
    cam_kw = {k: kw[k] for k in ("image_height", "image_width", "tanfovx", "tanfovy", "viewmatrix", "projmatrix",
                                 "campos", "sh_degree", "scale_modifier")}
    pre = ts.preprocess(sc.means3D.double(), sc.opacity.double().clamp(max=0.95), shs=sc.shs.double(),
                        scales=sc.scales.double(), rotations=sc.rotations.double(), **cam_kw)
    binning = ts.bin_tiles(pre)
    leaf = {k: pre[k].detach().clone().requires_grad_(True) for k in ("means2D", "conic", "opacity")}
    out = ts.render_tiles(dict(pre, **leaf), binning, image_height=H, image_width=W, bg=torch.zeros(3).double())
    g = torch.randn(1, H, W, generator=torch.Generator().manual_seed(1)).double()
    (out["alpha"] * g).sum().backward()

    P = sc.means3D.shape[0]
    rec = torch.zeros(P, 16, dtype=torch.float64)      # the gradient record: 0-2 mean2D, 3-5 conic, 9 opacity
    m2, con, op = pre["means2D"], pre["conic"], pre["opacity"]
    gx = (W + 15) // 16
    ncontrib = 0
    for t in range(gx * ((H + 15) // 16)):
        r0, r1 = int(binning["ranges"][t, 0]), int(binning["ranges"][t, 1])
        ty, tx = divmod(t, gx)
        for py in range(ty * 16, min(ty * 16 + 16, H)):
            for px in range(tx * 16, min(tx * 16 + 16, W)):
                ids = binning["point_list"][r0:r1]
                dx, dy = m2[ids, 0] - px, m2[ids, 1] - py
                power = -0.5 * (con[ids, 0] * dx * dx + con[ids, 2] * dy * dy) - con[ids, 1] * dx * dy
                G = torch.exp(power)
                alpha = torch.clamp(op[ids] * G, max=0.99)
                valid = (power <= 0) & (alpha >= 1.0 / 255.0)
                a = torch.where(valid, alpha, torch.zeros_like(alpha))
                contrib = valid & (torch.cumprod(1 - a, 0) >= 0.0001)     # stop before T would fall below 1e-4
                T_final = torch.prod(torch.where(contrib, 1 - a, torch.ones_like(a)))
                dL_dalpha = torch.where(contrib, float(g[0, py, px]) * T_final / (1 - a), torch.zeros_like(a))
                gd = G * dL_dalpha                                         # dL/dopacity
                w = op[ids] * gd                                           # dL/dG G
                tdx, tdy = w * dx, w * dy
                mx = -0.5 * W * (con[ids, 0] * tdx + con[ids, 1] * tdy)
                my = -0.5 * H * (con[ids, 1] * tdx + con[ids, 2] * tdy)
                upd = torch.stack([mx, my, mx.abs() + my.abs(), -0.5 * tdx * dx, -0.5 * tdx * dy, -0.5 * tdy * dy], 1)
                rec[:, 0:6].index_add_(0, ids, upd)
                rec[:, 9].index_add_(0, ids, gd)
                ncontrib += int(contrib.sum())
    assert ncontrib > 2000
    half = torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float64)

    def close(name, got, ref):
        err = float((got - ref).abs().max()) / float(ref.abs().max())
        assert float(ref.abs().max()) > 0 and err <= 1e-10, (name, err)
    close("mean2D", rec[:, 0:2], leaf["means2D"].grad * half)          # the op reports d / d(NDC)
    close("opacity", rec[:, 9], leaf["opacity"].grad)
    close("conic xx", rec[:, 3], leaf["conic"].grad[:, 0])
    close("conic xy", 2.0 * rec[:, 4], leaf["conic"].grad[:, 1])       # stored at half weight (backward.cu:635)
    close("conic yy", rec[:, 5], leaf["conic"].grad[:, 2])
    assert float(rec[:, 2].min()) >= 0.0 and float(rec[:, 2].sum()) > 0
