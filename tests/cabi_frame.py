"""One frame through the C ABI (grpg_forward / grpg_backward via ctypes: no _C, no torch types in the call) -- shared
by tests/test_gpu_cabi_backward.py and tests/test_gpu_preprocess_bwd_truth.py.  Imported by GPU tests only."""
import ctypes

import torch

from gaussianrpg_amd.build import LIB_PATH

ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


def load_lib():
    lb = ctypes.CDLL(LIB_PATH)
    lb.grpg_forward.restype = ctypes.c_int
    lb.grpg_forward_flags.restype = ctypes.c_int
    lb.grpg_backward.restype = ctypes.c_int
    lb.grpg_last_error.restype = ctypes.c_char_p
    return lb


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Frame:
    """One forward through the C ABI; keeps everything the backward needs alive.  scale_modifier goes to the forward
    and the backward alike; campos (default: the camera's) is the point the SH directions are taken from."""

    def __init__(self, lib, dev, sc, cam, colors=None, cov=None, flags=0, scale_modifier=1.0, campos=None):
        self.lib, self.dev = lib, dev
        d = sc.to(dev)
        self.P, self.H, self.W = d.means3D.shape[0], cam.image_height, cam.image_width
        self.M = 0 if colors is not None else d.shs.shape[1]
        self.D = sc.sh_degree
        self.blobs = []

        def alloc(nbytes, _user):
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            self.blobs.append(t)
            return t.data_ptr()
        self.cb = ALLOC(alloc)
        self.bg = torch.tensor([0.2, 0.1, 0.3], device=dev)
        self.view, self.proj = cam.viewmatrix.to(dev), cam.projmatrix.to(dev)
        self.campos = (cam.campos if campos is None else torch.as_tensor(campos)).float().contiguous().to(dev)
        self.tanx, self.tany = ctypes.c_float(cam.tanfovx), ctypes.c_float(cam.tanfovy)
        self.modifier = ctypes.c_float(scale_modifier)
        self.means, self.opac = d.means3D, d.opacity
        self.shs = None if colors is not None else d.shs
        self.colors = None if colors is None else colors.to(dev)
        self.scales = None if cov is not None else d.scales
        self.rots = None if cov is not None else d.rotations
        self.cov = None if cov is None else cov.to(dev)
        self.color = torch.empty(3, self.H, self.W, device=dev)
        self.depth = torch.empty(1, self.H, self.W, device=dev)
        self.alpha = torch.empty(1, self.H, self.W, device=dev)
        self.radii = torch.empty(self.P, dtype=torch.int32, device=dev)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        common = (self.cb, None, self.cb, None, self.cb, None, self.P, self.D, self.M, 0, p(self.bg), self.W,
                  self.H, p(self.means), p(self.shs), p(self.colors), None, p(self.opac), p(self.scales),
                  self.modifier, p(self.rots), p(self.cov), p(self.view), p(self.proj), p(self.campos),
                  self.tanx, self.tany, 0, p(self.color), p(self.depth), p(self.alpha), None, p(self.radii),
                  0, self.stream)
        self.R = lib.grpg_forward_flags(*common, flags) if flags else lib.grpg_forward(*common)
        assert self.R >= 0, lib.grpg_last_error()
        torch.cuda.synchronize()
        # allocation order of the forward: geometry, image, binning (re-carved last after an overflow)
        self.geom, self.image, self.binning = self.blobs[0], self.blobs[1], self.blobs[-1]

    def backward(self, outs, g_color=None):
        """outs: dict name -> tensor or None for the eleven gradient arrays of grpg_backward."""
        gen = torch.Generator().manual_seed(3)
        gc = (torch.randn(3, self.H, self.W, generator=gen) if g_color is None else g_color).to(self.dev)
        gd = torch.randn(1, self.H, self.W, generator=gen).to(self.dev)
        ga = torch.randn(1, self.H, self.W, generator=gen).to(self.dev)
        rc = self.lib.grpg_backward(
            self.P, self.D, self.M, self.R, 0, p(self.bg), self.W, self.H, p(self.means), p(self.shs),
            p(self.colors), None, p(self.alpha), p(self.scales), self.modifier, p(self.rots), p(self.cov),
            p(self.view), p(self.proj), p(self.campos), self.tanx, self.tany, p(self.radii), p(self.geom),
            p(self.binning), p(self.image), p(gc), p(gd), p(ga), None,
            p(outs["mean2D"]), p(outs["conic"]), p(outs["opacity"]), p(outs["color"]), p(outs["depth"]),
            p(outs["mean3D"]), p(outs["cov3D"]), p(outs["sh"]), p(outs["scale"]), p(outs["rot"]), None,
            0, self.stream)
        torch.cuda.synchronize()
        return rc, self.lib.grpg_last_error().decode()


def poisoned(dev, P, M, names):
    shapes = dict(mean2D=(P, 3), conic=(P, 4), opacity=(P, 1), color=(P, 3), depth=(P,), mean3D=(P, 3),
                  cov3D=(P, 6), sh=(P, max(M, 1), 3), scale=(P, 3), rot=(P, 4))
    return {k: (torch.full(shapes[k], float("nan"), device=dev) if k in names else None) for k in shapes}
