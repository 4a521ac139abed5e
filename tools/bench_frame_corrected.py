"""The corrected simulator frame (a scene trained with use_color_correction) at 1920x1280 on the bench scene with a
1024^2 sky: the colour correction inside the one-call frame's epilogue (forward_frame(..., affine=A)) against the route
it replaces, timed on the same GPU in ONE process, alternating batch by batch.

Corrected frame, "host" -- the bytes in pinned host memory, what the simulator consumes:
  (a) chain     forward_frame(planes=True, rgb8=False, sky_cube=None) + appearance.corrected_frame's launch + the copy
                of the bytes into a pinned tensor
  (b) one_call  forward_frame(..., affine=A, out=pinned)
and "device" -- the bytes in device memory: (a) without the copy, (b) with a device ``out``.

Uncorrected frame (forward_frame without affine, device bytes and pinned host), this tree's library against the PARENT
commit's, both driven through the C ABI (ctypes) with the same arguments:
  python tools/build_lib_from_commit.py HEAD~1 parent          (then a copy of the file as ..._parent_b.so)
  --parent build/variants/libgrpg_rasterizer_parent.so --parent-b build/variants/libgrpg_rasterizer_parent_b.so
The second copy gives the spread parent-against-parent shows in the very same job; the run-time branch of the epilogue
costs nothing when this-against-parent lies inside it.

Per route: the wall time per frame of a batch of --inner back-to-back frames between two synchronises; median over
--batches batches after --warmup batches, --reps times with their min - max.  Prints one JSON line; --out FILE also
writes it (profiles/frame_corrected_bench.json)."""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import benchkit
from benchkit import column, median
from gaussianrpg_amd import build, harness
from gaussianrpg_amd.rasterizer import _C
from gaussianrpg_amd.sky import SkyCubeMap, ray_matrix

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=30)
ap.add_argument("--height", type=int, default=1280)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--gaussians", type=int, default=2_000_000)
ap.add_argument("--sky-res", type=int, default=1024)
ap.add_argument("--parent", default=None, help="the parent commit's library (tools/build_lib_from_commit.py)")
ap.add_argument("--parent-b", default=None, help="a second copy of it (another file): the job's own spread")
ap.add_argument("--lib-order", default="this,parent,parent_b",
                help="the order in which the three libraries take their batches (a place in the order has a cost of its own)")
ap.add_argument("--skip-corrected", action="store_true", help="only the uncorrected A/B")
args = ap.parse_args()

benchkit.require_gpu("bench_frame_corrected")
dev = torch.device("cuda:0")
H, W = args.height, args.width


def measure(routes):
    """{route: {"us", "repetitions_us", "min_us", "max_us"}}; the routes alternate batch by batch; wall us per frame of
    args.inner back-to-back frames"""
    reps = {k: [] for k in routes}
    for _ in range(args.reps):
        seen = benchkit.alternating(routes, args.batches, args.warmup, inner=args.inner, events=False)
        for k in routes:
            reps[k].append(median(column(seen[k], "wall_us")))
    return {k: {"us": median(v), "repetitions_us": v, "min_us": min(v), "max_us": max(v)} for k, v in reps.items()}


from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
g = torch.Generator().manual_seed(H + W)
scene = harness.street_scene(args.gaussians, seed=2, sh_degree=1).to(dev)
cam = harness.trajectory_camera(0, W=W, H=H, device=dev)
K = torch.tensor([[harness.WAYMO_FX, 0.0, W / 2.0], [0.0, harness.WAYMO_FY, H / 2.0], [0.0, 0.0, 1.0]]).to(dev)
w2c = cam.viewmatrix.transpose(0, 1).contiguous()
sky = SkyCubeMap(args.sky_res, mode="evaluate").to(dev)
with torch.no_grad():
    sky.sky_cube_map.copy_((torch.rand(6, args.sky_res, args.sky_res, 3, generator=g) * 1.3 - 0.15).to(dev))
rm = ray_matrix(K, w2c)          # once: the camera is fixed; both routes take the same device matrix
affine = (torch.eye(4)[:3] + 0.1 * (torch.rand(3, 4, generator=g) - 0.5)).to(dev)
bg = torch.zeros(3, device=dev)
rast = GaussianRasterizer(GaussianRasterizationSettings(**harness.settings_kwargs(cam, scene.sh_degree, bg=bg)))
kw = dict(shs=scene.shs, scales=scene.scales, rotations=scene.rotations)
e = dict(sky_cube=sky.sky_cube_map, ray_matrix=rm)
pinned_a = torch.empty((H, W, 3), dtype=torch.uint8).pin_memory()
pinned_b = torch.empty((H, W, 3), dtype=torch.uint8).pin_memory()
dev_a = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
dev_b = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)


def chain(host):
    def run():
        with torch.no_grad():
            o = rast.forward_frame(scene.means3D, scene.opacity, planes=True, rgb8=False, sky_cube=None, clamp=True, **kw)
            # appearance.corrected_frame's launch, with the ray matrix both routes share (corrected_frame itself forms
            # it from K / w2c on every call: a dozen small launches that would count against this route alone)
            _C.color_correct(o["rgb"], affine, clamp=True, planes=False, rgb8=True, truncate=True, out=dev_a,
                             cube=sky.sky_cube_map, ray_matrix=rm, fill=sky.fill, acc=o["alpha"])
            if host:
                pinned_a.copy_(dev_a, non_blocking=True)
    return run


def one_call(out):
    def run():
        with torch.no_grad():
            rast.forward_frame(scene.means3D, scene.opacity, affine=affine, out=out, **kw, **e)
    return run


result = {"what": "corrected simulator frame at %dx%d, bench scene (P = %d), sky %d^2; us per frame: per route the median "
                  "over %d repetitions of (median over %d batches of %d back-to-back frames between two synchronises, "
                  "after %d warm-up batches), with the repetitions' min - max; routes alternate batch by batch in one "
                  "process" % (W, H, int(scene.means3D.shape[0]), args.sky_res, args.reps, args.batches, args.inner,
                               args.warmup),
          "device": torch.cuda.get_device_name(0),
          "kernel_resources": {k: v for k, v in build.kernel_resources("render_fwd.hip").items()
                               if "render_forward_kernel" in k} if os.path.exists(build.remarks_path("render_fwd.hip")) else None}

# same bytes on both routes before anything is timed
chain(True)(); one_call(pinned_b)(); one_call(dev_b)()
torch.cuda.synchronize()
result["routes_give_the_same_bytes"] = bool(torch.equal(pinned_a, pinned_b) and torch.equal(dev_a.cpu(), pinned_b) and
                                            torch.equal(dev_b.cpu(), pinned_b))

for name, host in (() if args.skip_corrected else (("host", True), ("device", False))):
    cell = measure({"chain": chain(host), "one_call": one_call(pinned_b if host else dev_b)})
    cell["chain_over_one_call"] = cell["chain"]["us"] / cell["one_call"]["us"]
    result["corrected_" + name] = cell


# ---- the uncorrected frame through the C ABI: this library against the parent's ----
class Epilogue(ctypes.Structure):     # grpg_frame_epilogue
    _fields_ = [("sky_cube", ctypes.c_void_p), ("sky_res", ctypes.c_int), ("ray_matrix", ctypes.c_void_p),
                ("ray_matrix_on_device", ctypes.c_int), ("sky_fill", ctypes.c_float), ("clamp", ctypes.c_int),
                ("out_rgb8", ctypes.c_void_p), ("truncate", ctypes.c_int), ("out_rgb8_on_host", ctypes.c_int)]


ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class CFrame:
    """grpg_forward_frame of one library: bytes only, blobs kept and grown like the binding's"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.grpg_forward_frame.restype = ctypes.c_int
        self.lib.grpg_last_error.restype = ctypes.c_char_p
        self.blobs = {}

        def alloc(nbytes, user):
            t = self.blobs.get(user)
            if t is None or t.numel() < nbytes:
                t = self.blobs[user] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            return t.data_ptr()
        self.cb = ALLOC(alloc)
        self.radii = torch.empty(scene.means3D.shape[0], dtype=torch.int32, device=dev)
        self.epi = {}

    def frame(self, out):
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        ep = self.epi.setdefault(out.data_ptr(), Epilogue(
            sky.sky_cube_map.data_ptr(), args.sky_res, rm.data_ptr(), 1, 0.0, 1, out.data_ptr(), 1, 0 if out.is_cuda else 1))
        P, M = int(scene.means3D.shape[0]), int(scene.shs.shape[1])
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        f = ctypes.c_float

        def run():
            rc = self.lib.grpg_forward_frame(
                self.cb, ctypes.c_void_p(1), self.cb, ctypes.c_void_p(2), self.cb, ctypes.c_void_p(3), P, scene.sh_degree, M,
                p(bg), W, H, p(scene.means3D), p(scene.shs), None, p(scene.opacity), p(scene.scales), f(1.0),
                p(scene.rotations), None, p(cam.viewmatrix), p(cam.projmatrix), p(cam.campos), f(cam.tanfovx),
                f(cam.tanfovy), None, None, None, None, None, None, None, None, None, p(self.radii), 0, stream,
                ctypes.byref(ep))
            assert rc >= 0, self.lib.grpg_last_error()
        return run


if args.parent and args.parent_b:
    paths = {"this": build.LIB_PATH, "parent": args.parent, "parent_b": args.parent_b}
    libs = {k: CFrame(paths[k]) for k in args.lib_order.split(",")}
    result["lib_order"] = list(libs)
    outs = {k: (torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W, 3), dtype=torch.uint8).pin_memory())
            for k in libs}
    for k, c in libs.items():
        c.frame(outs[k][0])(); c.frame(outs[k][1])()
    torch.cuda.synchronize()
    result["uncorrected_same_bytes_as_parent"] = bool(all(
        torch.equal(outs[k][i].cpu(), outs["parent"][i].cpu()) for k in libs for i in (0, 1)))
    for i, name in ((0, "device"), (1, "host")):
        cell = measure({k: c.frame(outs[k][i]) for k, c in libs.items()})
        # per repetition: this - parent beside parent_b - parent (the same job, the same alternation)
        d_this = [a - b for a, b in zip(cell["this"]["repetitions_us"], cell["parent"]["repetitions_us"])]
        d_self = [a - b for a, b in zip(cell["parent_b"]["repetitions_us"], cell["parent"]["repetitions_us"])]
        cell["this_minus_parent_us"] = {"median": median(d_this), "repetitions": d_this}
        cell["parent_b_minus_parent_us"] = {"median": median(d_self), "repetitions": d_self}
        cell["parent_against_parent_spread_us"] = max(abs(x) for x in d_self + [
            cell["parent"]["max_us"] - cell["parent"]["min_us"], cell["parent_b"]["max_us"] - cell["parent_b"]["min_us"]])
        cell["inside_spread"] = bool(abs(median(d_this)) <= cell["parent_against_parent_spread_us"])
        result["uncorrected_" + name] = cell
else:
    result["uncorrected_device"] = result["uncorrected_host"] = "not measured: no --parent / --parent-b library given"

benchkit.emit(result, args.out)
