"""Colour correction of the frame (gaussianrpg_amd/appearance.py): the three per-pixel steps behind the op in
StreetGaussianRenderer.render -- sky composite, ColorCorrection.forward, clamp -- and the simulator's byte conversion,
two routes timed on the same GPU in ONE process, alternating batch by batch, at 1920x1280:
(a) fused    harness.render_corrected(fused=True) / appearance.corrected_frame: one forward launch
             (csrc/color_correction.hip), a backward launch plus the fixed-order reduction and the sky backward;
(b) unfused  harness.render_corrected(fused=False): SkyCubeMap.composite (HIP, unclamped) -> the reference's einsum
             line in PyTorch -> clamp -> trajectory.pack_hwc.
Cases: "train"  forward + backward of sum(y * g) w.r.t. the cube map, rgb, acc and the matrix (train mode);
       "bytes"  the evaluation frame as uint8 [H,W,3] from the op's planes;
       "train_no_sky" / "bytes_no_sky"  the same without the composite (the correction alone against the einsum line):
                both routes of the first two cases share the camera's ray matrix (a 3x3 float64 inverse on the device,
                a dozen small launches) and, in training, the zero fill and scatter of the 1024^2 cube-map gradient.
Per route and case: the wall time per call of a batch of --inner back-to-back calls between two synchronises (what a
frame loop pays) and the device time per call between two events around the batch; median over --batches batches after
--warmup batches, --reps times.  Prints one JSON line; --out FILE also writes it (profiles/color_correction_bench.json)."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import benchkit
from benchkit import column, median
from gaussianrpg_amd import appearance, harness
from gaussianrpg_amd.sky import SkyCubeMap
from gaussianrpg_amd.trajectory import pack_hwc

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--height", type=int, default=1280)
ap.add_argument("--width", type=int, default=1920)
args = ap.parse_args()

benchkit.require_gpu("bench_color_correction")
dev = torch.device("cuda:0")
H, W = args.height, args.width

g = torch.Generator().manual_seed(H + W)
sky = SkyCubeMap(1024, mode="evaluate").to(dev)
with torch.no_grad():
    sky.sky_cube_map.copy_((torch.rand(6, 1024, 1024, 3, generator=g) * 1.2 - 0.1).to(dev))
cam = harness.trajectory_camera(0, W=W, H=H, device="cpu")
K = torch.tensor([[harness.WAYMO_FX, 0.0, W / 2.0], [0.0, harness.WAYMO_FY, H / 2.0], [0.0, 0.0, 1.0]]).to(dev)
w2c = cam.viewmatrix.transpose(0, 1).contiguous().to(dev)
rgb = torch.rand(3, H, W, generator=g).to(dev).requires_grad_(True)
acc = (torch.rand(1, H, W, generator=g) * 0.98).to(dev).requires_grad_(True)
affine = (torch.eye(4)[:3] + 0.1 * (torch.rand(3, 4, generator=g) - 0.5)).to(dev).requires_grad_(True)
up = torch.randn(3, H, W, generator=g).to(dev)
leaves = (sky.sky_cube_map, rgb, acc, affine)


def train(fused, s=sky):
    wrt = leaves if s is not None else (rgb, affine)

    def run():
        y = harness.render_corrected(rgb, acc, affine, s, K, w2c, train=True, fused=fused)
        return torch.autograd.grad(y, wrt, up)
    return run


def frame(fused, s=sky):
    r, a, A = rgb.detach(), acc.detach(), affine.detach()

    def run():
        if fused:
            return appearance.corrected_frame(r, a, A, sky=s, K=K, w2c=w2c)
        return pack_hwc(harness.render_corrected(r, a, A, s, K, w2c, fused=False), True)
    return run


result = {"what": "sky composite + colour correction (+ clamp + bytes) at %dx%d; us per call: per cell the median over "
                  "%d repetitions of (median over %d batches of %d back-to-back calls between two synchronises, after "
                  "%d warm-up batches); the routes alternate batch by batch in one process; the camera's ray matrix "
                  "(a 3x3 inverse on the device) is part of both routes" %
                  (W, H, args.reps, args.batches, args.inner, args.warmup),
          "device": torch.cuda.get_device_name(0), "cases": {}}
for name, make, s in (("train", train, sky), ("bytes", frame, sky), ("train_no_sky", train, None),
                      ("bytes_no_sky", frame, None)):
    routes = {"fused": make(True, s), "unfused": make(False, s)}
    reps = {k: {"wall": [], "device": []} for k in routes}
    for _ in range(args.reps):
        seen = benchkit.alternating(routes, args.batches, args.warmup, inner=args.inner)
        for k in routes:
            reps[k]["wall"].append(median(column(seen[k], "wall_us")))
            reps[k]["device"].append(median(column(seen[k], "device_us")))
    cell = {}
    for k in routes:
        cell[k] = {"wall_us": median(reps[k]["wall"]), "wall_repetitions_us": reps[k]["wall"],
                   "device_us": median(reps[k]["device"]), "device_repetitions_us": reps[k]["device"]}
    cell["unfused_over_fused_wall"] = cell["unfused"]["wall_us"] / cell["fused"]["wall_us"]
    cell["unfused_over_fused_device"] = cell["unfused"]["device_us"] / cell["fused"]["device_us"]
    result["cases"][name] = cell

benchkit.emit(result, args.out)
