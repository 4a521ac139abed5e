"""Frame -> detector input (gaussianrpg_amd/perception.py): three routes from the rendered frame on the device to the
detector's float32 [1,3,h,w] tensor, timed on the same GPU in ONE process, alternating batch by batch:
(a) fused       perception.detector_input on the uint8 [H,W,3] device frame: one launch (csrc/letterbox.hip);
(b) torch       PyTorch on the device: permute -> float -> F.interpolate(bilinear, align_corners=False) when the plan
                resizes -> F.pad(114) -> flip -> div; not bit-identical to (a) (float bilinear, no 8-bit rounding);
(c) host_copies the host round trip ALONE: the device->host copy of the float32 [3,H,W] planes plus the host->device
                copy of the uint8 [3,h,w] bytes, pageable memory as in the reference, nothing computed in between -- a
                lower bound of the reference's route (simulator.py:333-346), which also runs cv2 on the host.
Cases: 1066x1600 pad-only and 1280x1920 pad-only (the reference's imgsz = width), 1280x1920 -> 640.
Per route and case: the wall time per call of a batch of --inner back-to-back calls between two synchronises (what a
frame loop pays), median over --batches batches after --warmup batches, --reps times; for (a) and (b) also the device
time per call between two events around the batch.
Prints one JSON line; --out FILE also writes it (profiles/letterbox_bench.json)."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import benchkit
from benchkit import column, median
from gaussianrpg_amd.perception import LetterboxPlan, detector_input

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--inner", type=int, default=200)
args = ap.parse_args()

benchkit.require_gpu("bench_letterbox")
dev = torch.device("cuda:0")
CASES = [("1066x1600 pad-only", 1066, 1600, None), ("1280x1920 pad-only", 1280, 1920, None),
         ("1280x1920 -> 640", 1280, 1920, 640)]

result = {"what": "frame -> detector input, float32 [1,3,h,w]; us per call: per cell the median over %d repetitions of "
                  "(median over %d batches of %d back-to-back calls between two synchronises, after %d warm-up "
                  "batches); the routes alternate batch by batch in one process" %
                  (args.reps, args.batches, args.inner, args.warmup),
          "device": torch.cuda.get_device_name(0), "cases": {}}

for name, H, W, new_shape in CASES:
    plan = LetterboxPlan.for_simulator(H, W, device=dev) if new_shape is None else LetterboxPlan(H, W, new_shape, device=dev)
    h, w = plan.out_shape
    top, bottom, left, right = plan.pad
    g = torch.Generator().manual_seed(H + W)
    planes = torch.rand(3, H, W, generator=g).to(dev)
    frame = (planes.permute(1, 2, 0) * 255).to(torch.uint8).contiguous()
    host_bytes = torch.zeros(3, h, w, dtype=torch.uint8)

    def fused():
        return detector_input(frame, plan)

    def torch_route():
        x = frame.permute(2, 0, 1)[None].float()
        if plan.needs_resize:
            x = F.interpolate(x, size=plan.resized, mode="bilinear", align_corners=False)
        x = F.pad(x, (left, right, top, bottom), value=114.0)
        return x.flip(1) / 255.0

    def host_copies():
        planes.cpu()
        return host_bytes.to(dev)

    routes = {"fused": (fused, True), "torch": (torch_route, True), "host_copies": (host_copies, False)}
    reps = {k: {"wall": [], "device": []} for k in routes}
    for _ in range(args.reps):
        seen = {k: [] for k in routes}
        for b in range(args.warmup + args.batches):
            for k, (fn, dt) in routes.items():
                r = benchkit.batch(fn, args.inner, events=dt)
                if b >= args.warmup:
                    seen[k].append(r)
        for k in routes:
            reps[k]["wall"].append(median(column(seen[k], "wall_us")))
            if routes[k][1]:
                reps[k]["device"].append(median(column(seen[k], "device_us")))
    cell = {"plan": repr(plan), "bytes_read": 3 * H * W, "bytes_written": 12 * h * w}
    for k in routes:
        cell[k] = {"wall_us": median(reps[k]["wall"]), "wall_repetitions_us": reps[k]["wall"]}
        if routes[k][1]:
            cell[k].update(device_us=median(reps[k]["device"]), device_repetitions_us=reps[k]["device"])
    cell["torch_over_fused_wall"] = cell["torch"]["wall_us"] / cell["fused"]["wall_us"]
    cell["host_copies_over_fused_wall"] = cell["host_copies"]["wall_us"] / cell["fused"]["wall_us"]
    cell["fused_device_GBps"] = (cell["bytes_read"] + cell["bytes_written"]) / cell["fused"]["device_us"] / 1e3
    result["cases"][name] = cell

benchkit.emit(result, args.out)
