"""Training step (forward + backward down to the raw parameters and poses) of a composed frame whose loss has the
object-alpha term (lambda_reg > 0: every shipped config):
(a) two calls, the route without forward_objects -- ComposedRasterizer.forward on all models, forward on the object
    models (train.py:145-158, render_object), one backward of the summed loss;
(b) one call -- ComposedRasterizer.forward_objects (grpg_object_alpha_forward / grpg_backward_composed_objects).
Scenes: harness.actor_scene's layout as a scene graph, 1.9 M + 10 x 10 k and 1 M + 10 x 10 k, 1920x1280.  Both routes
run in ONE process, alternating call by call on the same frames; per route the median of --calls
synchronize-bracketed steps after --warmup steps, --reps times.  The two new kernels alone: the object-alpha forward
(flag clear, class array + tile flags, blend) between two device events on a finished frame's blobs, and the backward
kernel as the difference of the library's preprocess-backward device time (grpg_get_backward_timing, which contains
it) with and without the plane's gradient, same medians.
Prints one JSON line; --out FILE also writes it (profiles/object_alpha_bench.json)."""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import benchkit
from benchkit import median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.composed import ActorPose, ComposedRasterizer, ModelParams
from gaussianrpg_amd.loss import obj_acc_loss
from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings, _C

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--backgrounds", type=int, nargs="+", default=[1_900_000, 1_000_000])
ap.add_argument("--width", type=int, default=hz.WAYMO_W)
ap.add_argument("--height", type=int, default=hz.WAYMO_H)
args = ap.parse_args()

benchkit.require_gpu("bench_object_alpha")
dev = torch.device("cuda:0")
NA, PA = 10, 10_000
W, H = args.width, args.height
logit = lambda p: torch.log(p / (1 - p))   # noqa: E731


def build(NB, seed=2):
    """harness.actor_scene(NB, 10, 10 k) as models + poses: car-sized boxes of small Gaussians on the road ahead"""
    g = torch.Generator().manual_seed(seed)
    sc = hz.street_scene(NB, seed=seed)
    models = [ModelParams(sc.means3D, torch.log(sc.scales), sc.rotations * 1.7, logit(sc.opacity.clamp(1e-4, 1 - 1e-4)),
                          sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous())]
    for k in range(NA):
        models.append(ModelParams((torch.rand(PA, 3, generator=g) - 0.5) * torch.tensor([4.5, 1.6, 2.0]),
                                  math.log(0.05) + 0.5 * torch.randn(PA, 3, generator=g),
                                  torch.randn(PA, 4, generator=g), 1.0 + 2.0 * torch.randn(PA, 1, generator=g),
                                  0.5 * torch.randn(PA, 1, 3, generator=g), 0.15 * torch.randn(PA, 3, 3, generator=g)))
    return [ModelParams(*(t.to(dev).requires_grad_(True) for t in m[:6])) for m in models]


def poses_at(f):
    out = [None]
    for k in range(NA):
        a = 0.05 * k + 0.002 * f
        out.append(ActorPose([math.cos(a / 2), 0.0, math.sin(a / 2), 0.0],
                             [-12.0 + 2.5 * k, 0.8, 10.0 + 8.0 * k + 0.5 * f], 0.0))
    return out


nframes = args.warmup + args.calls
cams = [hz.trajectory_camera(f, W=W, H=H, device=dev) for f in range(nframes)]
rasts = [ComposedRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(c, 1))) for c in cams]
bound = (torch.rand(1, H, W, generator=torch.Generator().manual_seed(1)) < 0.3).to(dev)
result = {"what": "train step with the object-alpha term, background + 10 actors x 10 k, %dx%d; per cell the median over "
                  "%d repetitions of (median of %d synchronize-bracketed calls after %d warm-up calls), ms; the two "
                  "routes alternate call by call in one process" % (W, H, args.reps, args.calls, args.warmup),
          "device": torch.cuda.get_device_name(0), "scenes": {}}

for NB in args.backgrounds:
    models = build(NB)
    P = sum(m.xyz.shape[0] for m in models)

    def main_loss(o):
        return o[0].mean() + 0.1 * o[2].mean() + o[3].mean()

    def zero():
        for m in models:
            for t in m[:6]:
                t.grad = None

    def two_calls(f):
        zero()
        m2a = torch.zeros(P, 3, device=dev, requires_grad=True)
        m2b = torch.zeros(NA * PA, 3, device=dev, requires_grad=True)
        ps = poses_at(f)
        o = rasts[f].forward(models, ps, means2D=m2a)
        ob = rasts[f].forward(models[1:], ps[1:], means2D=m2b)
        (main_loss(o) + obj_acc_loss(ob[3], bound)).backward()

    def one_call(f):
        zero()
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        o = rasts[f].forward_objects(models, poses_at(f), means2D=m2)
        (main_loss(o) + obj_acc_loss(o[5], bound)).backward()

    def kernels(f):
        """device times, ms: (the object-alpha forward -- flag clear, class + flag pass, blend -- between two events on
        the stream; the preprocess-backward figure of the library's backward timing with the plane's gradient, which
        contains the object-alpha backward kernel; the same figure without)"""
        zero()
        o = rasts[f].forward_objects(models, poses_at(f))
        lm, lo = main_loss(o), obj_acc_loss(o[5], bound)
        geom, binning, img = o[5].grad_fn.saved_tensors[2:5]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _C.object_alpha_forward(geom, binning, img, P, torch.empty(0, dtype=torch.uint8), H, W)
        e1.record(); torch.cuda.synchronize()
        _C.get_backward_timing()                      # drop what the routes above left
        lm.backward(retain_graph=True); torch.cuda.synchronize()
        _, pre_plain, n0 = _C.get_backward_timing()
        zero()
        (lm + lo).backward(); torch.cuda.synchronize()
        _, pre_with, n1 = _C.get_backward_timing()
        assert n0 == 1 and n1 == 1, (n0, n1)
        return e0.elapsed_time(e1), pre_with, pre_plain
    reps = {"two_calls": [], "one_call": [], "object_alpha_forward_device": [], "preprocess_bwd_with_plane_device": [],
            "preprocess_bwd_plain_device": []}
    for _ in range(args.reps):
        t2, t1, ks = [], [], []
        for f in range(nframes):
            a = benchkit.once(two_calls, f, events=False)["wall_us"] / 1e3
            b = benchkit.once(one_call, f, events=False)["wall_us"] / 1e3
            _C.set_stage_timing(1)
            k = kernels(f)
            _C.set_stage_timing(0)
            if f >= args.warmup:
                t2.append(a); t1.append(b); ks.append(k)
        reps["two_calls"].append(median(t2)); reps["one_call"].append(median(t1))
        for j, name in enumerate(("object_alpha_forward_device", "preprocess_bwd_with_plane_device",
                                  "preprocess_bwd_plain_device")):
            reps[name].append(median([k[j] for k in ks]))
    cell = {k: {"median_ms": median(v), "repetitions_ms": v} for k, v in reps.items()}
    cell["ratio_two_over_one"] = cell["two_calls"]["median_ms"] / cell["one_call"]["median_ms"]
    cell["object_alpha_backward_device_ms"] = (cell["preprocess_bwd_with_plane_device"]["median_ms"] -
                                               cell["preprocess_bwd_plain_device"]["median_ms"])
    cell["P"] = P
    result["scenes"]["%d + %d x %d" % (NB, NA, PA)] = cell
    del models
    torch.cuda.empty_cache()

benchkit.emit(result, args.out)
