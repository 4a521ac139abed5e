"""The render's rectangle cull on the bench frame (experiment build -DGRPG_CULL_COUNT): batches that run with a
full and with a shrunk live box, and the entries the cull removes in each, per path of the launch.
usage:  python -c "from gaussianrpg_amd import build; build.build_variant('cullcount')" && python tools/cull_count.py
The variant library is loaded with RTLD_GLOBAL before the package is imported, so the binding's calls
resolve to it in this process; nothing is preloaded."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lib = ctypes.CDLL(os.path.join(ROOT, "build", "variants", "libgrpg_rasterizer_cullcount.so"), mode=ctypes.RTLD_GLOBAL)
import numpy as np
import torch
from gaussianrpg_amd import harness as hz
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
CULL_BLOCK_VALU = 94   # vector instructions of splat_misses_rect per batch (gfx950 listing of the bench variant)
dev = torch.device("cuda:0")
sc = hz.street_scene(2_000_000, seed=2, sh_degree=1).to(dev)
buf = (ctypes.c_ulonglong * 12)()


def counts(reset):
    rc = lib.grpg_debug_cull_count(buf, 1 if reset else 0)
    assert rc == 0, rc
    return np.array(buf[:], dtype=np.int64).reshape(3, 4)


frames = (0, 1, 2, 3)
total = np.zeros((3, 4), dtype=np.int64)
for k in frames:
    cam = hz.trajectory_camera(k, device=dev)
    r = GaussianRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1)))
    counts(True)
    with torch.no_grad():   # the evaluation entry, as in bench.py
        r(means3D=sc.means3D, means2D=None, opacities=sc.opacity, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    torch.cuda.synchronize()
    c = counts(True)
    total += c
    print("frame %d" % k)
    print("  %-13s %12s %12s %14s %14s %10s" % ("path", "full batches", "shrunk", "culled (full)", "culled (shr.)", "full share"))
    for name, row in zip(("light", "quarter wave", "producer"), c):
        print("  %-13s %12d %12d %14d %14d %10.3f" % (name, row[0], row[1], row[2], row[3], row[0] / max(1, row[0] + row[1])))
    s = c.sum(0)
    print("  %-13s %12d %12d %14d %14d %10.3f" % ("all", s[0], s[1], s[2], s[3], s[0] / max(1, s[0] + s[1])))
s = total.sum(0) / len(frames)
print("mean per frame: %.0f full-box batches of %.0f (%.1f %%), %.1f entries culled on a full box"
      % (s[0], s[0] + s[1], 100.0 * s[0] / max(1.0, s[0] + s[1]), s[2]))
print("estimate: %.0f full-box batches x %d vector instructions of the cull = %.2f M per launch"
      % (s[0], CULL_BLOCK_VALU, s[0] * CULL_BLOCK_VALU / 1e6))
