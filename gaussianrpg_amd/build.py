"""In-tree build of the native pieces (no JIT cache: the .so files must travel with the repo).

* ``libgrpg_rasterizer.so`` -- hand-written HIP for gfx950 + the C ABI (include/grpg_rasterizer.h),
  compiled with ``hipcc --offload-arch=gfx950``; no torch dependency.
* ``_C.<abi>.so`` -- the PyTorch-ROCm extension module (csrc/torch_binding.cpp) that exposes the
  reference's operator surface on top of the C ABI; compiled with g++ against torch's headers.

Both land next to this file.  ``python -m gaussianrpg_amd.build`` builds everything.
"""
import glob
import os
import shutil
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(ROOT, "build", "obj")
LIB_NAME = "libgrpg_rasterizer.so"
LIB_PATH = os.path.join(HERE, LIB_NAME)
EXT_PATH = os.path.join(HERE, "_C" + sysconfig.get_config_var("EXT_SUFFIX"))
ARCH = "gfx950"

# translation unit -> extra flags
HIP_UNITS = {
    # bit-exact integer outputs need the oracle's arithmetic: no FMA contraction
    # no SLP packing: with contraction off the unit is separate fp32 multiplies and adds, which the vectorizer pairs
    # into v_pk_mul_f32 / v_pk_add_f32 -- 4.15 SIMD cycles each against 2.25 for a plain one (tools/ubench/valu_rate.hip,
    # DESIGN_EXPERIMENTS.md section 6), plus the moves that gather the pairs; same IEEE result per operation
    "preprocess.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    "preprocess_bwd.hip": ["-ffp-contract=off"],
    "sort.hip": [],
    "binning.hip": [],
    "hier_binning.hip": [],
    "render_fwd.hip": [],
    # hardware global_atomic_add_f32 instead of a CAS loop; no SLP packing of the scalar gradient
    # arithmetic: a v_pk_fma_f32 occupies the gfx950 VALU 1.8x as long as a v_fma_f32
    # (tools/ubench/valu_rate.hip), so pairs only add moves
    "render_bwd.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    # object-alpha plane of a training frame and its backward: the blend's arithmetic, the same atomics
    "object_alpha.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    # bit-identical to oracle/knn_oracle.py: one rounding per operation
    "knn.hip": ["-ffp-contract=off"],
    # hardware float atomics for the cube-map gradient
    "sky.hip": ["-munsafe-fp-atomics"],
    # colour correction of the frame behind the sky composite: the affine map and A^T g are explicit fmaf chains, the
    # gradient terms single products (no FMA contraction); no atomics, deterministic fixed-order reduction
    "color_correction.hip": ["-ffp-contract=off"],
    # colour correction, use_mlp variant (pose -> the two 3x4 matrices): every layer a rounded multiply and a rounded
    # add per term in ascending order, as the numpy restatement (tests/color_mlp_truth.py); divisions and square roots
    # of the axis-angle correctly rounded; no atomics
    "color_mlp.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # pose correction of the background: every step the single float32 operation of the numpy restatement
    # (tests/pose_correction_truth.py), divisions and square roots correctly rounded; no atomics, deterministic
    # fixed-order reduction of the row's gradient
    "pose_correction.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # fused SSIM + L1 loss: no atomics, deterministic fixed-order reduction
    "ssim.hip": [],
    # fused lidar / sky / object-alpha losses: the error plane bit-identical to PyTorch's float32
    # expression (no FMA contraction); integer atomics only
    "aux_loss.hip": ["-ffp-contract=off"],
    # fused semantic cross-entropy: the backward recomputes the forward's softmax input bit for bit (no FMA
    # contraction); no atomics, deterministic fixed-order reduction
    "semantic_loss.hip": ["-ffp-contract=off"],
    # fused mono-normal loss, scale-flatten / opacity-sparse regularisers and PSNR: each backward recomputes its
    # forward bit for bit (no FMA contraction); no atomics, deterministic fixed-order reduction
    "normal_loss.hip": ["-ffp-contract=off"],
    "reg_loss.hip": ["-ffp-contract=off"],
    "metrics.hip": ["-ffp-contract=off"],
    # fused multi-tensor Adam step + densification statistics: one rounding per operation, in the order
    # written, on the vector and the scalar path alike (bit-identical across alignments)
    "optim.hip": ["-ffp-contract=off"],
    # fused densify-and-prune of all models: the apply pass recomputes a child's xyz / scaling with the bits the
    # classification saw (no FMA contraction); no atomics
    "densify.hip": ["-ffp-contract=off"],
    # feature planes of a composed frame: compose_one() must give the bits the composed preprocess sees (no FMA
    # contraction); no atomics, deterministic fixed-order reduction of the pose gradient
    "features.hip": ["-ffp-contract=off"],
    # frame -> detector input: the quantisation of the float planes must give pack_hwc's bytes and the host's
    # table arithmetic numpy's (no FMA contraction); q / 255 is a correctly rounded division, not a reciprocal
    "letterbox.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # detector output -> detections: every step of the IoU is one IEEE float32 operation as in the numpy restatement
    # (areaA + areaB - inter and iw * ih must not fuse), the division correctly rounded; no atomics.  The detector
    # head's decode lives here too: its sigmoid divides, and xy / wh are one rounding per step
    "nms.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # tracklets -> actor poses and back to opt_trans / opt_rots: every step the single float32 operation of the torch
    # restatement (tests/tracks_truth.py), divisions and square roots correctly rounded; no atomics
    "tracks.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # actor poses from device memory into the segment table: loads and stores only, no arithmetic
    "segment_pose.hip": [],
    # segment tables of a whole pose tape, baked once at bind time: loads and stores only as well
    "frame_table.hip": [],
    # the closed loop's tail (ranging, brake decision, ego step, next camera row): float64, every step the single
    # operation of the numpy restatement (tests/loop_truth.py) -- contraction off for the whole unit; the three
    # reductions numpy gives to BLAS are explicit fma() chains; the float32 xywh / gn a correctly rounded division;
    # no atomics
    "ego_loop.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # the detector's network: an implicit-GEMM convolution on the f32 matrix instructions (the chain of an output
    # element is the instruction's own, contraction has no say in it) and SPP's max-pools; SiLU's x * (1 / (1 + expf(-x)))
    # is a correctly rounded division and a rounded product, as nms.hip's sigmoid; no atomics
    "detector.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # the detector's network in fp16: the same launch list on the f16 matrix instructions, float32 accumulation and
    # epilogue, one rounding to fp16 per layer; SiLU as in detector.hip; no atomics
    "detector_f16.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # LPIPS: the detector's implicit-GEMM convolution with AlexNet's / VGG16's geometries, a z-score in the first
    # layer's gather ((x - mean) / std: a rounded subtraction and a correctly rounded division) and a ReLU epilogue;
    # the distance normalises with correctly rounded square roots and divisions and sums w (a - b)^2 one rounding per
    # operation (no FMA contraction; the sums of squares are explicit fmaf chains); no atomics, deterministic
    # fixed-order reduction
    "lpips.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    # LPIPS backward: convolution backward-data on the same matrix instructions, the pool's gather and the distance's
    # derivative with lpips.hip's roundings (its norms must be the forward's bits); no atomics
    "lpips_bwd.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
    "api.hip": [],
}
# units whose per-kernel register / scratch / LDS / occupancy report (-Rpass-analysis=kernel-resource-usage) is kept
# next to the object as <unit>.remarks: the render launch's occupancy is a budget the sources promise
# (render_fwd.hip render_min_waves; tests/test_render_resources.py reads the file), and so is
# the eight waves per SIMD of the specialised preprocess instantiations (tests/test_preprocess_resources.py); the
# use_mlp colour correction promises kernels without scratch (tests/test_color_mlp_host.py), and so do the detector's
# convolution and pool, whose LDS per workgroup is a budget too (tests/test_detector_resources.py,
# tests/test_detector_f16_resources.py) and LPIPS's kernels (tests/test_lpips_resources.py,
# tests/test_lpips_bwd_resources.py)
REMARK_UNITS = ("render_fwd.hip", "preprocess.hip", "color_mlp.hip", "detector.hip", "detector_f16.hip", "lpips.hip",
                "lpips_bwd.hip")


def headers():
    """The headers whose change makes every object stale: all of csrc/ and the public one."""
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(ROOT, "include", "grpg_rasterizer.h")]


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (needed to build the gfx950 kernels)")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd, keep=None):
    """keep: file that receives the command's output (the compiler's remarks)"""
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), p.stdout))
    if keep:
        with open(keep, "w") as f:
            f.write(p.stdout)
    return p.stdout


def compile_cmd(unit, extra, src_dir, obj):
    """The hipcc command line of one translation unit: its HIP_UNITS flags, then `extra`."""
    return [_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall",
            "-Wno-unused-function"] + HIP_UNITS[unit] + list(extra) + ["-c", os.path.join(src_dir, unit), "-o", obj]


def link_cmd(objs, out):
    return [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", out] + list(objs) + \
           ["-Wl,--enable-new-dtags", "-Wl,-rpath,/opt/rocm/lib"]


def _stale(obj, unit):
    return _newer(obj, [os.path.join(CSRC, unit)] + headers() + [os.path.abspath(__file__)])


def remarks_path(unit):
    return os.path.join(OBJ, unit.replace(".hip", ".remarks"))


def kernel_resources(unit="render_fwd.hip"):
    """{mangled kernel name: {"vgprs", "agprs", "sgprs", "scratch", "occupancy", "lds"}} as hipcc reported them when
    build_native() last compiled `unit` (one of REMARK_UNITS)."""
    import re
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}
    out, cur = {}, None
    with open(remarks_path(unit)) as f:
        for line in f:
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = out.setdefault(m.group(2), {})
            elif cur is not None and m.group(1) in keys:
                cur[keys[m.group(1)]] = int(m.group(2))
    return out


def build_native(force=False, verbose=False):
    """hipcc -> libgrpg_rasterizer.so (gfx950 only)."""
    os.makedirs(OBJ, exist_ok=True)
    jobs = []
    objs = []
    for unit in HIP_UNITS:
        obj = os.path.join(OBJ, unit.replace(".hip", ".o"))
        objs.append(obj)
        keep = remarks_path(unit) if unit in REMARK_UNITS else None
        if force or _stale(obj, unit) or (keep and not os.path.exists(keep)):
            extra = (["-Rpass-analysis=kernel-resource-usage"] if keep else []) + \
                    os.environ.get("GRPG_EXTRA_HIPCC_FLAGS", "").split()   # experiments (-D...)
            jobs.append((compile_cmd(unit, extra, CSRC, obj), keep))
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as ex:
            for (_, keep), out in zip(jobs, ex.map(lambda j: _run(*j), jobs)):
                if verbose and out.strip() and not keep:
                    print(out)
    if force or jobs or _newer(LIB_PATH, objs):
        _run(link_cmd(objs, LIB_PATH))
    return LIB_PATH


def build_binding(force=False, verbose=False):
    """g++ -> _C extension module linking libgrpg_rasterizer.so and torch."""
    import torch
    from torch.utils import cpp_extension as ce
    src = os.path.join(CSRC, "torch_binding.cpp")
    hdr = os.path.join(ROOT, "include", "grpg_rasterizer.h")
    if not (force or _newer(EXT_PATH, [src, hdr, os.path.abspath(__file__)])):
        return EXT_PATH
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-variable",
           "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DTORCH_EXTENSION_NAME=_C",
           "-DTORCH_API_INCLUDE_EXTENSION_H",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    for inc in ce.include_paths() + [sysconfig.get_paths()["include"], os.path.join(rocm, "include")]:
        cmd += ["-isystem", inc]
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    cmd += [src, "-o", EXT_PATH, "-L" + HERE, "-l:" + LIB_NAME, "-L" + torch_lib, "-ltorch",
            "-ltorch_cpu", "-ltorch_python", "-lc10", "-lc10_hip", "-ltorch_hip",
            "-Wl,--enable-new-dtags", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + torch_lib]
    out = _run(cmd)
    if verbose and out.strip():
        print(out)
    return EXT_PATH


# Test variants of the C-ABI library: the same sources with one translation unit recompiled under an
# extra -D.  They live under build/variants/ (git-ignored like every built file), are loaded through
# ctypes by the one test that needs them and are never imported by the package.
VARIANTS = {
    # every producer / consumer hand-over of the render gives up at once: the timeout -> error path
    # (render_fwd.hip pc_fail, tests/test_gpu_pc_timeout.py)
    "pcspin0": {"render_fwd.hip": ["-DGRPG_PC_SPIN_LIMIT=0"]},
}
# Instrumented builds of the stages DESIGN.md section 10 lists as open; outputs stay correct.  Not built by
# build_all: python -c "from gaussianrpg_amd import build; build.build_variant('dstrace')"
# (tests/test_build_variants.py holds every flag of both tables against the sources)
EXPERIMENT_VARIANTS = {
    # phase timestamps of the depth sort's scatter passes (tools/ds_trace.py)
    "dstrace": {"sort.hip": ["-DGRPG_DS_TRACE"]},
    # per-workgroup life of the point-list fill (tools/fill_trace.py)
    "filltrace": {"hier_binning.hip": ["-DGRPG_FILL_TRACE"]},
    # the render's rectangle cull: batches with a full / a shrunk live box and what the cull removes in each,
    # per path of the launch (tools/cull_count.py)
    "cullcount": {"render_fwd.hip": ["-DGRPG_CULL_COUNT"]},
}


def variant_path(name):
    return os.path.join(ROOT, "build", "variants", "libgrpg_rasterizer_%s.so" % name)


def build_variant(name, force=False):
    """build/variants/libgrpg_rasterizer_<name>.so from the objects of build_native(), except the
    units VARIANTS[name] lists, which are recompiled with the extra flags."""
    build_native()
    spec = VARIANTS.get(name) or EXPERIMENT_VARIANTS[name]
    out = variant_path(name)
    vobj = os.path.join(ROOT, "build", "obj_" + name)
    os.makedirs(vobj, exist_ok=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    objs = []
    for unit in HIP_UNITS:
        if unit not in spec:
            objs.append(os.path.join(OBJ, unit.replace(".hip", ".o")))
            continue
        obj = os.path.join(vobj, unit.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, unit):
            _run(compile_cmd(unit, spec[unit], CSRC, obj))
    if force or _newer(out, objs):
        _run(link_cmd(objs, out))
    return out


def build_all(force=False, verbose=False):
    build_native(force=force, verbose=verbose)
    build_binding(force=force, verbose=verbose)
    for name in VARIANTS:
        build_variant(name, force=force)
    return LIB_PATH, EXT_PATH


if __name__ == "__main__":
    paths = build_all(force="--force" in sys.argv, verbose=True)
    print("built:", *paths, sep="\n  ")
