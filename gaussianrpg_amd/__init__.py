"""gaussianrpg_amd -- MI355X-native (gfx950 / CDNA4) 3D-Gaussian-splatting rasterizer.

Drop-in for the hot path of GimpelZhang/GaussianRPG: the ``diff_gaussian_rasterization``
operator (``GaussianRasterizer`` / ``GaussianRasterizationSettings`` over
``_C.rasterize_gaussians`` / ``_C.rasterize_gaussians_backward``).

Layout:
  csrc/           hand-written HIP kernels + the C ABI (``libgrpg_rasterizer.so``) and the torch
                  binding (``_C``)
  rasterizer.py   host-side mirror of the reference's Python operator interface
  harness.py      build-owned counterpart of the reference's callers (cameras, synthetic scenes)
  trajectory.py   frame-sharded multi-GPU trajectory rendering (one process per GPU, RCCL gather)
  perception.py   the frame as the in-process detector's input: letterbox + CHW + / 255 in one launch;
                  the detector's output as detections: NMS + the mapping back to the frame, no host wait
  tracks.py       tracklets + optimised corrections + timestamp + ego pose -> every actor's world pose in one
                  launch, with backward to opt_trans / opt_rots (the step in front of composed.py)
  session.py      closed-loop evaluation: a scene bound once to a pose tape (segment tables of all frames baked on the
                  device), then one call per frame with nothing in front of its first launch
  closed_loop.py  the loop around the session on the device: detections -> object positions, brake decision, ego step
                  and the next frame's camera row in one launch per frame, no host wait
  lpips.py        LPIPS (AlexNet, VGG16) as one native call: the third number of the reference's metrics.py, next to
                  loss.ssim and loss.psnr
  build.py        in-tree build (hipcc for gfx950, g++ for the binding)

Importing this package does not load native code; ``gaussianrpg_amd.rasterizer`` does, and fails
loudly if the extension has not been built -- there is no CPU or PyTorch fallback.
"""
__version__ = "0.1.0"
