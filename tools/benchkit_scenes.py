"""The scene the closed-loop side benches share (bench_device_poses, bench_session, bench_ego_loop, bench_detector
--closed-loop): tracked actors on the road ahead, their models behind a street background, a pose tape, and the fixed
synthetic detector heads.  Imported by tools/bench_*.py after they have put the repository root on sys.path."""
import math

import numpy as np
import torch

from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.composed import ModelParams
from gaussianrpg_amd.tracks import TrackTable, TrackedActorPoses

LENGTH = 198
BASE = 1.5e9
FOURIER = 5

W, H = hz.WAYMO_W, hz.WAYMO_H
NC, NA, MAX_DET = 80, 3, 10
ANCHORS = [[[10, 13], [16, 30], [33, 23]], [[30, 61], [62, 45], [59, 119]], [[116, 90], [156, 198], [373, 326]]]
STRIDES = [8.0, 16.0, 32.0]


def make_actors(A, dev, seed=0):
    """A cars on the road ahead, ten to a row, driving slowly forward: tracks of LENGTH entries, one column per actor"""
    rng = np.random.RandomState(seed)
    F = LENGTH
    tr = np.zeros((F, A, 8), np.float32)
    for a in range(A):
        yaw = 0.05 * (a % 10) + 0.002 * np.arange(F) + rng.normal(0, 0.002, F)
        tr[:, a, 0] = a
        tr[:, a, 1:4] = np.stack([np.full(F, -12.0 + 2.5 * (a % 10)) + 0.6 * (a // 10), np.full(F, 0.8),
                                  10.0 + 8.0 * (a % 10) + 1.5 * (a // 10) + 0.05 * np.arange(F)], 1)
        tr[:, a, 4], tr[:, a, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    stamps = BASE + 0.1 * np.arange(F)
    info = {a: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1]) for a in range(A)}
    m = TrackedActorPoses(TrackTable.from_tracklets(tr, stamps, info), device=dev)
    with torch.no_grad():
        m.opt_trans.normal_(0, 0.02)
        m.opt_rots.normal_(0, 0.01)
    return m


def make_models(A, NB, PA, dev, grad, seed=2):
    g = torch.Generator().manual_seed(seed)
    sc = hz.street_scene(NB, seed=seed)
    op = sc.opacity.clamp(1e-4, 1 - 1e-4)
    raw = [(sc.means3D, torch.log(sc.scales), sc.rotations * 1.7, torch.log(op / (1 - op)), sc.shs[:, :1].contiguous(),
            sc.shs[:, 1:].contiguous())]
    for _ in range(A):
        raw.append(((torch.rand(PA, 3, generator=g) - 0.5) * torch.tensor([4.5, 1.6, 2.0]),
                    float(np.log(0.05)) + 0.5 * torch.randn(PA, 3, generator=g), torch.randn(PA, 4, generator=g),
                    1.0 + 2.0 * torch.randn(PA, 1, generator=g), 0.5 * torch.randn(PA, FOURIER, 3, generator=g),
                    0.15 * torch.randn(PA, 3, 3, generator=g)))
    return [ModelParams(*(t.to(dev).requires_grad_(grad) for t in m)) for m in raw]


def make_tape(T):
    """T entries spread over the tracks' life, a camera creeping forward with a slight yaw, the ego pose along"""
    tape = []
    for k in range(T):
        yaw = 0.01 * math.sin(0.1 * k)
        R = np.array([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
        C = np.array([0.0, 0.0, 0.02 * k])
        ego = np.eye(4)
        ego[:3, 3] = [0.3, -0.2, 0.5 + 0.02 * k]
        tape.append(dict(id=k, timestamp=BASE + 0.1 * (0.3 + k * (LENGTH - 2.0) / T), rotation_matrix=R.tolist(),
                         position=(-R.transpose() @ C).tolist(), ego_pose=ego.tolist()))
    return tape


def synthetic_heads(dev, boxes, seed=11):
    """three conv outputs [1, 255, H/s, W/s]: logits around -7 (nothing passes), and `boxes` cells of the coarsest
    level with objectness and the class 'car' (2) at +3, below the horizon row"""
    g = torch.Generator().manual_seed(seed)
    heads = [torch.randn(1, NA * (5 + NC), H // int(s), W // int(s), generator=g) * 0.5 - 7.0 for s in STRIDES]
    ny, nx = H // 32, W // 32
    for i in range(boxes):
        gy, gx, a = ny // 2 + 2 + (i % 5) * 3, 3 + (i * 7) % (nx - 6), i % NA
        base = a * (5 + NC)
        heads[2][0, base:base + 4, gy, gx] = torch.tensor([0.0, 0.0, -1.0 + 0.1 * i, -1.0])
        heads[2][0, base + 4, gy, gx] = 3.0 - 0.1 * i
        heads[2][0, base + 5 + 2, gy, gx] = 3.0
    return [h.contiguous().to(dev) for h in heads]
