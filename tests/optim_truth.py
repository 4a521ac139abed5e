"""Float64 statement of what gaussianrpg_amd.optim computes, written from the formulas (not from torch's source):

Adam (amsgrad = False, weight_decay = 0, maximize = False), per parameter with its own step count t:
    a parameter without a gradient is skipped entirely: p, m, v and t stay as they are;
    t = t + 1
    m = m + (g - m) (1 - beta1)
    v = v beta2 + (g g) (1 - beta2)
    p = p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

Densification statistics, per Gaussian i of a composed frame with radii[i] > 0, in model k's half-open range
[start, end), j = i - start:
    accum[k][j,0] += sqrt(g.x^2 + g.y^2);  accum[k][j,1] += |g.z|;  denom[k][j] += 1
    max_radii[k][j] = max(max_radii[k][j], radii[i])
"""
import math

import numpy as np

# the reference's optimizer (gaussian_model.py:292-304 with the shipped configs): one group per tensor
REF_EPS = 1e-15
REF_BETAS = (0.9, 0.999)
REF_GROUPS = (("xyz", 1.6e-4), ("f_dc", 0.0025), ("f_rest", 0.0025 / 20.0), ("opacity", 0.05),
              ("scaling", 0.005), ("rotation", 0.001), ("semantic", 0.0))


class AdamState:
    """One parameter: p, m, v as float64 arrays, t its step count."""

    def __init__(self, p):
        self.p = np.array(p, dtype=np.float64)
        self.p0 = self.p.copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.t = 0

    def step(self, g, lr, betas=REF_BETAS, eps=REF_EPS):
        if g is None:
            return self
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == self.p.shape
        beta1, beta2 = betas
        self.t += 1
        self.m = self.m + (g - self.m) * (1.0 - beta1)
        self.v = self.v * beta2 + (g * g) * (1.0 - beta2)
        step_size = lr / (1.0 - beta1 ** self.t)
        bc2_sqrt = math.sqrt(1.0 - beta2 ** self.t)
        self.p = self.p - step_size * self.m / (np.sqrt(self.v) / bc2_sqrt + eps)
        return self


def adam(p0, grads, lr, betas=REF_BETAS, eps=REF_EPS):
    """p0 stepped once per entry of `grads` (None: no gradient at that step).  Returns the AdamState."""
    s = AdamState(p0)
    for g in grads:
        s.step(g, lr, betas, eps)
    return s


def densify(grad, radii, ranges, accum, denom, max_radii):
    """In place, on float64 numpy arrays: accum[k] [n,2], denom[k] [n,1] or [n], max_radii[k] [n]."""
    grad = np.asarray(grad, dtype=np.float64)
    radii = np.asarray(radii)
    for k, (s, e) in enumerate(ranges):
        for j in range(e - s):
            i = s + j
            if radii[i] <= 0:
                continue
            accum[k][j, 0] += math.sqrt(grad[i, 0] * grad[i, 0] + grad[i, 1] * grad[i, 1])
            accum[k][j, 1] += abs(grad[i, 2])
            denom[k].reshape(-1)[j] += 1.0
            max_radii[k][j] = max(max_radii[k][j], float(radii[i]))


def densify_vectorized(grad, radii, ranges, accum, denom, max_radii):
    """The same statement without the Python loop (the 50-call test)."""
    grad = np.asarray(grad, dtype=np.float64)
    radii = np.asarray(radii)
    for k, (s, e) in enumerate(ranges):
        vis = radii[s:e] > 0
        g = grad[s:e]
        accum[k][vis, 0] += np.sqrt(g[vis, 0] * g[vis, 0] + g[vis, 1] * g[vis, 1])
        accum[k][vis, 1] += np.abs(g[vis, 2])
        denom[k].reshape(-1)[vis] += 1.0
        max_radii[k][vis] = np.maximum(max_radii[k][vis], radii[s:e][vis].astype(np.float64))


def rel_l2(a, b):
    """|a - b| / |b| over all elements, in float64; 0 when both are zero."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = float(np.linalg.norm(b))
    d = float(np.linalg.norm(a - b))
    return d / n if n > 0 else d
