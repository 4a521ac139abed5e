"""The case table of the selection tests (tests/test_selection_host.py, tests/test_gpu_selection.py): every fused op
of gaussianrpg_amd.loss that selects its elements, and the densification statistics of gaussianrpg_amd.optim, with
inputs whose deselected elements can be overwritten by a poison.  Host only: no GPU import.

The property: what a deselected element holds -- NaN, +-Inf, 1e30 -- changes no bit of the result.  The reference
selects with a boolean gather or torch.where, so its float64 statements in tests/ have the property already
(test_selection_host.py holds them to it); the kernels must have it too, and a gradient of exactly 0 at every
deselected element.  1e30 is the control: a kernel that multiplies by a 0/1 mask instead of selecting hides it
(0 * 1e30 = 0) but not NaN or Inf (0 * NaN = NaN).

A Case holds
  inputs     {name: CPU tensor}, float32 data, bool / uint8 masks, integer labels and radii
  selected   {name of a poisonable input: bool tensor of that input's shape, True where the op reads the element}
  targets    tuples of poisonable inputs that are poisoned together, one run each
  grads      the inputs that receive a gradient; grad_selected[name] (default selected[name]) is where it may be nonzero
  truth      f({name: tensor, float data in float64}) -> {output name: tensor}; 'loss' is the differentiable one
  reverse    the input that gets one NaN at a SELECTED element for the reverse check (None: no reverse check)
and poisoned(value, target) returns the inputs with every deselected element of the target's inputs set to value;
clean() is poisoned(0.0).

Out of scope: sky_loss and obj_acc_loss.  The reference reads every pixel of acc / acc_obj there (the mask only picks
the branch of a torch.where over the whole plane), and csrc/aux_loss.hip documents the same: the clamp passes NaN
through and NaN * 0 stays NaN.  In the aux_loss case with the sky term on, acc is therefore not poisoned.
A single tensor of N = 1 Gaussian cannot hold a selected and a deselected element at once; the one-Gaussian model is
the first of the three-model list instead.

Shapes are the smallest that cross the kernels' structure: the SSIM tile is 32x16 with a halo of 5, so 17x33 has four
tiles, three of them one pixel wide or high; the plane losses take four pixels at a time, so 8x8 is whole quads and
5x7 ends in a partial one; the semantic kernel keeps S <= 32 channels in registers and walks memory beyond; the
per-Gaussian kernels run 256 lanes to a workgroup."""
import math

import numpy as np
import torch

import aux_loss_truth
import normal_loss_truth
import optim_truth
import reg_loss_truth
import semantic_loss_truth
import ssim_truth

POISONS = (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")), ("1e30", 1e30))
SSIM_TILE = (16, 32)      # rows, columns of one workgroup's output tile (csrc/ssim.hip)
SSIM_HALO = 5


class Case:
    def __init__(self, op, name, inputs, selected, targets, truth, grads=(), grad_selected=None, reverse="first",
                 kwargs=None):
        self.op, self.name = op, name
        self.inputs, self.selected, self.targets, self.truth = inputs, selected, tuple(targets), truth
        self.grads = tuple(grads)
        self.grad_selected = dict(selected)
        self.grad_selected.update(grad_selected or {})
        self.reverse = next(iter(selected)) if reverse == "first" else reverse
        self.kwargs = kwargs or {}
        for n, s in selected.items():
            assert s.dtype == torch.bool and s.shape == inputs[n].shape, (op, name, n)

    @property
    def id(self):
        return "%s-%s" % (self.op, self.name)

    def poisoned(self, value, target=None):
        out = dict(self.inputs)
        for n in (self.selected if target is None else target):
            t = self.inputs[n].clone()
            t[~self.selected[n]] = value
            out[n] = t
        return out

    def clean(self):
        return self.poisoned(0.0)

    def nan_at_selected(self):
        """clean() with one NaN at the first selected element of the reverse input."""
        out = self.clean()
        t = out[self.reverse].clone()
        flat = torch.nonzero(self.selected[self.reverse].reshape(-1))[0, 0]
        t.view(-1)[flat] = float("nan")
        out[self.reverse] = t
        return out


def evaluate(case, inputs):
    """The float64 truth on `inputs` -> ({output: tensor}, {grad input: d loss / d input})."""
    x = {n: (t.double() if t.is_floating_point() else t) for n, t in inputs.items()}
    for n in case.grads:
        x[n] = x[n].clone().requires_grad_(True)
    vals = case.truth(x)
    grads = {}
    if case.grads:
        vals["loss"].backward()
        grads = {n: x[n].grad for n in case.grads}
    return {k: v.detach() for k, v in vals.items()}, grads


def same_bits(a, b):
    """Equal dtype, shape and bytes: NaN equals only the same NaN."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


# ---- SSIM / L1 / mix ----

def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    return a, b


def _ssim_masks():
    """name -> (image shape, mask)."""
    H, W = 17, 33
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    edge = ~((yy == 16) | (xx == 32))                      # false exactly on the one-pixel tiles
    seam = ~((xx >= 27) & (xx <= 36))                      # both sides of the column seam at 31 | 32
    first_tile = ~((yy < 16) & (xx < 32))
    one_true = (yy == 15) & (xx == 31)                     # the last pixel of the first tile
    checker = ((yy + xx) % 2) == 0
    per_channel = torch.stack([((yy + xx) % 3) != c for c in range(3)])
    y5, x5 = torch.meshgrid(torch.arange(5), torch.arange(7), indexing="ij")
    out = {
        "17x33-edge": ((3, H, W), edge[None]),
        "17x33-seam": ((3, H, W), seam[None]),
        "17x33-first_tile": ((3, H, W), first_tile[None]),
        "17x33-one_true": ((3, H, W), one_true[None]),
        "17x33-checker": ((3, H, W), checker[None]),
        "17x33-mask_chw": ((3, H, W), per_channel),
        "17x33-seam_uint8_255": ((3, H, W), seam[None].to(torch.uint8) * 255),
        "5x7-checker": ((1, 5, 7), (((y5 + x5) % 2) == 0)[None]),
        "2x3x17x33-mask_b1hw": ((2, 3, H, W), torch.stack([edge, seam])[:, None]),
    }
    return out


def _ssim_truth(kind):
    def f(x):
        m = x["mask"].bool()
        if kind == "ssim":
            return {"loss": ssim_truth.ssim(x["img1"], x["img2"], mask=m)}
        if kind == "l1_loss":
            return {"loss": ssim_truth.l1(x["img1"], x["img2"], m)}
        return {"loss": ssim_truth.mix(x["img1"], x["img2"], m), "l1": ssim_truth.l1(x["img1"], x["img2"], m),
                "ssim": ssim_truth.ssim(x["img1"], x["img2"], mask=m)}
    return f


def ssim_cases():
    out = []
    for k, (name, (shape, mask)) in enumerate(_ssim_masks().items()):
        a, b = _images(shape, 40 + k)
        sel = torch.broadcast_to(mask.bool(), shape).clone()
        for op in ("ssim", "l1_loss", "l1_ssim_loss"):
            out.append(Case(op, name, {"img1": a, "img2": b, "mask": mask}, {"img1": sel, "img2": sel},
                            [("img1",), ("img2",), ("img1", "img2")], _ssim_truth(op), grads=("img1",)))
    return out


def ssim_halo_ok(sel):
    """sel: bool [..., H, W].  -> (a deselected element lies within the halo of a selected one of its plane,
    such a pair lies in two different tiles -- None when the plane is a single tile)."""
    H, W = sel.shape[-2:]
    s = sel.reshape(-1, 1, H, W)

    def near(des):       # within SSIM_HALO of a deselected element of des
        return torch.nn.functional.max_pool2d(des.float(), 2 * SSIM_HALO + 1, 1, SSIM_HALO) > 0
    within = bool((near(~s) & s).any())
    if H <= SSIM_TILE[0] and W <= SSIM_TILE[1]:
        return within, None
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tile = (yy // SSIM_TILE[0]) * ((W + SSIM_TILE[1] - 1) // SSIM_TILE[1]) + xx // SSIM_TILE[1]
    across = False
    for t in tile.unique():
        inside = (tile == t)[None, None]
        across = across or bool((near(~s & inside) & s & ~inside).any())
    return within, across


# ---- PSNR ----

def psnr_cases():
    out = []
    for k, (H, W) in enumerate(((8, 8), (5, 7))):
        a, b = _images((3, H, W), 60 + k)
        g = torch.Generator().manual_seed(70 + k)
        mask = torch.rand(1, H, W, generator=g) < 0.6
        sel = torch.broadcast_to(mask, (3, H, W)).clone()
        out.append(Case("psnr", "%dx%d" % (H, W), {"img1": a, "img2": b, "mask": mask}, {"img1": sel, "img2": sel},
                        [("img1",), ("img2",)],
                        lambda x: {"psnr": reg_loss_truth.psnr64(x["img1"], x["img2"], x["mask"])}))
    return out


# ---- lidar depth (alone, in aux_loss, in aux_loss next to the sky term) ----

LAMBDA_LIDAR, LAMBDA_SKY, SKY_SCALE = 0.7, 0.3, 1.5


def _lidar_truth(op):
    def f(x):
        lid = aux_loss_truth.lidar(x["depth"], x["acc"], x["lidar"], x["mask"])
        if op == "lidar_depth_loss":
            return {"loss": lid}
        if op == "aux_loss_lidar":
            return {"loss": LAMBDA_LIDAR * lid, "lidar_depth_loss": lid}
        sky = aux_loss_truth.sky(x["acc"], x["sky"], SKY_SCALE)
        return {"loss": LAMBDA_LIDAR * lid + LAMBDA_SKY * sky, "lidar_depth_loss": lid, "sky_loss": sky}
    return f


def lidar_cases():
    out = []
    for k, (H, W) in enumerate(((8, 8), (5, 7))):
        g = torch.Generator().manual_seed(80 + k)
        shape = (1, H, W)
        depth = torch.rand(shape, generator=g) * 60 + 1
        acc = torch.rand(shape, generator=g) * 0.98 + 0.01
        lidar = torch.rand(shape, generator=g) * 80 + 0.5
        lidar[torch.rand(shape, generator=g) >= 0.6] = 0
        mask = torch.rand(shape, generator=g) < 0.7
        sky = torch.rand(shape, generator=g) < 0.25
        sel = aux_loss_truth.selection(lidar, mask)
        everywhere = torch.ones(shape, dtype=torch.bool)
        base = {"depth": depth, "acc": acc, "lidar": lidar, "mask": mask}
        # the lidar plane is poisonable where the mask is false: a NaN or -inf there deselects itself, +inf and
        # 1e30 are > 0 and only the mask keeps them out.  No reverse check: a NaN error at a selected pixel sorts
        # above +inf and the top-k rule decides (tests/test_gpu_aux_loss.py).
        selected = {"depth": sel, "acc": sel, "lidar": mask.clone()}
        for op in ("lidar_depth_loss", "aux_loss_lidar"):
            out.append(Case(op, "%dx%d" % (H, W), base, selected,
                            [("depth",), ("acc",), ("depth", "acc"), ("lidar",), ("depth", "acc", "lidar")],
                            _lidar_truth(op), grads=("depth", "acc"), reverse=None))
        # the sky term reads every pixel of acc
        out.append(Case("aux_loss_lidar_sky", "%dx%d" % (H, W), dict(base, sky=sky),
                        {"depth": sel, "lidar": mask.clone()}, [("depth",), ("lidar",), ("depth", "lidar")],
                        _lidar_truth("aux_loss_lidar_sky"), grads=("depth", "acc"),
                        grad_selected={"acc": everywhere}, reverse=None))
    return out


def shares_a_quad(sel):
    """Some group of four consecutive flat indices holds a selected and a deselected element."""
    s = sel.reshape(-1)
    for q in range(0, s.numel(), 4):
        quad = s[q:q + 4]
        if bool(quad.any()) and not bool(quad.all()):
            return True
    return False


# ---- semantic cross-entropy ----

def _semantic_truth(mode, stats):
    def f(x):
        loss = semantic_loss_truth.loss64(x["semantic"], x["gt"], mode)
        if not stats:
            return {"loss": loss}
        n_valid, n_bad, n_correct, _ = semantic_loss_truth.counts(x["semantic"], x["gt"])
        return {"loss": loss, "n_valid": torch.tensor(n_valid), "n_bad": torch.tensor(n_bad),
                "n_correct": torch.tensor(n_correct)}
    return f


def semantic_cases():
    out = []
    for S, H, W in ((1, 17, 33), (3, 17, 33), (19, 17, 33), (40, 17, 33), (3, 5, 7)):
        for mode in ("logits", "probabilities"):
            g = torch.Generator().manual_seed(1000 * S + H)
            sem = torch.randn(S, H, W, generator=g) if mode == "logits" else torch.rand(S, H, W, generator=g) * 0.98 + 0.01
            gt = torch.randint(0, S, (H, W), generator=g)
            gt[torch.rand(H, W, generator=g) < 0.25] = -1
            gt[0, 0], gt[1, 2], gt[H - 1, W - 1], gt[2, 1] = -(2 ** 40), -7, S, S + 3     # outside [-1, S): bad
            valid = (gt >= 0) & (gt < S)
            sel = torch.broadcast_to(valid[None], (S, H, W)).clone()
            for stats in (False, True):
                out.append(Case("semantic_loss_stats" if stats else "semantic_loss", "%s-S%d-%dx%d" % (mode, S, H, W),
                                {"semantic": sem, "gt": gt}, {"semantic": sel}, [("semantic",)],
                                _semantic_truth(mode, stats), grads=() if stats else ("semantic",),
                                kwargs={"mode": mode}))
    return out


# ---- mono-normal term ----

def _normal_truth(kw, terms):
    def f(x):
        l1, cos, n = normal_loss_truth.terms64(x["normals"], x["mono"], x["wvt"], x["mask"], x.get("sky"), **kw)
        if terms:
            return {"normal_l1_loss": l1, "normal_cos_loss": cos, "n_selected": torch.tensor(n)}
        return {"loss": l1 + cos}
    return f


def normal_cases():
    out = []
    for k, (H, W) in enumerate(((8, 8), (5, 7))):
        g = torch.Generator().manual_seed(90 + k)
        normals = torch.randn(3, H, W, generator=g) * (torch.rand(1, H, W, generator=g) * 2 + 0.05)
        mono = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        wvt = torch.eye(4)
        wvt[:3, :3] = q
        wvt[3, :3] = torch.randn(3, generator=g) * 10
        mask = torch.rand(1, H, W, generator=g) < 0.7
        sky = torch.rand(1, H, W, generator=g) < 0.3
        for name, s, top_rows in (("mask", None, 50), ("mask_sky_top2", sky, 2)):
            kw = {"normalize": True, "top_rows": top_rows}
            sel = normal_loss_truth.selection(mask, s, H, W, top_rows)
            sel3 = torch.broadcast_to(sel[None], (3, H, W)).clone()
            inputs = {"normals": normals, "mono": mono, "wvt": wvt, "mask": mask}
            if s is not None:
                inputs["sky"] = s
            for terms in (False, True):
                out.append(Case("normal_loss_terms" if terms else "normal_loss", "%dx%d-%s" % (H, W, name), inputs,
                                {"normals": sel3, "mono": sel3}, [("normals",), ("mono",), ("normals", "mono")],
                                _normal_truth(kw, terms), grads=() if terms else ("normals",), kwargs=kw))
    return out


# ---- opacity-sparse regulariser ----

LAMBDA_SCALE, LAMBDA_OPACITY = 0.5, 2.0


def _opacity_truth(names, with_scale):
    def f(x):
        o = reg_loss_truth.opacity_sparse64([x[n] for n in names], x["radii"])
        if not with_scale:
            return {"loss": o}
        s = reg_loss_truth.scale_flatten64(x["scaling"])
        return {"loss": LAMBDA_SCALE * s + LAMBDA_OPACITY * o, "scale_flatten_loss": s, "opacity_sparse_loss": o}
    return f


def opacity_cases():
    out = []
    for name, sizes in (("one_tensor_257", (257,)), ("three_models_1_257_41", (1, 257, 41))):
        g = torch.Generator().manual_seed(100 + len(sizes))
        N = sum(sizes)
        radii = (torch.rand(N, generator=g) < 0.6).int() * torch.randint(1, 40, (N,), generator=g).int()
        radii[0] = 0                       # the one-Gaussian model is invisible
        radii[1], radii[N - 1] = 5, 7
        radii[N // 2] = -1                 # a negative radius is invisible too
        names = ["opacities%d" % i for i in range(len(sizes))]
        inputs = {"radii": radii, "scaling": torch.randn(N, 3, generator=g) * 1.5 - 3}
        selected, start = {}, 0
        for n, size in zip(names, sizes):
            inputs[n] = torch.randn(size, 1, generator=g) * 4
            selected[n] = (radii[start:start + size] > 0)[:, None].clone()
            start += size
        for op in ("opacity_sparse_loss", "gaussian_reg_loss"):
            out.append(Case(op, name, inputs, selected, [tuple(names)],
                            _opacity_truth(names, op == "gaussian_reg_loss"),
                            grads=names, reverse=names[-1], kwargs={"names": names}))
    return out


# ---- densification statistics ----

DENSIFY_RANGES = ((0, 1), (1, 258))


def _densify_truth(x):
    sizes = [e - s for s, e in DENSIFY_RANGES]
    accum = [a.numpy().astype(np.float64).copy() for a in x["accum"].split(sizes)]
    denom = [d.numpy().astype(np.float64).copy() for d in x["denom"].split(sizes)]
    max_radii = [m.numpy().astype(np.float64).copy() for m in x["max_radii"].split(sizes)]
    optim_truth.densify_vectorized(x["grad_xyz"].numpy(), x["radii"].numpy(), DENSIFY_RANGES, accum, denom, max_radii)
    return {"accum": torch.from_numpy(np.concatenate(accum)), "denom": torch.from_numpy(np.concatenate(denom)),
            "max_radii": torch.from_numpy(np.concatenate(max_radii))}


def densify_cases():
    g = torch.Generator().manual_seed(110)
    P = DENSIFY_RANGES[-1][1]
    radii = (torch.rand(P, generator=g) < 0.6).int() * torch.randint(1, 200, (P,), generator=g).int()
    radii[0], radii[1], radii[P - 1], radii[P // 2] = 0, 3, 9, -4
    inputs = {"grad_xyz": torch.randn(P, 3, generator=g) * 1e-3, "radii": radii,
              "accum": torch.rand(P, 2, generator=g), "denom": torch.randint(0, 5, (P, 1), generator=g).float(),
              "max_radii": torch.randint(0, 100, (P,), generator=g).float()}
    sel = torch.broadcast_to((radii > 0)[:, None], (P, 3)).clone()
    return [Case("densify_stats", "1_257", inputs, {"grad_xyz": sel}, [("grad_xyz",)], _densify_truth)]


def all_cases():
    return (ssim_cases() + psnr_cases() + lidar_cases() + semantic_cases() + normal_cases() + opacity_cases()
            + densify_cases())


CASES = all_cases()
assert len({c.id for c in CASES}) == len(CASES)
assert all(math.isnan(v) or v != 0.0 for _, v in POISONS)
