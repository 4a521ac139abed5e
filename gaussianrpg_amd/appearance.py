"""Colour correction of the frame on the HIP library (csrc/color_correction.hip; additive API).

``StreetGaussianRenderer.render`` ends in three per-pixel steps (lib/models/street_gaussian_renderer.py:105-116):
``rgb + sky * (1 - acc)``, ``pc.color_correction(camera, rgb)`` and the evaluation clamp.  The middle one is
``ColorCorrection.forward`` (lib/models/color_correction.py:129-132), a learned 3x4 affine map of every pixel, one
matrix per image or per sensor.  This module provides it, alone and fused with its two neighbours:

    cc = ColorCorrection(num_images, mode='image').cuda()
    rgb = cc(camera, rgb)                                            # the reference's call, one launch each way
    rgb = sky_corrected(sky, rgb, acc, cc.get_affine_trans(camera), camera=camera)    # lines 106-116, ONE launch
    frame = corrected_frame(rgb, acc, A, sky=sky, K=K, w2c=w2c)      # evaluation: the uint8 [H,W,3] frame

The matrix is read from device memory by the kernel (``affine_trans[id]`` is a view: no host copy, no host wait), the
backward recomputes the kernel's input instead of storing it and sums the matrix gradient in a fixed order without
atomics: identical calls give identical bits.

Covered: the explicit variant (``use_mlp: false``), both modes, training and evaluation.  The layers of the ``use_mlp``
variant are ``ColorCorrectionMLP`` (below); the [3,4] matrix they regress goes through ``color_correct`` unchanged,
gradient included.  Not covered: colour correction inside ``forward_frame``'s own epilogue: such a scene takes
``forward_frame(planes=True, rgb8=False, sky_cube=None, clamp=True)`` and then ``corrected_frame``.

The ``use_mlp: true`` variant (csrc/color_mlp.hip) is ``ColorCorrectionMLP``: the matrix is regressed from the camera
pose itself -- ``ego_pose @ extrinsic``, ``matrix_to_axis_angle``, four ``Linear`` layers, ``+ eye(4)[:3]`` -- so it
exists for poses that were never trained, which is what a closed-loop simulator renders:

    cc = ColorCorrectionMLP().cuda()
    A = cc.affines(ego_pose, extrinsic)                              # [T,2,3,4] (0 plain, 1 sky): ONE launch
    frame = rast.forward_frame(..., affine=A[0, 0])                  # the matrix never visits the host
    rgb = cc(camera, rgb); loss = loss + cc.regularization_loss(camera)      # training: one launch each way
"""
import torch
import torch.nn as nn

from .rasterizer import _C
from .sky import _camera_args, ray_matrix


class _ColorCorrect(torch.autograd.Function):
    """y = A[:, :3] x + A[:, 3], unclamped."""

    @staticmethod
    def forward(ctx, image, affine):
        out, _ = _C.color_correct(image, affine)
        ctx.save_for_backward(image, affine)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        image, affine = ctx.saved_tensors
        need_x, need_a = ctx.needs_input_grad
        if not (need_x or need_a):
            return None, None
        return _C.color_correct_backward(image, affine, grad_out.contiguous(), need_x, need_a)


class _SkyCorrected(torch.autograd.Function):
    """A (rgb + clamp(sky, 0, 1) * (1 - acc)), unclamped (train mode)."""

    @staticmethod
    def forward(ctx, cube, rgb, acc, affine, rm, fill, mask, jitter):
        out, _ = _C.color_correct(rgb, affine, cube=cube, ray_matrix=rm, fill=float(fill), acc=acc, mask=mask,
                                  jitter=jitter)
        ctx.save_for_backward(cube, rgb, acc, affine)
        ctx.rm, ctx.fill, ctx.mask, ctx.jitter = rm, float(fill), mask, jitter
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cube, rgb, acc, affine = ctx.saved_tensors
        need_cube, need_rgb, need_acc, need_a = ctx.needs_input_grad[:4]
        sky = dict(cube=cube, ray_matrix=ctx.rm, fill=ctx.fill, acc=acc, mask=ctx.mask, jitter=ctx.jitter)
        need_x = need_cube or need_rgb or need_acc
        grad_x, grad_a = _C.color_correct_backward(rgb, affine, grad_out.contiguous(), need_x, need_a, **sky)
        grad_cube = grad_acc = None
        if need_cube or need_acc:      # the composite's own backward, on A^T g
            grad_cube, grad_acc = _C.sky_backward(cube, ctx.rm, ctx.fill, acc, grad_x, ctx.mask, ctx.jitter)
            grad_acc = grad_acc.reshape(acc.shape)
        return grad_cube, grad_x, grad_acc, grad_a, None, None, None, None


def color_correct(image: torch.Tensor, affine: torch.Tensor, *, clamp: bool = False) -> torch.Tensor:
    """``einsum('ij,jhw->ihw', affine[:, :3], image) + affine[:, 3, None, None]`` (color_correction.py:131) for a
    float32 device image [3,H,W] and ANY float32 [3,4] device tensor: a row of the module's parameter, or the matrix
    the reference's MLP variant regresses.  Differentiable w.r.t. both; ``clamp=True`` is the evaluation form
    (clamped to [0,1], no gradient)."""
    if clamp:
        with torch.no_grad():
            return _C.color_correct(image, affine, clamp=True)[0]
    return _ColorCorrect.apply(image, affine)


class ColorCorrection(nn.Module):
    """Drop-in for the explicit variant of lib/models/color_correction.py:ColorCorrection (``use_mlp: false``): the
    same parameter names, shapes and initial values, the same ``get_id`` / ``get_affine_trans`` / ``forward`` /
    ``regularization_loss`` and the same ``{'params': ...}`` state-dict layout, so state dicts interchange.
    ``num_corrections`` is ``metadata['num_images']`` for ``mode='image'`` (one matrix per ``camera.id``) and
    ``metadata['num_cams']`` for ``mode='sensor'`` (one per ``camera.meta['cam']``).

    The ``use_mlp`` variant is NOT constructed here: it is ``ColorCorrectionMLP``, whose matrix goes through
    ``color_correct`` like this one's.  The optimizer is the caller's (``optim.FusedAdam`` or torch's)."""

    def __init__(self, num_corrections: int, mode: str = "image"):
        super().__init__()
        if mode not in ("image", "sensor"):
            raise ValueError("Invalid mode: %s" % mode)
        self.mode = mode
        eye = torch.eye(4).float()[:3]
        # not part of the state dict: the reference keeps it as a plain attribute
        self.register_buffer("identity_matrix", eye.clone(), persistent=False)
        self.affine_trans = nn.Parameter(eye.unsqueeze(0).repeat(int(num_corrections), 1, 1))
        self.affine_trans_sky = nn.Parameter(eye.unsqueeze(0).repeat(int(num_corrections), 1, 1))
        self.cur_affine_trans = None

    def save_state_dict(self, is_final: bool = True):
        state_dict = {"params": self.state_dict()}
        if not is_final and getattr(self, "optimizer", None) is not None:
            state_dict["optimizer"] = self.optimizer.state_dict()
        return state_dict

    def load_state_dict(self, state_dict, strict: bool = True):
        params = state_dict["params"]
        if "affine_trans" not in params:
            raise ValueError("the state dict holds the use_mlp variant of the colour correction (%s ...): its layers "
                             "are not constructed here, see gaussianrpg_amd.appearance" % sorted(params)[:1])
        return super().load_state_dict(params, strict=strict)

    def get_id(self, camera):
        if self.mode == "image":
            return camera.id
        return camera.meta["cam"]

    def get_affine_trans(self, camera, use_sky: bool = False):
        id = self.get_id(camera)
        affine_trans = self.affine_trans_sky[id] if use_sky else self.affine_trans[id]
        self.cur_affine_trans = affine_trans
        return affine_trans

    def forward(self, camera, image: torch.Tensor, use_sky: bool = False):
        return color_correct(image, self.get_affine_trans(camera, use_sky))

    def regularization_loss(self, camera):
        # twelve numbers: stays PyTorch (color_correction.py:134-140)
        affine_trans = self.get_affine_trans(camera, use_sky=False)
        affine_trans_sky = self.get_affine_trans(camera, use_sky=True)
        loss = torch.abs(affine_trans - self.identity_matrix) + torch.abs(affine_trans_sky - self.identity_matrix)
        return loss.mean()


class _ColorMlp(torch.autograd.Function):
    """(affine [T,2,3,4], reg [T], x [T,6]) from the poses and the sixteen parameters (eight weights, then eight
    biases, network-major).  One launch each way; nothing flows back to the poses."""

    @staticmethod
    def forward(ctx, ego_pose, extrinsic, state, *params):
        weights, biases = list(params[:8]), list(params[8:])
        affine, x, reg, hidden = _C.color_mlp_forward(weights, biases, ego_pose, extrinsic, True, True)
        ctx.save_for_backward(x, hidden, affine, *params)
        ctx.state = state
        ctx.mark_non_differentiable(x)
        ctx.set_materialize_grads(False)           # an absent upstream gradient stays None: a NULL in the backward
        return affine, reg, x

    @staticmethod
    def backward(ctx, grad_affine, grad_reg, _grad_x):
        x, hidden, affine, *params = ctx.saved_tensors
        if ctx.state is not None:
            ctx.state["consumed"] = True           # the node's buffers go with this call: the cache entry is spent
        if grad_affine is None and grad_reg is None:
            return (None,) * (3 + len(params))
        gw, gb = _C.color_mlp_backward(list(params[:8]), list(params[8:]), x, hidden, affine, grad_affine, grad_reg)
        return (None, None, None) + tuple(gw) + tuple(gb)


def _mlp(input_ch: int = 6, dim: int = 64) -> nn.Sequential:
    net = nn.Sequential(nn.Linear(input_ch, dim), nn.ReLU(), nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, dim),
                        nn.ReLU(), nn.Linear(dim, 12))
    net[6].weight.data.fill_(0)
    net[6].bias.data.fill_(0)
    return net


MLP_KEYS = tuple("%s.%d.%s" % (net, layer, kind) for net in ("affine_trans", "affine_trans_sky")
                 for layer in (0, 2, 4, 6) for kind in ("weight", "bias"))


class ColorCorrectionMLP(nn.Module):
    """Drop-in for the ``use_mlp: true`` variant of lib/models/color_correction.py:ColorCorrection: the two
    ``nn.Sequential`` networks of the reference's shape under the reference's names (state-dict keys
    ``affine_trans.0.weight`` ... ``affine_trans_sky.6.bias``, last layer zero-initialised), the same
    ``get_affine_trans`` / ``forward`` / ``regularization_loss`` and the same ``{'params': ...}`` state-dict layout.
    The matrix is regressed from the camera pose itself (``camera.ego_pose @ camera.extrinsic``), so it exists for
    poses that were never trained.  ``mode`` is kept for the reference's configuration; the networks do not depend on
    it.

    ``affines(ego_pose, extrinsic)`` -> ``[T,2,3,4]`` (index 0 plain, 1 sky) is ONE launch for T cameras and both
    networks; ``affines_and_reg`` returns the regulariser ``[T]`` of the same launch as well.  Both are differentiable
    w.r.t. the parameters (one backward launch for all sixteen gradients); the pose gets no gradient, as in the
    reference.  A row ``affines(...)[t, 0]`` is directly what ``color_correct`` / ``forward_frame(affine=...)`` take.

    Cache.  One training iteration calls ``get_affine_trans`` plain, sky and ``regularization_loss`` on the same
    camera; the three share the last launch when NOTHING it read can have changed: the same camera object, the same
    pose tensors at the same version, the same parameter storages at the same versions (an optimizer step, ``copy_``
    or ``load_state_dict`` bumps the version; a replaced ``.data`` changes the storage), the same grad mode, and its
    autograd node not yet backpropagated.  The three results then hang off ONE autograd node: backpropagate them
    together (the sum of the losses, as the trainer does), or pass ``retain_graph=True`` to separate backward calls,
    or set ``cache = False`` -- then every method call launches once.  Poses held as numpy arrays are never cached.

    No CPU path.  The optimizer is the caller's."""

    def __init__(self, mode: str = "image"):
        super().__init__()
        if mode not in ("image", "sensor"):
            raise ValueError("Invalid mode: %s" % mode)
        self.mode = mode
        self.register_buffer("identity_matrix", torch.eye(4).float()[:3].clone(), persistent=False)
        self.affine_trans = _mlp()
        self.affine_trans_sky = _mlp()
        self.cur_affine_trans = None
        self.cache = True
        self._cached = None        # (key, camera, state, affine, reg, x)

    def __getstate__(self):
        # copies and pickles leave the cache behind: it holds results with an autograd history and a camera
        state = self.__dict__.copy()
        state["_cached"] = None
        return state

    def save_state_dict(self, is_final: bool = True):
        state_dict = {"params": self.state_dict()}
        if not is_final and getattr(self, "optimizer", None) is not None:
            state_dict["optimizer"] = self.optimizer.state_dict()
        return state_dict

    def load_state_dict(self, state_dict, strict: bool = True):
        params = state_dict["params"]
        if "affine_trans" in params:
            raise ValueError("the state dict holds the explicit variant of the colour correction (affine_trans "
                             "[N,3,4]): load it into gaussianrpg_amd.appearance.ColorCorrection")
        return super().load_state_dict(params, strict=strict)

    def get_id(self, camera):
        if self.mode == "image":
            return camera.id
        return camera.meta["cam"]

    def _params(self):
        nets = (self.affine_trans, self.affine_trans_sky)
        weights = [net[l].weight for net in nets for l in (0, 2, 4, 6)]
        biases = [net[l].bias for net in nets for l in (0, 2, 4, 6)]
        if not weights[0].is_cuda:
            raise RuntimeError("no CPU path: ColorCorrectionMLP runs on a ROCm/HIP device only")
        return weights + biases

    def _poses(self, ego_pose, extrinsic, params):
        dev = params[0].device
        ego = torch.as_tensor(ego_pose, dtype=torch.float32, device=dev)
        ext = torch.as_tensor(extrinsic, dtype=torch.float32, device=dev)
        return ego.reshape(-1, 4, 4), ext.reshape(-1, 4, 4)

    def affines_and_reg(self, ego_pose, extrinsic, _state=None):
        """``(affine [T,2,3,4], reg [T], x [T,6])`` of ONE launch: ``ego_pose`` [T,4,4] (or [4,4]), ``extrinsic``
        [T,4,4] or one [4,4] / [1,4,4] for all T.  ``reg[t]`` is ``regularization_loss`` of camera t; ``x`` the
        axis-angle and translation the networks were fed (no gradient)."""
        params = self._params()
        ego, ext = self._poses(ego_pose, extrinsic, params)
        return _ColorMlp.apply(ego.detach(), ext.detach(), _state, *params)

    def affines(self, ego_pose, extrinsic):
        return self.affines_and_reg(ego_pose, extrinsic)[0]

    def _camera(self, camera):
        """(affine [1,2,3,4], reg [1]) of one camera object, through the cache (class docstring)."""
        ego, ext = camera.ego_pose, camera.extrinsic
        if not (self.cache and isinstance(ego, torch.Tensor) and isinstance(ext, torch.Tensor)):
            return self.affines_and_reg(ego, ext)[:2]
        params = self._params()
        key = (id(camera), id(ego), ego._version, id(ext), ext._version, torch.is_grad_enabled(),
               tuple((id(p), p.data_ptr(), p._version, p.requires_grad) for p in params))
        c = self._cached
        if c is not None and c[0] == key and c[1] is camera and c[2] is ego and c[3] is ext \
                and not c[4]["consumed"]:
            return c[5], c[6]
        state = {"consumed": False}
        affine, reg, _ = self.affines_and_reg(ego, ext, state)
        # the entry keeps the camera and its pose tensors alive, so their ids cannot be handed out again
        self._cached = (key, camera, ego, ext, state, affine, reg)
        return affine, reg

    def get_affine_trans(self, camera, use_sky: bool = False):
        affine_trans = self._camera(camera)[0][0, 1 if use_sky else 0]
        self.cur_affine_trans = affine_trans
        return affine_trans

    def forward(self, camera, image: torch.Tensor, use_sky: bool = False):
        return color_correct(image, self.get_affine_trans(camera, use_sky))

    def regularization_loss(self, camera):
        affine, reg = self._camera(camera)
        self.cur_affine_trans = affine[0, 1]       # the reference's last get_affine_trans call is the sky one
        return reg[0]


def _sky_inputs(sky, rgb, camera, K, w2c, mask, jitter):
    if camera is not None:
        K, w2c, _, _ = _camera_args(camera)
    mask, jitter = sky._train_extras(camera, rgb.shape[1], rgb.shape[2], mask, jitter)
    return ray_matrix(K, w2c), mask, jitter


def sky_corrected(sky, rgb, acc, affine, *, camera=None, K=None, w2c=None, train=None, mask=None, jitter=None):
    """Lines 106-116 of ``StreetGaussianRenderer.render`` in ONE forward launch: ``rgb + sky * (1 - acc)`` with the
    bits of ``sky.composite``, the colour correction by ``affine`` [3,4], and outside train mode the clamp.  ``sky`` is
    a ``gaussianrpg_amd.sky.SkyCubeMap``; camera / K / w2c / mask / jitter as in ``SkyCubeMap.composite``.  With
    ``train=True`` (default: ``sky.mode == 'train'``) the planes are unclamped and differentiable w.r.t. the cube map,
    ``rgb``, ``acc`` and ``affine``; otherwise they are clamped and carry no gradient."""
    if train is None:
        train = sky.mode == "train"
    rm, mask, jitter = _sky_inputs(sky, rgb, camera, K, w2c, mask, jitter)
    if train:
        return _SkyCorrected.apply(sky.sky_cube_map, rgb, acc, affine, rm, sky.fill, mask, jitter)
    with torch.no_grad():
        return _C.color_correct(rgb, affine, clamp=True, cube=sky.sky_cube_map, ray_matrix=rm, fill=sky.fill,
                                acc=acc, mask=mask, jitter=jitter)[0]


def corrected_frame(rgb, acc, affine, *, sky=None, camera=None, K=None, w2c=None, mask=None, jitter=None,
                    truncate=True, out=None):
    """Evaluation only: the uint8 [H,W,3] frame the simulator publishes, for a scene trained with colour correction
    (``forward_frame``'s own bytes are clamped and converted before the correction could be applied).  ``rgb`` / ``acc``
    are the planes of ``forward_frame(planes=True, rgb8=False, sky_cube=None, clamp=True)``; with ``sky`` the composite
    is done here, in front of the correction.  ``truncate`` as in ``pack_hwc``; ``out``: a preallocated uint8 [H,W,3]
    device tensor.  The bytes are ``pack_hwc`` of the clamped planes ``sky_corrected`` / ``color_correct`` return."""
    with torch.no_grad():
        if sky is None:
            return _C.color_correct(rgb, affine, clamp=True, planes=False, rgb8=True, truncate=bool(truncate),
                                    out=out)[1]
        rm, mask, jitter = _sky_inputs(sky, rgb, camera, K, w2c, mask, jitter)
        return _C.color_correct(rgb, affine, clamp=True, planes=False, rgb8=True, truncate=bool(truncate), out=out,
                                cube=sky.sky_cube_map, ray_matrix=rm, fill=sky.fill, acc=acc, mask=mask,
                                jitter=jitter)[1]
