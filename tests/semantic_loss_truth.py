"""Float64 statement of the reference's semantic training term (train.py:129-143) with the 'probabilities'
transform of street_gaussian_renderer.py:248-256, for the tests of gaussianrpg_amd.loss.semantic_loss.
Differentiable with autograd.  The same in float32 (loss32) is the reference's own arithmetic.

  semantic: [S,H,W] (or [1,S,H,W]); gt_semantic: [H,W] (or [1,H,W]) integer labels
  mode 'probabilities': x = log(semantic / (sum_c semantic + 1e-8) + 1e-8), else x = semantic
  loss = 0 when every label is -1 (the torch.all(gt_semantic == -1) guard), else
         F.cross_entropy(x[None], gt[None], ignore_index=-1, reduction='mean')

A label outside [-1, S) makes PyTorch raise a device assert; the fused kernel counts it as bad and ignores it, so
the statement here maps such labels to -1 first (sanitize)."""
import torch

EPS = 1e-8


def transform(semantic, mode):
    """street_gaussian_renderer.py:248-256 in the dtype of ``semantic``."""
    if mode == "logits":
        return semantic
    assert mode == "probabilities"
    x = semantic / (torch.sum(semantic, dim=0, keepdim=True) + EPS)
    return torch.log(x + EPS)


def sanitize(gt_semantic, S):
    """labels outside [-1, S) -> -1 (bad pixels are ignored)."""
    gt = gt_semantic.long()
    return torch.where((gt >= 0) & (gt < S), gt, torch.full_like(gt, -1))


def _loss(semantic, gt_semantic, mode, dtype):
    sem = semantic.reshape(semantic.shape[-3:]).to(dtype)
    gt = sanitize(gt_semantic.reshape(gt_semantic.shape[-2:]), sem.shape[0])
    if torch.all(gt == -1):
        return (sem * 0).sum()          # 0 with a zero gradient (train.py: torch.zeros_like(Ll1))
    x = transform(sem, mode).unsqueeze(0)   # [1,S,H,W]
    return torch.nn.functional.cross_entropy(input=x, target=gt.unsqueeze(0), ignore_index=-1, reduction="mean")


def loss64(semantic, gt_semantic, mode="logits"):
    return _loss(semantic, gt_semantic, mode, torch.float64)


def loss32(semantic, gt_semantic, mode="logits"):
    return _loss(semantic, gt_semantic, mode, torch.float32)


def manual64(semantic, gt_semantic, mode="logits"):
    """The same value from its definition (no F.cross_entropy): mean over the valid pixels of logsumexp - x_target."""
    sem = semantic.reshape(semantic.shape[-3:]).double()
    gt = sanitize(gt_semantic.reshape(gt_semantic.shape[-2:]), sem.shape[0])
    valid = gt >= 0
    if not bool(valid.any()):
        return (sem * 0).sum()
    x = transform(sem, mode)
    lse = torch.logsumexp(x, dim=0)
    xt = torch.gather(x, 0, gt.clamp_min(0).unsqueeze(0))[0]
    return ((lse - xt) * valid).sum() / valid.sum()


def counts(semantic, gt_semantic):
    """(n_valid, n_bad, n_correct, labels): labels = argmax over the channels of the raw planes (lowest on ties)."""
    sem = semantic.reshape(semantic.shape[-3:])
    gt = gt_semantic.reshape(gt_semantic.shape[-2:]).long()
    S = sem.shape[0]
    valid = (gt >= 0) & (gt < S)
    labels = torch.argmax(sem, dim=0)
    return int(valid.sum()), int((~valid & (gt != -1)).sum()), int(((labels == gt) & valid).sum()), labels
