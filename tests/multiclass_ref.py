"""float64 restatement of the multi-label and multi-class losses (smp 0.3-0.5 defaults: from_logits=True, smooth=0, eps=1e-7,
log_loss=False, dims (0, 2), mean over classes) in closed form: the per-class sums and the analytic gradient that the HIP kernels
compute.  tests/test_multiclass_cpu.py checks it against torch autograd of the smp formulas; the GPU tests compare the kernels to it."""
import torch

EPS = 1e-7


def _dice_terms(p, onehot, w_dice):
    """p, onehot: float64 [N,C,HW].  Returns the Dice loss and dDice/dp (times w_dice)."""
    C = p.shape[1]
    inter = (p * onehot).sum(dim=(0, 2))
    card = (p + onehot).sum(dim=(0, 2))
    tsum = onehot.sum(dim=(0, 2))
    den = card.clamp_min(EPS)
    mask = (tsum > 0).double()
    dice = ((1 - 2 * inter / den) * mask).mean()
    ky = -2 * w_dice * mask / (C * den)
    k0 = torch.where(card > EPS, 2 * w_dice * mask * inter / (C * den * den), torch.zeros_like(card))
    g = ky.view(1, C, 1) * onehot + k0.view(1, C, 1)
    return dice, g


def multilabel(x, y, w_bce=1.0, w_dice=1.0):
    """BCEWithLogitsLoss()(x, y) + DiceLoss("multilabel")(x, y); x, y [N,C,H,W].  Returns (total, bce, dice, dlogits) in float64."""
    shape = x.shape
    N, C = shape[0], shape[1]
    x = x.double().reshape(N, C, -1)
    y = y.double().expand(shape).reshape(N, C, -1)
    p = torch.sigmoid(x)
    bce = (x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
    dice, g = _dice_terms(p, y, w_dice)
    dl = w_bce * (p - y) / x.numel() + g * p * (1 - p)
    return w_bce * bce + w_dice * dice, bce, dice, dl.reshape(shape)


def multiclass(x, t, w_ce=1.0, w_dice=1.0):
    """CrossEntropyLoss()(x, t) + DiceLoss("multiclass")(x, t); x [N,C,H,W], t int64 [N,H,W].  Returns (total, ce, dice, dlogits)."""
    shape = x.shape
    N, C = shape[0], shape[1]
    x = x.double().reshape(N, C, -1)
    t = t.reshape(N, -1)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    onehot = torch.nn.functional.one_hot(t, C).permute(0, 2, 1).double()
    ce = -(logp * onehot).sum(dim=1).mean()
    dice, g = _dice_terms(p, onehot, w_dice)
    count = N * x.shape[2]
    dl = w_ce * (p - onehot) / count + p * (g - (p * g).sum(dim=1, keepdim=True))
    return w_ce * ce + w_dice * dice, ce, dice, dl.reshape(shape)
