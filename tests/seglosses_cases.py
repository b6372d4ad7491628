"""Inputs and the covering set of loss configurations shared by tests/test_seglosses_cpu.py and tests/test_seglosses_gpu.py.

Inputs: logits 3 * randn (seeded); targets with 5 % (binary, multilabel) or uniform (multiclass) foreground, one class absent from
the batch when C > 1, and for the ignore cases 10 % of the entries set to ignore_index = 255.  Everything is drawn on the CPU, so the
CPU reference and the device see the same numbers."""
import torch

IGN = 255
MODE_C = [("binary", 1), ("multilabel", 1), ("multilabel", 4), ("multilabel", 16),
          ("multiclass", 2), ("multiclass", 3), ("multiclass", 5), ("multiclass", 16)]
SHAPES = [(3, 40, 56), (2, 33, 47)]            # HW % 4 == 0: 16-byte path; 33 x 47: scalar path
FOCAL = [(None, 2.0), (0.25, 2.0), (0.25, 1.5), (None, 1.0), (None, 0.0)]


def make_inputs(mode, C, N, H, W, ignore, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 17 * C + H)
    x = 3.0 * torch.randn(N, C, H, W, generator=g)
    absent = 1 if C > 1 else None
    if mode == "multiclass":
        t = torch.randint(0, C - 1, (N, H, W), generator=g)
        t = t + (t >= absent).long()                       # classes 0 .. C-1 without `absent`
        if ignore:
            t[torch.rand(N, H, W, generator=g) < 0.1] = IGN
        return x, t
    y = (torch.rand(N, C, H, W, generator=g) < 0.05).float()
    if absent is not None:
        y[:, absent] = 0.0
    if ignore:
        y[torch.rand(N, C, H, W, generator=g) < 0.1] = float(IGN)
    return x, y


def case_names():
    return (["pix_soft", "pix_nn"] + ["focal%d" % i for i in range(len(FOCAL))]
            + ["dice", "dice_opts", "jaccard", "jaccard_log", "tversky", "tversky_log", "sum5"])


def ignored(name, shape_index):
    """whether this case runs with ignore_index: the five-term sum always, the single terms alternate (and swap with the shape, so
    every term meets ignore_index on one of the two shapes)"""
    if name == "sum5":
        return True
    return (case_names().index(name) + shape_index) % 2 == 0


def build(Ls, name, mode, C, ignore):
    """the loss object of case `name` from the vk.seglosses module `Ls`"""
    ign = IGN if ignore else None
    multiclass = mode == "multiclass"
    pw = [1.0 + 0.5 * c for c in range(C)]
    sub = [0, C - 1]

    def pix_soft():
        if multiclass:
            return Ls.SoftCrossEntropyLoss(smooth_factor=0.1, ignore_index=ign)
        return Ls.SoftBCEWithLogitsLoss(smooth_factor=0.1, pos_weight=torch.tensor(pw).view(1, C, 1, 1), ignore_index=ign)

    def pix_nn():
        if multiclass:
            return Ls.CrossEntropyLoss(ignore_index=ign if ignore else -100, label_smoothing=0.1)
        return Ls.BCEWithLogitsLoss(pos_weight=torch.tensor(pw))

    if name == "pix_soft":
        return pix_soft()
    if name == "pix_nn":
        loss = pix_nn()
        if ignore and not multiclass:            # torch's BCE has no ignore_index of its own: it takes the sum's
            loss = loss + 0.0 * Ls.DiceLoss(mode, ignore_index=ign)
        return loss
    if name.startswith("focal"):
        a, g = FOCAL[int(name[5:])]
        return Ls.FocalLoss(mode, alpha=a, gamma=g, ignore_index=ign)
    if name == "dice":
        return Ls.DiceLoss(mode, ignore_index=ign)
    if name == "dice_opts":
        return Ls.DiceLoss(mode, classes=sub, log_loss=True, smooth=1.0, eps=1e-6, ignore_index=ign)
    if name == "jaccard":
        return Ls.JaccardLoss(mode, smooth=1.0, ignore_index=ign)
    if name == "jaccard_log":
        return Ls.JaccardLoss(mode, log_loss=True, classes=sub, eps=1e-6, ignore_index=ign)
    if name == "tversky":
        return Ls.TverskyLoss(mode, alpha=0.3, beta=0.7, gamma=1.5, ignore_index=ign)
    if name == "tversky_log":
        return Ls.TverskyLoss(mode, log_loss=True, smooth=1.0, ignore_index=ign)
    if name == "sum5":
        px = Ls.SoftCrossEntropyLoss(smooth_factor=0.1, ignore_index=ign) if multiclass else \
            Ls.SoftBCEWithLogitsLoss(smooth_factor=0.1, pos_weight=pw, ignore_index=ign)
        return (px + 0.5 * Ls.FocalLoss(mode, alpha=0.25, gamma=2.0, ignore_index=ign) + Ls.DiceLoss(mode, ignore_index=ign)
                + 0.7 * Ls.JaccardLoss(mode, smooth=1.0, ignore_index=ign)
                + 1.3 * Ls.TverskyLoss(mode, alpha=0.3, beta=0.7, gamma=1.5, ignore_index=ign))
    raise KeyError(name)
