"""profiles/multiclass_eval: vk.multiclass validation metrics and inference post-processing, event-timed on one MI355X.

Metrics: N = 32, 512 x 512 fp32 logits (the bf16 model's output), C in {2, 4, 16}, both modes, against the HBM floor (bytes the pass
must read at 6.29 TB/s) and against the torch composition a user would otherwise write (argmax / sigmoid, one_hot, products, sums).
Post-processing: 3072 x 2048 and 1280 x 1024 originals from a 512 x 512 C = 4 logit map ("centered" letterbox), labels / masks /
probabilities, against the output write floor and torch's own (softmax / sigmoid, crop, F.interpolate)."""
import importlib
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
M = vk.multiclass

dev = torch.device("cuda:0")
HBM_TBPS = 6.29          # measured copy rate (MI355X_MICROARCH.md)
N, S = 32, 512
REPS, ROUNDS = 20, 3


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3       # us per call


def median_of_rounds(fns):
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            res[k].append(timed(fn))
    return {k: sorted(v)[len(v) // 2] for k, v in res.items()}


def torch_metrics(x, t, mode, thr=0.5, eps=1e-7):
    """What a user writes without vk.multiclass.seg_metrics: per image and class dice / iou, then means."""
    C = x.shape[1]
    if mode == "multiclass":
        pred = F.one_hot(x.argmax(1), C).permute(0, 3, 1, 2).float()
        tgt = F.one_hot(t, C).permute(0, 3, 1, 2).float()
    else:
        pred = (torch.sigmoid(x) > thr).float()
        tgt = t
    inter = (pred * tgt).sum(dim=(2, 3))
    card = pred.sum(dim=(2, 3)) + tgt.sum(dim=(2, 3))
    dice = (2 * inter + eps) / (card + eps)
    iou = (inter + eps) / (card - inter + eps)
    return torch.stack([dice.mean(), iou.mean()])


torch.manual_seed(0)
print("metrics, N = 32, 512^2, fp32 logits: median of %d rounds x %d calls" % (ROUNDS, REPS))
rows = []
for C in (2, 4, 16):
    x = torch.randn(N, C, S, S, device=dev) * 3
    tl = (torch.rand(N, C, S, S, device=dev) < 0.044).float()
    tc = torch.randint(0, C, (N, S, S), device=dev)
    fns = {("multilabel", "vk"): lambda: M.seg_metrics_device(x, tl, "multilabel"),
           ("multilabel", "torch"): lambda: torch_metrics(x, tl, "multilabel"),
           ("multiclass", "vk"): lambda: M.seg_metrics_device(x, tc, "multiclass"),
           ("multiclass", "torch"): lambda: torch_metrics(x, tc, "multiclass")}
    med = median_of_rounds(fns)
    for mode in ("multilabel", "multiclass"):
        nbytes = N * S * S * (4 * C + (4 * C if mode == "multilabel" else 8))
        floor = nbytes / (HBM_TBPS * 1e12) * 1e6
        v, tt = med[(mode, "vk")], med[(mode, "torch")]
        print(f"  C={C:2d} {mode:10s} vk {v:8.1f} us  floor {floor:6.1f} us ({floor / v * 100:5.1f} % of the floor's rate)  "
              f"torch {tt:8.1f} us ({tt / v:5.1f}x)", flush=True)
    del x, tl, tc
    torch.cuda.empty_cache()


def torch_post(lg, meta, what):
    _, geo, (h, w) = meta
    _, nh, nw, top, left = geo
    if what == "labels":
        lab = lg.argmax(0)[top:top + nh, left:left + nw]
        return F.interpolate(lab[None, None].float(), size=(h, w), mode="nearest")[0, 0].to(torch.uint8)
    p = torch.softmax(lg, 0) if what == "probs_multiclass" else torch.sigmoid(lg)
    if what == "masks":
        m = ((p >= 0.5).to(torch.uint8) * 255)[:, top:top + nh, left:left + nw]
        return F.interpolate(m[None].float(), size=(h, w), mode="nearest")[0].to(torch.uint8)
    crop = p[:, top:top + nh, left:left + nw]
    return F.interpolate(crop[None], size=(h, w), mode="bilinear", align_corners=False)[0].clamp(0, 1)


print("\npost-processing from a 512^2 C = 4 logit map, 'centered' letterbox: median of %d rounds x %d calls" % (ROUNDS, REPS))
C = 4
lg = torch.randn(C, S, S, device=dev) * 3
for h, w in ((3072, 2048), (1280, 1024)):
    geo = vk.prepost.letterbox_geometry(h, w, S, "centered")
    meta = (geo[0], geo, (h, w))
    fns = {("labels", "vk"): lambda: M.postprocess_labels(lg, meta),
           ("labels", "torch"): lambda: torch_post(lg, meta, "labels"),
           ("masks", "vk"): lambda: M.postprocess_masks(lg, meta),
           ("masks", "torch"): lambda: torch_post(lg, meta, "masks"),
           ("probs_multilabel", "vk"): lambda: M.postprocess_probs(lg, meta, "multilabel"),
           ("probs_multilabel", "torch"): lambda: torch_post(lg, meta, "probs_multilabel"),
           ("probs_multiclass", "vk"): lambda: M.postprocess_probs(lg, meta, "multiclass"),
           ("probs_multiclass", "torch"): lambda: torch_post(lg, meta, "probs_multiclass")}
    med = median_of_rounds(fns)
    for what, out_bytes in (("labels", 1), ("masks", C), ("probs_multilabel", 4 * C), ("probs_multiclass", 4 * C)):
        floor = (h * w * out_bytes + C * geo[1] * geo[2] * 4) / (HBM_TBPS * 1e12) * 1e6
        v, tt = med[(what, "vk")], med[(what, "torch")]
        print(f"  {h}x{w} {what:17s} vk {v:8.1f} us  floor {floor:6.1f} us ({floor / v * 100:5.1f} % of the floor's rate)  "
              f"torch {tt:8.1f} us ({tt / v:5.1f}x)", flush=True)
