"""profiles/seglosses: the configurable loss (vk.seglosses, csrc/seg_loss.hip) beside the existing loss kernels, bs 32, 512 x 512,
classes 1, 4 and 16, one process, the two sides alternating, vk_prof family times (device events around each launch family).

  1. seg_loss with pix + dice only beside the existing bce_dice_loss / multilabel_loss / multiclass_loss computing the same loss, on the
     same logits; the existing kernel's own max - min over the repetitions is the margin.
  2. the five-term sum beside pix + dice (cost is per pass, not per term).
  3. bytes moved from shapes (reduce: x + target; backward: x + target + dlogits) over the family time, against the 6.29 TB/s copy rate.
  4. the fused bf16 step loss_and_backward(loss=0.5 * Focal + Tversky) beside the default step, ms/step (with FusedAdamW.step).

  python tools/seglosses_step.py [--reps 7] [--quick]"""
import argparse
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
Ls = vk.seglosses

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--quick", action="store_true", help="one repetition, no step timing (for a kernel trace)")
args = ap.parse_args()
REPS = 1 if args.quick else max(5, args.reps)

dev = torch.device("cuda:0")
N, S = 32, 512
HBM_TBPS = 6.29          # measured copy rate (MI355X_MICROARCH.md)
L = vk.lib()
torch.manual_seed(0)


def family_ms(fn, tag):
    """time of launch family `tag` over one call of fn (device events recorded by the library)"""
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.vk_prof_enable(0)
    tab = vk._lib.prof_collect()
    assert set(tab) == {tag}, sorted(tab)
    return tab[tag]["ms"]


def five(mode):
    px = Ls.SoftCrossEntropyLoss(smooth_factor=0.1, ignore_index=None) if mode == "multiclass" else \
        Ls.SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=None)
    return (px + 0.5 * Ls.FocalLoss(mode, alpha=0.25) + Ls.DiceLoss(mode) + 0.7 * Ls.JaccardLoss(mode, smooth=1.0)
            + 1.3 * Ls.TverskyLoss(mode, alpha=0.3, beta=0.7, gamma=1.5))


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


print(f"loss kernels on fp32 logits [{N}, C, {S}, {S}] with gradient, {REPS} alternating repetitions after one warm-up; median [min, max] ms")
print("  C  mode        existing family              ms                    | seg_loss pix+dice ms            | seg_loss five terms ms"
      "         | bytes    of the floor's rate (pix+dice, five)")
CASES = [(1, "binary"), (4, "multilabel"), (4, "multiclass"), (16, "multilabel"), (16, "multiclass")]
for C, mode in CASES:
    x = (3 * torch.randn(N, C, S, S, device=dev)).requires_grad_()
    if mode == "multiclass":
        t = torch.randint(0, C, (N, S, S), device=dev)
        old, old_tag = vk.multiclass.CEDiceLoss(), "multiclass_loss"
        new = Ls.CrossEntropyLoss() + Ls.DiceLoss(mode)
        nbytes = N * S * S * (2 * (4 * C + 8) + 4 * C)
    else:
        t = (torch.rand(N, C, S, S, device=dev) < 0.05).float()
        old, old_tag = vk.multiclass.BCEDiceLoss(mode), ("bce_dice_loss" if C == 1 else "multilabel_loss")
        new = Ls.BCEWithLogitsLoss() + Ls.DiceLoss(mode)
        nbytes = N * S * S * C * (2 * (4 + 4) + 4)
    sum5 = five(mode)
    sides = [(old, old_tag), (new, "seg_loss"), (sum5, "seg_loss")]
    for fn, tag in sides:                        # warm-up
        family_ms(lambda: fn(x, t), tag)
    ms = [[] for _ in sides]
    for _ in range(REPS):
        for i, (fn, tag) in enumerate(sides):
            ms[i].append(family_ms(lambda: fn(x, t), tag))
    (a, a0, a1), (b, b0, b1), (c, c0, c1) = (stats(v) for v in ms)
    floor = nbytes / (HBM_TBPS * 1e12) * 1e3
    print(f"  {C:2d} {mode:10s}  {old_tag:16s} {a:8.4f} [{a0:.4f}, {a1:.4f}] | {b:8.4f} [{b0:.4f}, {b1:.4f}] | {c:8.4f} [{c0:.4f}, {c1:.4f}]"
          f" | {nbytes / 1e6:7.1f} MB  {100 * floor / b:5.1f} %  {100 * floor / c:5.1f} %   (existing {100 * floor / a:5.1f} %)", flush=True)
    del x, t

if not args.quick:
    print(f"\nfused step, bf16, bs {N}, {S}^2: loss_and_backward + FusedAdamW.step, ms/step; 10 steps per repetition, {REPS} alternating repetitions")
    xin = torch.randn(N, 3, S, S, device=dev)
    for C in (1, 4, 16):
        mode = "binary" if C == 1 else "multiclass"
        model = vk.multiclass.Unet(encoder_weights=None, classes=C).to(dev).train()
        opt = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
        t = (torch.rand(N, 1, S, S, device=dev) < 0.05).float() if C == 1 else torch.randint(0, C, (N, S, S), device=dev)
        loss = 0.5 * Ls.FocalLoss(mode) + Ls.TverskyLoss(mode, alpha=0.3, beta=0.7)

        def step(kw):
            opt.zero_grad(set_to_none=True)
            model.loss_and_backward(xin, t, dtype=torch.bfloat16, **kw)
            opt.step()

        def timed(kw, steps=10):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(kw)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / steps

        sides = [dict(mode=None if C == 1 else mode), dict(loss=loss)]
        for kw in sides:
            for _ in range(3):
                step(kw)
        ms = [[], []]
        for _ in range(REPS):
            for i, kw in enumerate(sides):
                ms[i].append(timed(kw))
        (a, a0, a1), (b, b0, b1) = stats(ms[0]), stats(ms[1])
        print(f"  C={C:2d}  default step {a:8.3f} [{a0:.3f}, {a1:.3f}]   loss=0.5*Focal+Tversky {b:8.3f} [{b0:.3f}, {b1:.3f}]   ({b - a:+.3f} ms)", flush=True)
        del model, opt
