"""profiles/keypoints_loss: vk_kp_loss (csrc/kp_loss.hip), event-timed on one MI355X, the fused step with the new loss sum against the
same step with the recipe of profiles/keypoints, and that page's 400-step run repeated with the new loss.

(a) vk_kp_loss at 32 x 2 x 512 x 512 with both masks set (plane 0 BCE, plane 1 heat): values only, with the gradient written, and
with the gradient added (accumulate), next to the floor its bytes give at the measured HBM copy rate of 6.29 TB/s: the reduce reads 8
bytes per entry, the backward reads 8 and writes 4, plus 4 read with accumulate.  Kernel times come from the library's own per-launch
events (vk_prof_enable), median (min .. max) of 5 rounds of 20 calls.

(b) The fused bf16 step of vk.multiclass.Unet(classes=2), batch 32 at 512 x 512, with PlaneBCE([0]) + DiceLoss("multilabel",
classes=[0]) + w HeatmapFocalLoss([1]) (vk_unet_loss_kp) against the same step with SoftBCEWithLogitsLoss(pos_weight=[1, 20]) +
DiceLoss("multilabel", classes=[0]) (vk_unet_loss_cfg), both from this library, as interleaved pairs of timed windows.

(c) ``--train STEPS`` (0 skips it): the run of tools/keypoints_step.py (b) with the same seeds, scenes and read-out, and the new loss
with the heat term weighted by ``--w-heat`` (``--only-train`` skips (a) and (b), for a run at another weight).
These are numbers on synthetic scenes, and no claim about real micrographs."""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib
K = vk.keypoints
Ls = vk.seglosses

ap = argparse.ArgumentParser()
ap.add_argument("--train", type=int, default=400)
ap.add_argument("--val", type=int, default=64)
ap.add_argument("--pos-weight", type=float, default=20.0, help="of the recipe this is compared with")
ap.add_argument("--w-heat", type=float, default=1.0)
ap.add_argument("--sigma", type=float, default=2.0)
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--steps", type=int, default=30, help="fused steps per timed window of (b)")
ap.add_argument("--only-train", action="store_true", help="skip (a) and (b): only the training run of (c), for another --w-heat")
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the MI355X"
dev = torch.device("cuda:0")
S, BATCH = 512, 32
REPS, ROUNDS = 20, 5
HBM = 6.29e12                                # bytes/s, float4 copy


def kernel_rounds(fn, tag, reps=REPS):
    """Median (min .. max) over ROUNDS of the mean kernel time of `reps` launches of family `tag`, in us."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(ROUNDS):
        L.prof_collect()
        L.lib().vk_prof_enable(1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        L.lib().vk_prof_enable(0)
        v.append(L.prof_collect()[tag]["ms"] / reps * 1e3)
    v.sort()
    return v[len(v) // 2], v[0], v[-1]


def new_loss():
    return (K.PlaneBCE([0]) + Ls.DiceLoss("multilabel", classes=[0])
            + args.w_heat * K.HeatmapFocalLoss([1], pos_threshold=K.positive_threshold(args.sigma)))


def old_loss():
    return Ls.SoftBCEWithLogitsLoss(ignore_index=None, pos_weight=[1.0, args.pos_weight]) + Ls.DiceLoss("multilabel", classes=[0])


ds = vk.MicrographDataset(4096, size=S, seed=0, device=dev)


def measure_kernel_and_step():
    """(a) and (b)"""
    x0, y0, _ = ds.batch(list(range(BATCH)))
    y2 = K.make_targets(y0, sigma=args.sigma)
    logits = torch.randn(BATCH, 2, S, S, device=dev) * 3.0
    dl = torch.zeros_like(logits)
    kp = (K.PlaneBCE([0]) + K.HeatmapFocalLoss([1], pos_threshold=K.positive_threshold(args.sigma)))
    cfg = kp.kp_cfg(2)
    HW = S * S
    ws = kp.workspace(BATCH, 2, HW, dev)
    out = torch.zeros(8, device=dev)
    pos = torch.zeros(16, dtype=torch.int64, device=dev)
    entries = BATCH * 2 * HW

    def call(grad, acc):
        L.check(L.lib().vk_kp_loss(cfg, BATCH, 2, HW, logits.data_ptr(), y2.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), pos.data_ptr(),
                                   dl.data_ptr() if grad else None, 1.0, acc, L.current_stream()), "vk_kp_loss")

    print(f"vk_kp_loss on {BATCH} x 2 x {S} x {S} ({entries / 1e6:.1f} M entries; plane 0 BCE, plane 1 heat with alpha 2, beta 4, threshold "
          f"{cfg.pos_threshold:.4f}); median (min .. max) of {ROUNDS} rounds x {REPS} calls; floors at {HBM / 1e12:.2f} TB/s")
    for name, grad, acc, nbytes in (("values only (reduce, finalize)", False, 0, 8.0 * entries),
                                    ("with the gradient written", True, 0, 20.0 * entries),
                                    ("with the gradient added (accumulate)", True, 1, 24.0 * entries)):
        k = kernel_rounds(lambda: call(grad, acc), "kp_loss")
        floor = nbytes / HBM * 1e6
        print(f"  {name:38s}: {k[0]:7.1f} us ({k[1]:.1f} .. {k[2]:.1f}); {nbytes / 1e6:6.1f} MB = {nbytes / k[0] / 1e6:5.2f} TB/s, byte floor "
              f"{floor:5.1f} us ({k[0] / floor:4.2f} x)")
    call(False, 0)
    torch.cuda.synchronize()
    print(f"  values {out[:3].tolist()}, positives of plane 1: {int(pos[1])}", flush=True)

    # ---- (b) the fused step, interleaved pairs
    vk.seed_everything(42)
    model = vk.multiclass.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=2, activation=None).to(dev).train()
    opt = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
    losses = {"new sum (vk_unet_loss_kp)": new_loss(), "recipe of profiles/keypoints (vk_unet_loss_cfg)": old_loss()}

    def window(loss, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            model.loss_and_backward(x0, y2, dtype=torch.bfloat16, loss=loss)
            opt.step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for loss in losses.values():
        window(loss, 5)                                       # warm-up of either route
    times = {k: [] for k in losses}
    for _ in range(args.pairs):
        for k, loss in losses.items():
            times[k].append(window(loss, args.steps))
    print(f"(b) fused bf16 step (forward, loss, backward, AdamW) of resnet34 with classes=2, batch {BATCH} at {S} x {S}: {args.pairs} interleaved "
          f"pairs of windows of {args.steps} steps")
    for k, v in times.items():
        s = sorted(v)
        print(f"  {k:48s}: median {s[len(s) // 2]:.3f} ms per step ({s[0]:.3f} .. {s[-1]:.3f})")
    a, b = (np.array(v) for v in times.values())
    r = np.sort(a / b)
    print(f"  new / recipe per pair: median {r[len(r) // 2]:.4f} ({r[0]:.4f} .. {r[-1]:.4f})", flush=True)


if not args.only_train:
    measure_kernel_and_step()

# ---- (c) the 400-step run of tools/keypoints_step.py (b), with the new loss
if args.train <= 0:
    print("(c) skipped: --train 0")
    sys.exit(0)
vk.seed_everything(42)
model = vk.multiclass.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=2, activation=None).to(dev).train()
opt = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
loss = new_loss()
aug = vk.AugmentSampler(seed=1)
step, t0, seen, epoch = 0, time.perf_counter(), [], 0
while step < args.train:
    for x, yy, _ in K.with_targets(ds.loader(BATCH, shuffle=True, sampler=aug, seed=epoch), sigma=args.sigma):
        if x.shape[0] != BATCH or step >= args.train:
            break
        opt.zero_grad(set_to_none=True)
        o = model.loss_and_backward(x, yy, dtype=torch.bfloat16, loss=loss)
        opt.step()
        step += 1
        if step % 50 == 0 or step == args.train:
            seen.append((step, [float(v) for v in o[[0, 3, 7, 8]]]))
    epoch += 1
torch.cuda.synchronize()
print(f"(c) {step} bf16 training steps of resnet34 with classes=2, batch {BATCH}, on MicrographDataset(seed=0).loader with AugmentSampler(seed=1), "
      f"targets by make_targets (sigma {args.sigma}), PlaneBCE([0]) + DiceLoss('multilabel', classes=[0]) + {args.w_heat:g} HeatmapFocalLoss([1], "
      f"pos_threshold={K.positive_threshold(args.sigma):.4f}), AdamW lr 5e-5 wd 1e-4: {time.perf_counter() - t0:.1f} s with the host draws")
print("  step: total, dice, heat, plane_bce: " + "; ".join(f"{s}: " + ", ".join(f"{v:.4f}" for v in vals) for s, vals in seen), flush=True)

model.eval()
val = vk.MicrographDataset(args.val, size=S, seed=1, device=dev)


def diag_errors(rows_per_map, truths):
    """Mean |d_mean - true| / true over the truth indentations whose box holds exactly one detection centre; (mean, matched, truths)."""
    errs, n_t = [], 0
    for rows, tr in zip(rows_per_map, truths):
        n_t += len(tr)
        for t in tr:
            bx0, by0, bx1, by1 = t["box"]
            hit = [d for (cx, cy, d) in rows if bx0 <= cx <= bx1 and by0 <= cy <= by1]
            if len(hit) == 1:
                errs.append(abs(hit[0] - t["d_mean"]) / t["d_mean"])
    return (float(np.mean(errs)) if errs else float("nan")), len(errs), n_t


plain, sub, kpp, kpc, truths, dices = [], [], [], [], [], []
flag_count, n_vert = {k: 0 for k in K.FLAGS}, 0
vm = dict(tp=0, fp=0, fn=0)
dist = []
with torch.no_grad():
    for a0 in range(0, args.val, BATCH):
        ids = list(range(a0, min(a0 + BATCH, args.val)))
        x, y, _ = val.batch(ids)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            probs2 = torch.sigmoid(model(x).float())
        p = probs2[:, 0].contiguous()
        d, _ = vk.seg_metrics(probs2[:, :1].contiguous(), y, from_logits=False)
        dices.append((float(d), len(ids)))
        tr = [val.truth(i) for i in ids]
        truths += tr
        plain += [[(float(r["cx"]), float(r["cy"]), float(r["d_mean"])) for r in rows if r["valid"]] for rows in vk.geometry.detect(p, fit="quad").records()]
        sub += [[(q["center"][0], q["center"][1], q["d_mean"]) for q in rows] for rows in vk.subpix.postprocess(p, fit="quad", method="lines")[1]]
        for method, dst in (("parabola", kpp), ("centroid", kpc)):
            lists = K.postprocess(probs2, fit="quad", method=method)[1]
            dst += [[(q["center"][0], q["center"][1], q["d_mean"]) for q in rows] for rows in lists]
            if method == "parabola":
                for rows in lists:
                    for q in rows:
                        n_vert += 4
                        for name, bit in K.FLAGS.items():
                            flag_count[name] += int(((q["subpix_flags"] & bit) != 0).sum())
        for recs, t in zip(K.peaks(probs2[:, 1]).records(), tr):
            gt = np.concatenate([q["vertices"] for q in t]) if t else np.zeros((0, 2))
            m = K.vertex_metrics(recs, gt, tol_px=2.0)
            for k_ in vm:
                vm[k_] += m[k_]
            if m["tp"]:
                dist.append((m["mean_dist"], m["tp"]))
dice = sum(d * n for d, n in dices) / sum(n for _, n in dices)
md = sum(d * n for d, n in dist) / max(sum(n for _, n in dist), 1)
print(f"validation on {args.val} held-out scenes (seed 1, {sum(len(t) for t in truths)} indentations): Dice of plane 0 {dice:.4f}; vertex peaks "
      f"(min_peak 0.3, r 2) within 2 px of a true vertex: tp {vm['tp']} fp {vm['fp']} fn {vm['fn']}, mean distance of the matched {md:.3f} px")
print(f"  vk.keypoints.refine flags over {n_vert} vertices: " + ", ".join(f"{k_} {v}" for k_, v in flag_count.items())
      + (f" (at_edge share {flag_count['at_edge'] / n_vert:.3f})" if n_vert else ""))
for name, rows in (("plain quadrilateral fit", plain), ("vk.subpix (lines)", sub), ("vk.keypoints.refine (parabola)", kpp),
                   ("vk.keypoints.refine (centroid)", kpc)):
    e, k_, n = diag_errors(rows, truths)
    print(f"  diagonal error against truth(), {name}: mean |d - d_true| / d_true = {e:.5f} over {k_} of {n} indentations", flush=True)
print("These are numbers on synthetic scenes after a short run from random weights: no claim about real micrographs.", flush=True)
