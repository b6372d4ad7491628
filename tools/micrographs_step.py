"""profiles/micrographs: the synthetic micrograph renderer (vk.micrographs), event-timed on one MI355X, and a first accuracy figure on
held-out synthetic scenes.

(a) vk_mg_render for 32 scenes of 512 x 512 at SceneSampler's defaults, next to vk_augment_batch over the buffers it filled (same box, same
run) and next to its byte floor: 4 output bytes per pixel at the measured HBM copy rate of 6.29 TB/s.  Kernel times come from the
library's own per-launch events (vk_prof_enable), whole calls from device events round them.  No gate: the kernel has no parent.

(b) ``--train STEPS`` (0 skips it): STEPS bf16 training steps of the resnet34 model on MicrographDataset.loader (batch 32, AugmentSampler, the
reference's BCE + Dice and AdamW lr 5e-5, weight decay 1e-4), then validation on held-out items of another seed: Dice, PQ and mean_rel_d
of ObjectMetrics against detect_gt of the exact masks, and the diagonal error against truth() for the plain quadrilateral fit, with
vk.subpix and with vk.zoom.  These are numbers on synthetic scenes, and no claim about real micrographs."""
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
M = vk.micrographs

ap = argparse.ArgumentParser()
ap.add_argument("--train", type=int, default=400)
ap.add_argument("--val", type=int, default=64)
args = ap.parse_args()

dev = torch.device("cuda:0")
S, BATCH = 512, 32
REPS, ROUNDS = 20, 5
HBM = 6.29e12                                # bytes/s, float4 copy


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


def rounds(fn, reps=REPS):
    v = sorted(timed(fn, reps) for _ in range(ROUNDS))
    return v[len(v) // 2], v[0], v[-1]


def kernel_times(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    L.lib().vk_prof_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {k: v["ms"] / reps * 1e3 for k, v in L.prof_collect().items()}
    L.lib().vk_prof_enable(0)
    return out


# ---- (a) render time
ds = vk.MicrographDataset(4096, size=S, seed=0, device=dev)
idx = list(range(BATCH))
t0 = time.perf_counter()
scenes = np.stack([ds.scene(i) for i in idx])
host_ms = (time.perf_counter() - t0) * 1e3
n_ind, n_scr = scenes["n_indents"].sum(), scenes["n_scratches"].sum()
print(f"{BATCH} scenes of {S} x {S} at the sampler's defaults: {n_ind} indentations, {n_scr} scratches, {scenes['n_blobs'].sum()} blobs, "
      f"{scenes['n_rects'].sum()} rects, blur radii {np.bincount(scenes['blur_r'], minlength=4).tolist()}; host draws {host_ms:.1f} ms "
      f"({host_ms / BATCH * 1e3:.0f} us per scene); median (min .. max) of {ROUNDS} rounds x {REPS} calls")
by = 4.0 * BATCH * S * S
kt = kernel_times(lambda: M.render(scenes, S, dev))["mg_render"]
whole = rounds(lambda: M.render(scenes, S, dev))
print(f"vk_mg_render: kernel {kt:7.1f} us = {by / kt / 1e6:5.2f} TB/s of {by / 1e6:5.1f} MB written, byte floor {by / HBM * 1e6:5.1f} us "
      f"({kt / (by / HBM * 1e6):5.1f} x); whole call with the record copy {whole[0]:7.1f} us ({whole[1]:.1f} .. {whole[2]:.1f})")
blank = np.stack([M.blank_scene() for _ in idx])
kb = kernel_times(lambda: M.render(blank, S, dev))["mg_render"]
print(f"vk_mg_render, scenes without records or optics: kernel {kb:7.1f} us ({kb / (by / HBM * 1e6):5.1f} x the floor): the cost of the tile "
      f"machinery alone")
sm = vk.AugmentSampler(seed=0)
draws = [sm.sample() for _ in idx]
ka = kernel_times(lambda: ds.batch(idx, draws=draws))
wb = rounds(lambda: ds.batch(idx, draws=draws))
print(f"vk_augment_batch over the rendered buffers, AugmentSampler(seed=0) draws ({[d['photo'] for d in draws].count(2)} CLAHE, "
      f"{sum(d['rotate'] for d in draws)} rotated): kernels {ka['augment']:7.1f} us; mg_render inside the same calls {ka['mg_render']:7.1f} us")
print(f"MicrographDataset.batch, whole call (host draws of {BATCH} scenes, render, augment): {wb[0]:7.1f} us ({wb[1]:.1f} .. {wb[2]:.1f}) "
      f"= {wb[0] / 10600 * 100:.1f} % of a 10.6 ms training step", flush=True)

# ---- (b) accuracy on held-out scenes
if args.train <= 0:
    print("(b) skipped: --train 0")
    sys.exit(0)
vk.seed_everything(42)
model = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev).train()
opt = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
aug = vk.AugmentSampler(seed=1)
step, t0, losses = 0, time.perf_counter(), []
epoch = 0
while step < args.train:
    for x, y, _ in ds.loader(BATCH, shuffle=True, sampler=aug, seed=epoch):
        if x.shape[0] != BATCH or step >= args.train:
            break
        opt.zero_grad(set_to_none=True)
        out = model.loss_and_backward(x, y, dtype=torch.bfloat16)
        opt.step()
        step += 1
        if step % 50 == 0 or step == args.train:
            losses.append((step, float(out[0])))
    epoch += 1
torch.cuda.synchronize()
print(f"(b) {step} bf16 training steps of resnet34, batch {BATCH}, on MicrographDataset(seed=0).loader with AugmentSampler(seed=1), BCE + Dice, "
      f"AdamW lr 5e-5 wd 1e-4: {time.perf_counter() - t0:.1f} s with the host draws; loss " + ", ".join(f"{s}: {v:.4f}" for s, v in losses), flush=True)

model.eval()
val = vk.MicrographDataset(args.val, size=S, seed=1, device=dev)
om = vk.ObjectMetrics(fit="quad")
dices = []


def diag_errors(rows_per_map, truths):
    """Mean |d_mean - true| / true over the truth indentations whose box holds exactly one detection centre; (mean, matched, truths)."""
    errs, n_t = [], 0
    for rows, tr in zip(rows_per_map, truths):
        n_t += len(tr)
        for t in tr:
            x0, y0, x1, y1 = t["box"]
            hit = [d for (cx, cy, d) in rows if x0 <= cx <= x1 and y0 <= cy <= y1]
            if len(hit) == 1:
                errs.append(abs(hit[0] - t["d_mean"]) / t["d_mean"])
    return (float(np.mean(errs)) if errs else float("nan")), len(errs), n_t


plain, sub, zoomed, truths = [], [], [], []
with torch.no_grad():
    for a in range(0, args.val, BATCH):
        ids = list(range(a, min(a + BATCH, args.val)))
        x, y, _ = val.batch(ids)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            prob = torch.sigmoid(model(x).float())
        d, _ = vk.seg_metrics(prob, y, from_logits=False)
        dices.append((float(d), len(ids)))
        om.update(prob[:, 0], y[:, 0])
        p = prob[:, 0].contiguous()
        truths += [val.truth(i) for i in ids]
        plain += [[(float(r["cx"]), float(r["cy"]), float(r["d_mean"])) for r in rows if r["valid"]] for rows in vk.geometry.detect(p, fit="quad").records()]
        sub += [[(d["center"][0], d["center"][1], d["d_mean"]) for d in rows] for rows in vk.subpix.postprocess(p, fit="quad", method="lines")[1]]
m = om.compute()
dice = sum(d * n for d, n in dices) / sum(n for _, n in dices)
print(f"validation on {args.val} held-out scenes (seed 1, {sum(len(t) for t in truths)} indentations): Dice {dice:.4f}; against detect_gt of the exact "
      f"masks at IoU 0.5: PQ {m['pq'][0]:.4f}, tp {int(m['tp'][0])} fp {int(m['fp'][0])} fn {int(m['fn'][0])}, mean_rel_d {m['mean_rel_d'][0]:.5f}")
for name, rows in (("plain quadrilateral fit", plain), ("vk.subpix (lines)", sub)):
    e, k, n = diag_errors(rows, truths)
    print(f"  diagonal error against truth(), {name}: mean |d - d_true| / d_true = {e:.5f} over {k} of {n} indentations", flush=True)
with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
    for a in range(0, args.val, BATCH):
        ids = list(range(a, min(a + BATCH, args.val)))
        x, _, _ = val.batch(ids)
        p = torch.sigmoid(model(x).float())[:, 0].contiguous()
        imgs = [im.clone() for im in val.images(ids)]
        zoomed += [[(d["center"][0], d["center"][1], d["d_mean"]) for d in rows]
                   for rows in vk.zoom.postprocess(lambda t: model(t).float(), imgs, p, fit="quad", method="lines", S=S)[1]]
e, k, n = diag_errors(zoomed, truths)
print(f"  diagonal error against truth(), vk.zoom (lines): mean |d - d_true| / d_true = {e:.5f} over {k} of {n} indentations")
print("These are numbers on synthetic scenes after a short run from random weights: no claim about real micrographs.", flush=True)
