"""profiles/keypoints: the vertex heatmap kernels (vk.keypoints, csrc/keypoints.hip), event-timed on one MI355X, and a first accuracy
figure on held-out synthetic scenes, with the method of profiles/micrographs/README.md.

(a) vk_kp_targets, vk_kp_peaks and vk_kp_refine for 32 maps of 512 x 512 at SceneSampler's defaults, next to their byte floors at the
measured HBM copy rate of 6.29 TB/s (targets: 4 bytes written per pixel; peaks: 4 bytes read per pixel; refine: its records), the table
read from memory against the table staged in LDS, and make_targets as a share of a training step.  Kernel times come from the
library's own per-launch events (vk_prof_enable), whole calls from device events round them.  No gate: the kernels have no parent.

(b) ``--train STEPS`` (0 skips it): the run of tools/micrographs_step.py (b) with the same seeds, repeated with
vk.multiclass.Unet(classes=2), targets by make_targets on the augmented masks and SoftBCEWithLogitsLoss(pos_weight=[1, w]) +
DiceLoss("multilabel", classes=[0]); then the diagonal error against truth() for the plain quadrilateral fit, vk.subpix (lines) and
vk.keypoints.refine from the same model.  These are numbers on synthetic scenes, and no claim about real micrographs."""
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
ap.add_argument("--pos-weight", type=float, default=20.0)
ap.add_argument("--sigma", type=float, default=2.0)
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


def kernel_rounds(fn, tag, reps=REPS):
    """Median (min .. max) over ROUNDS of the mean kernel time of `reps` launches of family `tag`, in us."""
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


# ---- (a) kernel times
ds = vk.MicrographDataset(4096, size=S, seed=0, device=dev)
idx = list(range(BATCH))
mask = ds.masks(idx).clone()
dets = vk.instances.detect_gt(mask, fit="quad", fit_outset_px=0)
n_rec = int(dets.counts.clamp(max=dets.max_components).sum())
print(f"{BATCH} maps of {S} x {S}, SceneSampler defaults: {n_rec} records ({4 * n_rec} vertices), sigma {args.sigma} "
      f"(table of {K.gaussian_table(args.sigma).numel()} entries); median (min .. max) of {ROUNDS} rounds x {REPS} calls")
px_bytes = 4.0 * BATCH * S * S
floor = px_bytes / HBM * 1e6
heat = K.targets(dets, sigma=args.sigma)
for name, tab in (("table in memory", "memory"), ("table in LDS", "lds"), ("library's choice", None)):
    if tab == "lds" and K.gaussian_table(args.sigma).numel() > L.VK_KP_TABLE_LDS_MAX:
        print(f"vk_kp_targets, {name}: the table does not fit")
        continue
    k = kernel_rounds(lambda: K.targets(dets, sigma=args.sigma, out=heat, table=tab), "kp_targets")
    print(f"vk_kp_targets, {name:17s}: kernel {k[0]:7.1f} us ({k[1]:.1f} .. {k[2]:.1f}) = {px_bytes / k[0] / 1e6:5.2f} TB/s of {px_bytes / 1e6:5.1f} MB "
          f"written, byte floor {floor:5.1f} us ({k[0] / floor:5.1f} x)")
y2 = torch.empty(BATCH, 2, S, S, device=dev)
k = kernel_rounds(lambda: K.targets(dets, sigma=args.sigma, out=y2[:, 1]), "kp_targets")
print(f"vk_kp_targets into plane 1 of [N, 2, H, W]: kernel {k[0]:7.1f} us ({k[1]:.1f} .. {k[2]:.1f})")
k = kernel_rounds(lambda: K.peaks(heat), "kp_peaks")
w = rounds(lambda: K.peaks(heat))
print(f"vk_kp_peaks (min_peak 0.3, r 2, three launches): kernels {k[0]:7.1f} us ({k[1]:.1f} .. {k[2]:.1f}), byte floor {floor:5.1f} us "
      f"({k[0] / floor:5.1f} x); whole call with its allocations {w[0]:7.1f} us; {int(K.peaks(heat).counts.sum())} peaks")
noise = torch.rand(BATCH, S, S, device=dev)
k = kernel_rounds(lambda: K.peaks(noise, min_peak=0.0), "kp_peaks")
print(f"vk_kp_peaks on uniform noise with min_peak 0 (every pixel tests its window): kernels {k[0]:7.1f} us ({k[1]:.1f} .. {k[2]:.1f}), "
      f"{k[0] / floor:5.1f} x the floor")
for method in ("parabola", "centroid"):
    k = kernel_rounds(lambda: K.refine(dets, heat, method=method), "kp_refine")
    rec_bytes = BATCH * dets.max_components * 200
    print(f"vk_kp_refine ({method}, search 6): kernel {k[0]:7.1f} us ({k[1]:.1f} .. {k[2]:.1f}) for {BATCH} x {dets.max_components} slots, "
          f"{n_rec} used; its records are {rec_bytes / 1e3:.0f} KB ({rec_bytes / HBM * 1e6:.2f} us at the copy rate): launch-bound")
ymask = mask[:, None].float()
w = rounds(lambda: K.make_targets(ymask, sigma=args.sigma))
print(f"make_targets (detect_gt, targets, the plane copy), whole call: {w[0]:7.1f} us ({w[1]:.1f} .. {w[2]:.1f}) = {w[0] / 10600 * 100:.1f} % of a "
      f"10.6 ms training step", flush=True)

# ---- (b) accuracy on held-out scenes
if args.train <= 0:
    print("(b) skipped: --train 0")
    sys.exit(0)
vk.seed_everything(42)
model = vk.multiclass.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=2, activation=None).to(dev).train()
opt = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
loss = Ls.SoftBCEWithLogitsLoss(ignore_index=None, pos_weight=[1.0, args.pos_weight]) + Ls.DiceLoss("multilabel", classes=[0])
aug = vk.AugmentSampler(seed=1)
step, t0, losses, epoch = 0, time.perf_counter(), [], 0
while step < args.train:
    for x, y2, _ in K.with_targets(ds.loader(BATCH, shuffle=True, sampler=aug, seed=epoch), sigma=args.sigma):
        if x.shape[0] != BATCH or step >= args.train:
            break
        opt.zero_grad(set_to_none=True)
        out = model.loss_and_backward(x, y2, dtype=torch.bfloat16, loss=loss)
        opt.step()
        step += 1
        if step % 50 == 0 or step == args.train:
            losses.append((step, float(out[0])))
    epoch += 1
torch.cuda.synchronize()
print(f"(b) {step} bf16 training steps of resnet34 with classes=2, batch {BATCH}, on MicrographDataset(seed=0).loader with AugmentSampler(seed=1), "
      f"targets by make_targets (sigma {args.sigma}), SoftBCEWithLogitsLoss(pos_weight=[1, {args.pos_weight:g}]) + DiceLoss('multilabel', classes=[0]), "
      f"AdamW lr 5e-5 wd 1e-4: {time.perf_counter() - t0:.1f} s with the host draws; loss " + ", ".join(f"{s}: {v:.4f}" for s, v in losses), flush=True)

model.eval()
val = vk.MicrographDataset(args.val, size=S, seed=1, device=dev)


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


plain, sub, kp, kpc, truths, dices = [], [], [], [], [], []
flag_count, n_vert = {k: 0 for k in K.FLAGS}, 0
vm = dict(tp=0, fp=0, fn=0)
with torch.no_grad():
    for a in range(0, args.val, BATCH):
        ids = list(range(a, min(a + BATCH, args.val)))
        x, y, _ = val.batch(ids)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            probs2 = torch.sigmoid(model(x).float())
        p = probs2[:, 0].contiguous()
        d, _ = vk.seg_metrics(probs2[:, :1].contiguous(), y, from_logits=False)
        dices.append((float(d), len(ids)))
        tr = [val.truth(i) for i in ids]
        truths += tr
        plain += [[(float(r["cx"]), float(r["cy"]), float(r["d_mean"])) for r in rows if r["valid"]] for rows in vk.geometry.detect(p, fit="quad").records()]
        sub += [[(d["center"][0], d["center"][1], d["d_mean"]) for d in rows] for rows in vk.subpix.postprocess(p, fit="quad", method="lines")[1]]
        for method, dst in (("parabola", kp), ("centroid", kpc)):
            lists = K.postprocess(probs2, fit="quad", method=method)[1]
            dst += [[(d["center"][0], d["center"][1], d["d_mean"]) for d in rows] for rows in lists]
            if method == "parabola":
                for rows in lists:
                    for d in rows:
                        n_vert += 4
                        for name, bit in K.FLAGS.items():
                            flag_count[name] += int(((d["subpix_flags"] & bit) != 0).sum())
        for recs, t in zip(K.peaks(probs2[:, 1]).records(), tr):
            gt = np.concatenate([q["vertices"] for q in t]) if t else np.zeros((0, 2))
            m = K.vertex_metrics(recs, gt, tol_px=2.0)
            for k_ in vm:
                vm[k_] += m[k_]
dice = sum(d * n for d, n in dices) / sum(n for _, n in dices)
print(f"validation on {args.val} held-out scenes (seed 1, {sum(len(t) for t in truths)} indentations): Dice of plane 0 {dice:.4f}; vertex peaks "
      f"(min_peak 0.3, r 2) within 2 px of a true vertex: tp {vm['tp']} fp {vm['fp']} fn {vm['fn']}")
print(f"  vk.keypoints.refine flags over {n_vert} vertices: " + ", ".join(f"{k_} {v}" for k_, v in flag_count.items()))
for name, rows in (("plain quadrilateral fit", plain), ("vk.subpix (lines)", sub), ("vk.keypoints.refine (parabola)", kp),
                   ("vk.keypoints.refine (centroid)", kpc)):
    e, k_, n = diag_errors(rows, truths)
    print(f"  diagonal error against truth(), {name}: mean |d - d_true| / d_true = {e:.5f} over {k_} of {n} indentations", flush=True)
print("These are numbers on synthetic scenes after a short run from random weights: no claim about real micrographs.", flush=True)
