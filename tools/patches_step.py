"""profiles/patches: native-resolution patch training (vk.patches), event-timed on one MI355X.

32 built 3072 x 2048 images (uint8 BGR, a 4.4 % diamond of foreground each), patch 512, batch 32, draws from PatchSampler(seed=0).
Reported: the index build (once), then per batch the origins kernel, the crop kernel (its achieved bytes/s against its algorithmic
bytes, 4 read + 4 written per output pixel) and the augmentation pass, and beside them DeviceDataset.batch — the letterboxed pipeline —
with the same augmentation draws, so the cost of the extra crop pass is read against it.  Kernel times come from the library's own
per-launch events (vk_prof_enable), whole calls from device events around them."""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib

dev = torch.device("cuda:0")
N_IMG, H, W, S, BATCH = 32, 2048, 3072, 512, 32
REPS, ROUNDS = 10, 3


def timed(fn, reps=REPS, warm=2):
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


def median_of_rounds(fns, reps=REPS):
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            res[k].append(timed(fn, reps))
    return {k: sorted(v)[len(v) // 2] for k, v in res.items()}


def kernel_times(fn, reps=REPS):
    """us per call of every kernel family the library launches inside fn (its own events, one pair per launch)."""
    fn()
    torch.cuda.synchronize()
    L.lib().vk_prof_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {k: v["ms"] / reps * 1e3 for k, v in L.prof_collect().items()}
    L.lib().vk_prof_enable(0)
    return out


def build():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    images, masks = [], []
    for i in range(N_IMG):
        cy, cx = int(rng.integers(400, H - 400)), int(rng.integers(400, W - 400))
        images.append(np.roll(base, (37 * i, 91 * i), axis=(0, 1)))
        masks.append(((np.abs(xx - cx) + np.abs(yy - cy)) < 372).astype(np.uint8) * 255)
    return images, masks


images, masks = build()
fg = float(np.mean([(m > 0).mean() for m in masks]))
pds = vk.PatchDataset(images, masks, patch_size=S, device=dev)
dds = vk.DeviceDataset(images, masks, img_size=S, device=dev)
print(f"{N_IMG} images {H}x{W} ({pds.images.numel() / 1e6:.0f} MB of pixels, {pds.masks.numel() / 1e6:.0f} MB of masks, mean foreground "
      f"{100 * fg:.2f} %), patch {S}, batch {BATCH}; median of {ROUNDS} rounds x {REPS} calls")


def index():
    L.check(L.lib().vk_patch_index(len(pds), pds.items, pds._items_dev.data_ptr(), pds.images.numel(), pds.masks.data_ptr(), pds.masks.numel(),
                                   pds.rowcum.data_ptr(), pds.rowcum.numel(), L.current_stream()))


t_index = median_of_rounds({"index": index})["index"]
b_index = pds.masks.numel() + 12.0 * pds.rowcum.numel()
print(f"index build (once)  {t_index:9.1f} us ({b_index / t_index / 1e3:7.1f} GB/s of {b_index / 1e6:6.1f} MB)")

sm = vk.PatchSampler(seed=0)
idx = list(range(BATCH))
draws = [sm.sample(i, *pds.shapes[i], pds.fg_counts[i], S) for i in idx]
patch_draws = [dict(p, item=i) for i, (p, _) in zip(idx, draws)]
copy_draws = [dict(p, zoom=1.0, cos_a=1.0, sin_a=0.0) for p in patch_draws]
# the letterboxed pipeline with the same draws: the rotation goes back where the reference applies it
aug_draws = [dict(a, rotate=int((p["cos_a"], p["sin_a"]) != (1.0, 0.0)), cos_a=p["cos_a"], sin_a=p["sin_a"]) for p, a in draws]
n_rot = sum(d["rotate"] for d in aug_draws)
n_fg = sum(p["k"] >= 0 for p in patch_draws)
print(f"draws: {n_fg} of {BATCH} foreground-anchored, {n_rot} rotated, zoom {min(p['zoom'] for p in patch_draws):.3f}..{max(p['zoom'] for p in patch_draws):.3f}, "
      f"photometric {[a['photo'] for _, a in draws].count(1)} RBC / {[a['photo'] for _, a in draws].count(2)} CLAHE / {[a['photo'] for _, a in draws].count(3)} blur")

b_crop = 8.0 * BATCH * S * S
for name, pd in (("sampled draws", patch_draws), ("identity draws (copy path)", copy_draws)):
    k = kernel_times(lambda: pds.crop(pd))
    print(f"{name}:")
    print(f"  origins kernel    {k['patch_origins']:9.1f} us")
    print(f"  crop kernel       {k['patch_crop']:9.1f} us ({b_crop / k['patch_crop'] / 1e3:7.1f} GB/s of {b_crop / 1e6:6.1f} MB)")
k = kernel_times(lambda: pds.batch(idx, draws=draws))
kd = kernel_times(lambda: dds.batch(idx, draws=aug_draws))
print(f"PatchDataset.batch kernels : origins {k['patch_origins']:.1f} us, crop {k['patch_crop']:.1f} us, augment {k['augment']:.1f} us")
print(f"DeviceDataset.batch kernels: augment {kd['augment']:.1f} us (rotation inside it)")
med = median_of_rounds({"patch_batch": lambda: pds.batch(idx, draws=draws), "crop_only": lambda: pds.crop(patch_draws),
                        "letterboxed_batch": lambda: dds.batch(idx, draws=aug_draws)})
print(f"whole calls (host work, parameter upload and launches included):")
print(f"  PatchDataset.batch   {med['patch_batch']:9.1f} us   of which PatchDataset.crop {med['crop_only']:9.1f} us")
print(f"  DeviceDataset.batch  {med['letterboxed_batch']:9.1f} us   (the letterboxed pipeline, same augmentation draws)")
print(f"  extra cost of patch training per batch: {med['patch_batch'] - med['letterboxed_batch']:9.1f} us "
      f"= {(med['patch_batch'] - med['letterboxed_batch']) / 10700 * 100:5.2f} % of a 10.7 ms training step", flush=True)
torch.cuda.synchronize()
