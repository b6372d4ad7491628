"""profiles/copypaste: instance copy-paste (vk.copypaste), event-timed on one MI355X.

183 built 768 x 1024 images (uint8 BGR) letterboxed to 512, with the component counts the training masks have (164 with one
indentation, 10 with two, 9 with three), each a diamond whose box is about 0.32 of the short side of the content.  Reported: the bank
build (once: detect_gt, vk_cp_boxes, vk_cp_alpha and the read-back), then CopyPaste.compose for 32 samples with 0, 1 and 3 pastes of
the median donor at scale 1 — the kernel against its byte floor (4 bytes read and 4 written per pixel, plus 5 bytes per pixel of the
donor boxes, at the measured HBM copy rate of 6.29 TB/s) — and vk_augment_batch for the same batch, so the cost of the extra pass is
read against it.  Kernel times come from the library's own per-launch events (vk_prof_enable), whole calls from device events round
them; the bank build from a host clock round work that ends in its read-back."""
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

dev = torch.device("cuda:0")
N_IMG, H, W, S, BATCH = 183, 768, 1024, 512, 32
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
    r = int(0.32 * H / 2)
    centres = {1: [(H // 2, W // 2)], 2: [(H // 2, W // 4), (H // 2, 3 * W // 4)], 3: [(H // 3, W // 5), (2 * H // 3, W // 2), (H // 3, 4 * W // 5)]}
    images, masks = [], []
    for i in range(N_IMG):
        k = 1 if i < 164 else 2 if i < 174 else 3
        m = np.zeros((H, W), np.uint8)
        for cy, cx in centres[k]:
            dy, dx = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
            m[(np.abs(xx - cx - dx) + np.abs(yy - cy - dy)) < r] = 255
        images.append(np.roll(base, (37 * i, 91 * i), axis=(0, 1)))
        masks.append(m)
    return images, masks


images, masks = build()
ds = vk.DeviceDataset(images, masks, img_size=S, device=dev)
del images, masks
print(f"{N_IMG} items letterboxed to {S} x {S} ({ds.images.numel() / 1e6:.0f} MB of pixels, {ds.masks.numel() / 1e6:.0f} MB of masks), batch {BATCH}; "
      f"median (min .. max) of {ROUNDS} rounds x {REPS} calls")

# ---- the bank, once per dataset
bank = vk.InstanceBank(ds)
walls = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bank = vk.InstanceBank(ds)                # ends in the read-back of the boxes
    walls.append((time.perf_counter() - t0) * 1e3)
L.lib().vk_prof_enable(1)
vk.InstanceBank(ds)
torch.cuda.synchronize()
kb = L.prof_collect()
L.lib().vk_prof_enable(0)
n_comp = np.bincount(np.minimum(bank.counts, 4), minlength=5)
print(f"bank: {len(bank.records)} components ({n_comp[1]} items with one, {n_comp[2]} with two, {n_comp[3]} with three), {len(bank.donors)} donors; "
      f"median donor box {int(np.median(bank.donors['x1'] - bank.donors['x0'] + 1))} x {int(np.median(bank.donors['y1'] - bank.donors['y0'] + 1))}")
print(f"bank build, whole call, host clock: {sorted(walls)[1]:.1f} ms ({min(walls):.1f} .. {max(walls):.1f}); of it cp_boxes "
      f"{kb['cp_boxes']['ms'] * 1e3:.1f} us in {kb['cp_boxes']['n']} calls, cp_alpha {kb['cp_alpha']['ms'] * 1e3:.1f} us in {kb['cp_alpha']['n']} calls; "
      f"the rest is detect_gt, float copies of the masks and the read-back")

# ---- compose
cp = vk.CopyPaste(ds, bank)
idx = list(range(0, N_IMG, N_IMG // BATCH))[:BATCH]
donors = bank.donors[np.argsort((bank.donors["x1"] - bank.donors["x0"]) * (bank.donors["y1"] - bank.donors["y0"]))]
med = donors[len(donors) // 2]
sw, sh = int(med["x1"] - med["x0"] + 1), int(med["y1"] - med["y0"] + 1)
top, left, nh, nw = (int(v) for v in ds.content[0])
places = [(left + 2, top + 2), (left + nw - sw - 2, top + nh - sh - 2), (left + nw - sw - 2, top + 2)]


def record(j, p):
    """Paste p of sample j: one of the donors of median size (the built diamonds differ by a pixel or two), unscaled, turned by 0 or 180
    degrees with or without the mirror."""
    d = donors[(len(donors) // 2 + 7 * j + p) % len(donors)]
    w, h = int(d["x1"] - d["x0"] + 1), int(d["y1"] - d["y0"] + 1)
    return dict(donor=int(d["item"]), sx0=int(d["x0"]), sy0=int(d["y0"]), sw=w, sh=h, d4=((j + p) % 8) & 6, dx0=places[p][0], dy0=places[p][1],
                dw=w, dh=h)


def records(k):
    return [[record(j, p) for p in range(k)] for j in range(BATCH)]


sm = vk.AugmentSampler(seed=0)
draws = [sm.sample() for _ in idx]
floor_px = 8.0 * BATCH * S * S
print(f"compose, {BATCH} samples; pastes of {sw} x {sh} at scale 1; byte floor = (8 S^2 per sample + 5 bytes per donor pixel) / {HBM / 1e12:.2f} TB/s")
for k in (0, 1, 3):
    recs = records(k)
    by = floor_px + 5.0 * sum(r["sw"] * r["sh"] for lst in recs for r in lst)
    kt = kernel_times(lambda: cp.compose(idx, recs))["cp_paste"]
    whole = rounds(lambda: cp.compose(idx, recs))
    print(f"  {k} pastes: kernel {kt:7.1f} us = {by / kt / 1e6:5.2f} TB/s of {by / 1e6:5.1f} MB, floor {by / HBM * 1e6:5.1f} us ({kt / (by / HBM * 1e6):4.2f} x); "
          f"whole call {whole[0]:7.1f} us ({whole[1]:.1f} .. {whole[2]:.1f})")
ka = kernel_times(lambda: ds.batch(idx, draws=draws))
wa = rounds(lambda: ds.batch(idx, draws=draws))
recs = records(3)
wb = rounds(lambda: cp.batch(idx, draws=draws, pastes=recs))
print(f"vk_augment_batch, same batch, AugmentSampler(seed=0) draws ({[d['photo'] for d in draws].count(2)} CLAHE, {sum(d['rotate'] for d in draws)} rotated): "
      f"kernels {ka['augment']:7.1f} us; DeviceDataset.batch whole call {wa[0]:7.1f} us ({wa[1]:.1f} .. {wa[2]:.1f})")
print(f"CopyPaste.batch with 3 pastes, whole call {wb[0]:7.1f} us ({wb[1]:.1f} .. {wb[2]:.1f}): {wb[0] - wa[0]:+.1f} us over DeviceDataset.batch "
      f"= {(wb[0] - wa[0]) / 10300 * 100:.2f} % of a 10.3 ms training step", flush=True)
torch.cuda.synchronize()
