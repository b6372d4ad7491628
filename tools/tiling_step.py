"""profiles/tiling: sliding-window inference (vk.tiling), event-timed on one MI355X.

1200 x 1600 and 2048 x 2048 uint8 images, tile 512, overlap 64, tta "none" and "d4", vk.Unet (resnet34, fp32, eval), chunks of 16 tiles.
Per configuration: vk_tile_preprocess, the forward passes, vk_tile_blend; the two kernels against their algorithmic bytes
(3hw + 12 T^2 ntiles nv, and 4 C T^2 ntiles nv + 4 C h w) and against the same result composed from torch ops (slice / flip / transpose /
sigmoid / slice-accumulate) on the same device in the same run; pre + blend as a share of the forward time."""
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
TL = vk.tiling

dev = torch.device("cuda:0")
T, OVERLAP, BATCH = 512, 64, 16
REPS, ROUNDS = 10, 3
MEAN = torch.tensor([0.485, 0.456, 0.406], device=dev).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225], device=dev).view(3, 1, 1)


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


def view(a, v):
    """View v of [..., T, T] with torch ops."""
    if v & 2:
        a = a.flip(-2)
    if v & 1:
        a = a.flip(-1)
    return a.transpose(-1, -2) if v & 4 else a


def unview(a, v):
    if v & 4:
        a = a.transpose(-1, -2)
    if v & 2:
        a = a.flip(-2)
    return a.flip(-1) if v & 1 else a


def torch_pre(src, grid, views):
    """What a user writes without vk.tiling.tile_preprocess (every image here is at least one tile, so no padding)."""
    out = []
    for y0 in grid.ys:
        for x0 in grid.xs:
            a = src[y0:y0 + T, x0:x0 + T].permute(2, 0, 1).flip(0).float()
            a = (a / 255.0 - MEAN) / STD
            out.extend(view(a, v) for v in views)
    return torch.stack(out)


def torch_blend(logits, grid, views, w2d):
    nv = len(views)
    C = logits.shape[1]
    acc = torch.zeros(C, grid.h, grid.w, device=dev)
    wsum = torch.zeros(grid.h, grid.w, device=dev)
    t = 0
    for y0 in grid.ys:
        for x0 in grid.xs:
            p = torch.sigmoid(logits[t * nv:(t + 1) * nv])
            q = torch.stack([unview(p[k], v) for k, v in enumerate(views)]).mean(0)
            acc[:, y0:y0 + T, x0:x0 + T] += w2d * q
            wsum[y0:y0 + T, x0:x0 + T] += w2d
            t += 1
    return (acc / wsum).clamp_(0, 1)


def forward_all(model, x):
    out = []
    with torch.no_grad():
        for i in range(0, x.shape[0], BATCH):
            chunk = x[i:i + BATCH]
            k = chunk.shape[0]
            if k < BATCH:
                chunk = torch.cat([chunk, x.new_zeros(BATCH - k, *x.shape[1:])])
            out.append(model(chunk)[:k])
    return torch.cat(out)


torch.manual_seed(0)
model = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev).eval()
w1 = TL.window_1d(T, OVERLAP).to(dev)
w2d = w1[:, None] * w1[None, :]
print(f"tile {T}, overlap {OVERLAP}, chunks of {BATCH}, vk.Unet resnet34 fp32 eval; median of {ROUNDS} rounds x {REPS} calls (forward: {ROUNDS} x 2)")
for h, w in ((1200, 1600), (2048, 2048)):
    src = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev)
    grid = TL.tile_grid(h, w, T, OVERLAP)
    for tta in ("none", "d4"):
        views = TL.TTA_VIEWS[tta]
        n = grid.ntiles * len(views)
        x = TL.tile_preprocess(src, grid, tta, dev)
        logits = forward_all(model, x)
        # the yardstick computes the same thing
        d_pre = (torch_pre(src, grid, views) - x).abs().max().item()
        d_blend = (torch_blend(logits, grid, views, w2d)[0] - TL.tile_blend(logits, grid, tta)[0]).abs().max().item()
        med = median_of_rounds({"pre": lambda: TL.tile_preprocess(src, grid, tta, dev), "pre_torch": lambda: torch_pre(src, grid, views),
                                "blend": lambda: TL.tile_blend(logits, grid, tta), "blend_torch": lambda: torch_blend(logits, grid, views, w2d)})
        fwd = median_of_rounds({"fwd": lambda: forward_all(model, x)}, reps=2)["fwd"]
        b_pre = 3.0 * h * w + 12.0 * T * T * n
        b_blend = 4.0 * T * T * n + 4.0 * h * w
        print(f"{h}x{w} tta={tta}: {grid.ny}x{grid.nx} tiles x {len(views)} views = {n} forward tiles; max|vk - torch| pre {d_pre:.1e} blend {d_blend:.1e}")
        print(f"  pre     vk {med['pre']:9.1f} us ({b_pre / med['pre'] / 1e3:7.1f} GB/s of {b_pre / 1e6:6.1f} MB)   torch {med['pre_torch']:9.1f} us ({med['pre_torch'] / med['pre']:5.1f}x)")
        print(f"  blend   vk {med['blend']:9.1f} us ({b_blend / med['blend'] / 1e3:7.1f} GB/s of {b_blend / 1e6:6.1f} MB)   torch {med['blend_torch']:9.1f} us ({med['blend_torch'] / med['blend']:5.1f}x)")
        print(f"  forward    {fwd / 1e3:9.2f} ms; pre + blend = {(med['pre'] + med['blend']) / fwd * 100:5.2f} % of it (torch composition: "
              f"{(med['pre_torch'] + med['blend_torch']) / fwd * 100:5.2f} %)", flush=True)
        del x, logits
        torch.cuda.empty_cache()
