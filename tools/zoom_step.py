"""profiles/zoom: the second pass of vk.zoom, event-timed on one MI355X.

One built 3072 x 2048 image (uint8 BGR, dark diamonds on a bright ground) with 1, 4 and 16 indentations, first pass on the 512-pixel
letterbox through a stand-in segmenter (a fixed affine function of the red plane, so that the detections are where the diamonds are),
S = 512.  Reported: the three kernels (the library's own per-launch events, vk_prof_enable), the gather's achieved bytes/s against the
bytes of its source footprints plus its output, the direct gather (the default) beside the staged form (VK_ZOOM_STAGED), also at s = 3 exactly,
the whole refine_detections call with vk.Unet resnet34 under bf16 autocast in eval mode as the second-pass segmenter (untrained
weights: only its time means anything), and Segmenter.infer_tiled on the same image, the other route to native-resolution evidence."""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib
Z = vk.zoom

dev = torch.device("cuda:0")
H, W, S, BATCH = 2048, 3072, 512, 16
REPS, ROUNDS = 10, 3
DARK, BRIGHT = 40, 200
X_MID = (0.5 * (DARK + BRIGHT) / 255.0 - 0.485) / 0.229


def standin(x):
    return (x[:, 0:1] - X_MID) * -1.0


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
    fn()
    torch.cuda.synchronize()
    L.lib().vk_prof_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {k: v["ms"] / reps * 1e3 for k, v in L.prof_collect().items()}
    L.lib().vk_prof_enable(0)
    return out


def build(n):
    """n diamonds on a grid: diagonal 740 for 1 and 4 of them (4.4 % of the frame each), 360 for 16."""
    g = {1: (1, 1, 370), 4: (2, 2, 370), 16: (4, 4, 180)}[n]
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.full((H, W), BRIGHT, np.uint8)
    for iy in range(g[0]):
        for ix in range(g[1]):
            cy, cx = (iy + 0.5) * H / g[0] + 3 * ix, (ix + 0.5) * W / g[1] + 5 * iy
            img[(np.abs(xx - cx) + np.abs(yy - cy)) < g[2]] = DARK
    return np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))


def footprint_bytes(win, n):
    w = win.cpu().numpy().reshape(-1).view(Z.WINDOW_DTYPE)[:n]
    tot = 0.0
    for r in w:
        span = S * float(r["s"])
        x0, x1 = max(float(r["X0"]), 0.0), min(float(r["X0"]) + span, W)
        y0, y1 = max(float(r["Y0"]), 0.0), min(float(r["Y0"]) + span, H)
        tot += 3.0 * max(x1 - x0, 0.0) * max(y1 - y0, 0.0)
    return tot


torch.manual_seed(0)
model = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev).eval()


def unet_bf16(x):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return model(x)


print(f"image {H}x{W}, S = {S}, chunks of {BATCH}; kernels: mean of {REPS} calls (vk_prof_enable); whole calls: median of {ROUNDS} rounds x {REPS} calls")
for n_ind in (1, 4, 16):
    img = torch.from_numpy(build(n_ind)).to(dev)
    with torch.no_grad():
        x, _ = vk.prepost.preprocess(img, S, "centered", dev, pad_value=BRIGHT)
        prob = torch.sigmoid(standin(x))[:, 0].contiguous()
    dets = vk.geometry.detect(prob, fit="quad")
    aff = vk.subpix.letterbox_affine(H, W, S, "centered")
    win, cnt = Z.windows(dets, [[H, W]], aff, S=S)
    n = int(cnt.item())
    scales = win.cpu().numpy().reshape(-1).view(Z.WINDOW_DTYPE)[:n]["s"]
    print(f"{n_ind} indentation(s): {int(dets.counts[0])} detected, {n} windows, s = {scales.min():.3f}..{scales.max():.3f}")
    fine = Z.refine_detections(standin, [img], dets, prob, affine=aff, S=S, batch=BATCH, pad_value=BRIGHT)
    st = fine.status[0, :n].cpu().numpy()
    print(f"  with the stand-in as second-pass segmenter: {int(((st & Z.STATUS['zoomed']) != 0).sum())} of {n} slots zoomed, status {sorted(set(st.tolist()))}")
    k = kernel_times(lambda: Z.refine_detections(standin, [img], dets, prob, affine=aff, S=S, batch=BATCH, pad_value=BRIGHT))
    b_foot, b_out = footprint_bytes(win, n), 12.0 * n * S * S
    print(f"  zoom_windows {k['zoom_windows']:8.1f} us   zoom_gather {k['zoom_gather']:8.1f} us ({(b_foot + b_out) / k['zoom_gather'] / 1e3:7.1f} GB/s of "
          f"{b_foot / 1e6:.1f} MB footprint + {b_out / 1e6:.1f} MB output)   zoom_merge {k['zoom_merge']:8.1f} us")
    kd = kernel_times(lambda: Z.gather([img], win, n, S, BRIGHT, 0))
    ks = kernel_times(lambda: Z.gather([img], win, n, S, BRIGHT, L.VK_ZOOM_STAGED))
    print(f"  gather alone: direct (default) {kd['zoom_gather']:8.1f} us, staged {ks['zoom_gather']:8.1f} us ({ks['zoom_gather'] / kd['zoom_gather']:.2f}x)")
    med = median_of_rounds({"zoom_standin": lambda: Z.refine_detections(standin, [img], dets, prob, affine=aff, S=S, batch=BATCH, pad_value=BRIGHT),
                            "zoom_unet": lambda: Z.refine_detections(unet_bf16, [img], dets, prob, affine=aff, S=S, batch=BATCH, pad_value=BRIGHT),
                            "coarse": lambda: vk.subpix.refine(dets, prob, affine=aff)})
    print(f"  refine_detections, whole call: stand-in {med['zoom_standin']:9.1f} us, vk.Unet bf16 eval (chunks of {BATCH}) {med['zoom_unet'] / 1e3:9.2f} ms; "
          f"the coarse refinement alone {med['coarse']:7.1f} us", flush=True)

# s = 3 exactly: 16 windows of the 16-indentation image at fixed scale
w3 = np.zeros(16, Z.WINDOW_DTYPE)
for i in range(16):
    w3[i] = (0, i, 0, 0, 100.0 + 90.5 * i, 40.25 + 30.0 * i, 3.0)
w3d = torch.from_numpy(w3.view(np.uint8).reshape(-1).copy()).to(dev)
w3d = torch.zeros(16 * 5, dtype=torch.int64, device=dev).view(torch.uint8).copy_(w3d)
kd = kernel_times(lambda: Z.gather([img], w3d, 16, S, BRIGHT, 0))["zoom_gather"]
ks = kernel_times(lambda: Z.gather([img], w3d, 16, S, BRIGHT, L.VK_ZOOM_STAGED))["zoom_gather"]
same = torch.equal(Z.gather([img], w3d, 16, S, BRIGHT, 0), Z.gather([img], w3d, 16, S, BRIGHT, L.VK_ZOOM_STAGED))
b3 = 16 * (3.0 * (3 * S) ** 2 + 12.0 * S * S)
print(f"s = 3, 16 windows inside the image: direct (default) {kd:8.1f} us ({b3 / kd / 1e3:7.1f} GB/s of {b3 / 1e6:.1f} MB), staged {ks:8.1f} us ({ks / kd:.2f}x), same bits: {same}")

seg = vk.Segmenter(model, img_size=S, device=dev)
host = img.cpu().numpy()


def tiled():
    with torch.autocast("cuda", dtype=torch.bfloat16):
        seg.infer_tiled(host, overlap=64, batch=BATCH)


grid = vk.tiling.tile_grid(H, W, S, 64)
t_tiled = median_of_rounds({"tiled": tiled}, reps=2)["tiled"]
print(f"Segmenter.infer_tiled on the same image (tile {S}, overlap 64, {grid.ntiles} tiles, bf16 autocast, host copy of the map included): {t_tiled / 1e3:9.2f} ms",
      flush=True)
torch.cuda.synchronize()
