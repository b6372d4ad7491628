"""profiles/render: vk.render, event-timed on one MI355X.

val_panels at N = 18 (the reference's validation split) of 512 x 512; the draw on one built 3072 x 2048 image (dark diamonds on a
bright ground) with 1, 4 and 16 detections, tile-binned (the default) beside the direct form (VK_RENDER_DIRECT), with the GB/s of the
bytes that must move (source 3, mask 1, three outputs 9 per pixel); the box reduction with k = 4; and, as the only host-side number
there is to put beside them (cv2 is not installed), the time of tests/render_ref.py's vectorised numpy panels on this box's CPUs: a
restatement's time, not the reference's.  Kernel times are the library's own per-launch events (vk_prof_enable); whole calls are device
events round the Python call, median and spread of the rounds."""
import importlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
vk = importlib.import_module("vickers-hardness-unet_amd")
import render_ref as RR  # noqa: E402

L = vk._lib
Rn = vk.render
dev = torch.device("cuda:0")
H, W, S = 2048, 3072, 512
REPS, ROUNDS = 10, 5
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


def build(n):
    g = {1: (1, 1, 370), 4: (2, 2, 370), 16: (4, 4, 180)}[n]
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.full((H, W), BRIGHT, np.uint8)
    for iy in range(g[0]):
        for ix in range(g[1]):
            cy, cx = (iy + 0.5) * H / g[0] + 3 * ix, (ix + 0.5) * W / g[1] + 5 * iy
            img[(np.abs(xx - cx) + np.abs(yy - cy)) < g[2]] = DARK
    return np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))


print(f"kernels: mean of {REPS} calls (vk_prof_enable); whole calls: median (min .. max) of {ROUNDS} rounds x {REPS} calls")

# ------------------------------------------------------------------------------------------------ panels
N, P = 18, 512
g = torch.Generator(device="cpu").manual_seed(0)
x = torch.randn(N, 3, P, P, generator=g)
y = (torch.rand(N, 1, P, P, generator=g) > 0.5).float()
pr = torch.rand(N, 1, P, P, generator=g)
xd, yd, pd = x.to(dev), y.to(dev), pr.to(dev)
k = kernel_times(lambda: Rn.val_panels(xd, yd, pd))["render_panels"]
moved = N * P * P * (20.0 + 12.0)
med, lo, hi = rounds(lambda: Rn.val_panels(xd, yd, pd))
print(f"val_panels N = {N}, {P} x {P}: kernel {k:8.1f} us ({moved / k / 1e3:7.1f} GB/s of {moved / 1e6:.1f} MB: 20 bytes read, 12 written per pixel); "
      f"whole call {med:8.1f} us ({lo:.1f} .. {hi:.1f})")
t_back = rounds(lambda: Rn.val_panels(xd, yd, pd).cpu(), reps=3)
print(f"  with the read-back of the {N * P * 4 * P * 3 / 1e6:.1f} MB canvas: {t_back[0] / 1e3:8.2f} ms ({t_back[1] / 1e3:.2f} .. {t_back[2] / 1e3:.2f})")
t_planes = rounds(lambda: (xd.cpu(), yd.cpu(), pd.cpu()), reps=3)
print(f"  the reference's read-back instead (five float32 planes per image, {N * P * P * 20 / 1e6:.1f} MB): {t_planes[0] / 1e3:8.2f} ms "
      f"({t_planes[1] / 1e3:.2f} .. {t_planes[2] / 1e3:.2f})")
xn, yn, pn = x.numpy(), y.numpy(), pr.numpy()
torch.set_num_threads(16)
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    ref = RR.val_panels_ref(xn, yn, pn)
    ts.append(time.perf_counter() - t0)
same = np.array_equal(ref.reshape(N, P, 4 * P, 3), Rn.val_panels(xd, yd, pd).cpu().numpy())
print(f"  tests/render_ref.py's numpy panels on the host (a restatement's time, not the reference's): {sorted(ts)[1] * 1e3:8.1f} ms "
      f"({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f}), same bytes: {same}", flush=True)

# ------------------------------------------------------------------------------------------------ draw
for n_ind in (1, 4, 16):
    host = build(n_ind)
    img = torch.from_numpy(host).to(dev)
    with torch.no_grad():
        xin, _ = vk.prepost.preprocess(img, S, "centered", dev, pad_value=BRIGHT)
        prob = torch.sigmoid(standin(xin))[:, 0].contiguous()
    dets = vk.geometry.detect(prob, fit="quad")
    aff = vk.subpix.letterbox_affine(H, W, S, "centered")
    fine = vk.subpix.refine(dets, prob, affine=aff)
    mask = (img[..., 0] < 120).to(torch.uint8) * 255
    outs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(3)]
    prims, drawn, skipped = Rn.primitives(fine)
    kp = kernel_times(lambda: Rn.primitives(fine))["render_prims"]
    res = {}
    for name, flags in (("binned", 0), ("direct", L.VK_RENDER_DIRECT)):
        tag = "render_draw_direct" if flags else "render_draw"
        res[name] = kernel_times(lambda: Rn.draw(img, mask, outs, prims=prims, drawn=drawn, flags=flags))[tag]
        res[name + "_out"] = [o.clone() for o in outs]
    same = all(torch.equal(a, b) for a, b in zip(res["binned_out"], res["direct_out"]))
    k0 = kernel_times(lambda: Rn.draw(img, mask, outs))["render_draw"]
    moved = H * W * 13.0
    print(f"{n_ind} indentation(s): {int(drawn[0])} drawn, {int(skipped[0])} skipped; primitives {kp:6.1f} us; draw binned {res['binned']:8.1f} us "
          f"({moved / res['binned'] / 1e3:7.1f} GB/s of {moved / 1e6:.1f} MB), direct {res['direct']:8.1f} us ({res['direct'] / res['binned']:.2f}x), "
          f"no list {k0:8.1f} us; same bytes: {same}")
    med, lo, hi = rounds(lambda: Rn.draw_detections_on_three(img, mask, None, fine))
    med4, lo4, hi4 = rounds(lambda: Rn.draw_detections_on_three(img, mask, None, fine, reduce=4))
    print(f"  draw_detections_on_three, whole call: {med:8.1f} us ({lo:.1f} .. {hi:.1f}); with reduce=4: {med4:8.1f} us ({lo4:.1f} .. {hi4:.1f})", flush=True)

kr = kernel_times(lambda: Rn.box_reduce(outs[0], 4))["render_reduce"]
moved = 3.0 * (H * W + (H // 4) * (W // 4))
print(f"box_reduce k = 4 of {H} x {W}: kernel {kr:8.1f} us ({moved / kr / 1e3:7.1f} GB/s of {moved / 1e6:.1f} MB)")
full = rounds(lambda: [o.cpu() for o in outs], reps=3)
small = [Rn.box_reduce(o, 4) for o in outs]
red = rounds(lambda: [o.cpu() for o in small], reps=3)
print(f"read-back of the three views: full size ({3 * H * W * 3 / 1e6:.1f} MB) {full[0] / 1e3:8.2f} ms ({full[1] / 1e3:.2f} .. {full[2] / 1e3:.2f}); "
      f"after k = 4 ({3 * (H // 4) * (W // 4) * 3 / 1e6:.1f} MB) {red[0] / 1e3:8.2f} ms ({red[1] / 1e3:.2f} .. {red[2] / 1e3:.2f})")
pm = rounds(lambda: prob.new_empty(H, W).cpu(), reps=3)
print(f"read-back of one float32 map of {H} x {W} ({H * W * 4 / 1e6:.1f} MB), what the GUIs take to the host: {pm[0] / 1e3:8.2f} ms ({pm[1] / 1e3:.2f} .. {pm[2] / 1e3:.2f})",
      flush=True)
torch.cuda.synchronize()
