"""profiles/instances: the object-level metrics (vk.instances), timed on one MI355X at the workload's validation shape, batch 32 at
512 x 512; prints the table of profiles/instances/README.md (``--write PATH`` also writes it to a file).

Two things on the same machine, in alternating rounds:
  geometry x2      the two geometry calls alone (prediction: rectangle fit with the reference's defaults; target: the ground-truth
                   preset), through ctypes on buffers allocated once: the cost that exists without this module;
  object_metrics   the whole of vk.object_metrics: both detections with their slot maps, the contingency table, the matching and the
                   read-back of the totals (host clock around a call that ends in a device synchronisation), and the same work without
                   the read-back as ObjectMetrics.update (HIP events).
Beside them each new launch alone (HIP events, buffers allocated once) and the contingency kernel's multiple of its byte floor: two
int32 maps read once, 8 B per pixel, over 5 TB/s.

The input: per image five squares of 40 to 90 px at random places and angles as the target, the prediction a probability map of the
same squares moved by up to 3 px and grown or shrunk by up to 2 px: the dataset's statistic of a few large indentations on background."""
import argparse
import ctypes as C
import importlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
I, L = vk.instances, vk._lib

dev = torch.device("cuda:0")
N, S, CAP = 32, 512, 64
REPS, ROUNDS = 20, 7
HBM_TBS = 5.0


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


def host_timed(fn, reps=REPS, warm=3):
    """fn ends in a device synchronisation."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def median_of_rounds(fns):
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, (fn, timer) in fns.items():
            res[k].append(timer(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in res.items()}


def inputs():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    tgt = np.zeros((N, S, S), np.float32)
    prob = np.full((N, S, S), 0.02, np.float32)

    def square(m, cy, cx, half, a, v):
        u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a)
        w = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
        m[(np.abs(u) <= half) & (np.abs(w) <= half)] = v

    for i in range(N):
        for _ in range(5):
            cy, cx = rng.integers(70, S - 70, 2)
            half, a = rng.integers(20, 46), rng.random() * np.pi / 2
            square(tgt[i], cy, cx, half, a, 1.0)
            square(prob[i], cy + rng.integers(-3, 4), cx + rng.integers(-3, 4), half + rng.integers(-2, 3), a, 0.97)
    return torch.from_numpy(prob).to(dev), torch.from_numpy(tgt).to(dev)


class RawGeometry:
    """One geometry call with its slot map on buffers allocated once."""

    def __init__(self, x, bin_thresh, morph_kernel, min_area):
        self.lib = L.lib()
        self.x = x
        self.desc = L.vk_geom_desc(S, S, bin_thresh, morph_kernel, 1, 1, min_area, CAP)
        self.nbytes = int(self.lib.vk_geom_workspace_bytes(C.byref(self.desc), N))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.clean = torch.empty(N, S, S, dtype=torch.uint8, device=dev)
        self.raw = torch.zeros(N, CAP, C.sizeof(L.vk_geom_det), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(N, dtype=torch.int32, device=dev)
        self.slots = torch.empty(N, S, S, dtype=torch.int32, device=dev)

    def geometry(self):
        L.check(self.lib.vk_geom_minarearect(C.byref(self.desc), N, self.x.data_ptr(), self.clean.data_ptr(), self.raw.data_ptr(),
                                             self.counts.data_ptr(), self.ws.data_ptr(), self.nbytes, L.current_stream()))

    def slot_map(self):
        L.check(self.lib.vk_geom_slot_map(C.byref(self.desc), N, self.ws.data_ptr(), self.nbytes, self.slots.data_ptr(), L.current_stream()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prob, tgt = inputs()
    lib = L.lib()
    pred = RawGeometry(prob, 0.5, 3, max(200, int(0.0008 * S * S)))
    gt = RawGeometry(tgt, 0.5, 1, 1)
    for g in (pred, gt):
        g.geometry()
        g.slot_map()
    table = torch.empty(N, CAP + 1, CAP + 1, dtype=torch.int32, device=dev)
    thr = np.ascontiguousarray(I.DEFAULT_IOU_THRESHOLDS)
    K, rec, off = len(thr), I.STATS_DTYPE.itemsize, int(L.vk_geom_det.d_mean.offset)
    pair_gt = torch.empty(N, CAP, dtype=torch.int32, device=dev)
    pair_iou = torch.empty(N, CAP, dtype=torch.float64, device=dev)
    pair_derr = torch.empty(N, CAP, dtype=torch.float64, device=dev)
    per_image = torch.empty(N * K * rec // 8, dtype=torch.int64, device=dev)
    totals = torch.empty(K * rec // 8, dtype=torch.int64, device=dev)

    def cont():
        L.check(lib.vk_inst_contingency(N, S, S, pred.slots.data_ptr(), gt.slots.data_ptr(), CAP, CAP, table.data_ptr(), L.current_stream()))

    def mat():
        L.check(lib.vk_inst_match(N, CAP, CAP, table.data_ptr(), pred.counts.data_ptr(), gt.counts.data_ptr(), K, thr.ctypes.data,
                                  pred.raw.data_ptr() + off, rec_bytes, gt.raw.data_ptr() + off, rec_bytes, pair_gt.data_ptr(),
                                  pair_iou.data_ptr(), pair_derr.data_ptr(), per_image.data_ptr(), totals.data_ptr(), 0, L.current_stream()))

    rec_bytes = C.sizeof(L.vk_geom_det)
    cont()
    mat()
    torch.cuda.synchronize()
    # the timed pieces compute what the public path computes
    om = vk.ObjectMetrics(max_components=CAP)
    res = om.update(prob, tgt)
    assert torch.equal(res.table, table) and om.totals().tobytes() == totals.cpu().numpy().tobytes()
    m = om.compute()
    objects = int(m["n_gt"][0])

    def geometry_x2():
        pred.geometry()
        gt.geometry()

    def update():
        vk.ObjectMetrics(max_components=CAP).update(prob, tgt)

    def whole():
        vk.object_metrics(prob, tgt, max_components=CAP)

    med = median_of_rounds({"geometry x2": (geometry_x2, timed), "slot_map x2": (lambda: (pred.slot_map(), gt.slot_map()), timed),
                            "contingency": (cont, timed), "match": (mat, timed), "update": (update, timed), "whole": (whole, host_timed)})
    floor_us = 8.0 * N * S * S / (HBM_TBS * 1e12) * 1e6
    say("N = %d, %d x %d, max_components %d, %d target objects in all (tp %d, pq %.4f at IoU > 0.5); median [min, max] of %d rounds x %d calls; %s"
        % (N, S, S, CAP, objects, int(m["tp"][0]), float(m["pq"][0]), ROUNDS, REPS, torch.cuda.get_device_name(0)))
    say()
    say("| what | clock | us per call |")
    say("|---|---|---|")
    names = {"geometry x2": ("vk_geom_minarearect, prediction + target (exists without this module)", "HIP events"),
             "slot_map x2": ("vk_geom_slot_map, prediction + target", "HIP events"),
             "contingency": ("vk_inst_contingency", "HIP events"), "match": ("vk_inst_match (two launches)", "HIP events"),
             "update": ("ObjectMetrics.update: all of the above through the Python API, no read-back", "HIP events"),
             "whole": ("vk.object_metrics: the same with the read-back of the totals", "host clock, ends in a synchronisation")}
    for k, (what, clock) in names.items():
        say("| %s | %s | %.1f [%.1f, %.1f] |" % (what, clock, *med[k]))
    say()
    new = med["slot_map x2"][0] + med["contingency"][0] + med["match"][0]
    say("new launches together: %.1f us = %.1f %% of the two geometry calls (%.1f us)" % (new, 100.0 * new / med["geometry x2"][0], med["geometry x2"][0]))
    say("contingency kernel: %.1f us for %.1f MB = %.0f GB/s; byte floor at %.0f TB/s: %.1f us; multiple of the floor: %.1fx"
        % (med["contingency"][0], 8.0 * N * S * S / 1e6, 8.0 * N * S * S / med["contingency"][0] / 1e3, HBM_TBS, floor_us,
           med["contingency"][0] / floor_us))
    if args.write:
        Path(args.write).parent.mkdir(parents=True, exist_ok=True)
        Path(args.write).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
