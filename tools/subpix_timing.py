"""profiles/subpix: the sub-pixel refinement (vk.subpix), timed on one MI355X at the workload's validation shape, batch 32 at
512 x 512, max_components 64; prints the table of profiles/subpix/README.md (``--write PATH`` also writes it to a file).

Beside the call stands the geometry call it follows, on the same machine in alternating rounds (HIP events, buffers allocated once,
medians of the rounds): the rectangle and the quadrilateral fit of the prediction, each followed by the refinement of its records with
either estimator at its defaults, and with the widest parameters the call takes (win 15; 32 stations, reach 15).

The input: per image five squares of 40 to 90 px at random places and angles, rendered as a probability map with an edge ramp of about
two pixels (a 3 x 3 box blur of the 0 / 0.97 map): the dataset's statistic of a few large indentations on background."""
import argparse
import ctypes as C
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
I, L, S_ = vk.instances, vk._lib, vk.subpix

dev = torch.device("cuda:0")
N, S, CAP = 32, 512, 64
REPS, ROUNDS = 20, 7


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


def median_of_rounds(fns):
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            res[k].append(timed(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in res.items()}


def inputs():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    prob = np.full((N, S, S), 0.02, np.float32)
    for i in range(N):
        for _ in range(5):
            cy, cx = rng.integers(70, S - 70, 2)
            half, a = rng.integers(20, 46), rng.random() * np.pi / 2
            u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a)
            w = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
            prob[i][(np.abs(u) <= half) & (np.abs(w) <= half)] = 0.97
    t = torch.from_numpy(prob).to(dev)
    return torch.nn.functional.avg_pool2d(t[:, None], 3, 1, 1, count_include_pad=False)[:, 0].contiguous()


class Geometry:
    """One geometry call on buffers allocated once."""

    def __init__(self, x, fit):
        self.lib, self.x, self.fit = L.lib(), x, fit
        self.ct = L.vk_geom_det if fit == "rect" else L.vk_geom_quad
        self.desc = L.vk_geom_desc(S, S, 0.5 if fit == "rect" else 0.45, 3, 1, 1, max(200, int(0.0008 * S * S)), CAP)
        self.nbytes = int(self.lib.vk_geom_workspace_bytes(C.byref(self.desc), N))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.clean = torch.empty(N, S, S, dtype=torch.uint8, device=dev)
        self.raw = torch.zeros(N, CAP, C.sizeof(self.ct), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(N, dtype=torch.int32, device=dev)
        self.out = torch.zeros(N * CAP * C.sizeof(L.vk_subpix_quad) // 8, dtype=torch.int64, device=dev)

    def geometry(self):
        a = (N, self.x.data_ptr(), self.clean.data_ptr(), self.raw.data_ptr(), self.counts.data_ptr(), self.ws.data_ptr(), self.nbytes,
             L.current_stream())
        if self.fit == "rect":
            L.check(self.lib.vk_geom_minarearect(C.byref(self.desc), *a))
        else:
            L.check(self.lib.vk_geom_quadrilateral(C.byref(self.desc), 2, *a))

    def refine(self, p):
        L.check(self.lib.vk_subpix_refine(C.byref(p), N, S, S, self.x.data_ptr(), self.raw.data_ptr(), C.sizeof(self.ct), self.ct.box.offset,
                                          self.ct.valid.offset if self.fit == "quad" else -1, self.counts.data_ptr(), CAP, None,
                                          self.out.data_ptr(), L.current_stream()))

    def records(self):
        return self.out.view(torch.uint8).cpu().numpy().view(S_.RECORD_DTYPE).reshape(N, CAP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prob = inputs()
    variants = {"corner, defaults (win 5)": S_.params("corner"), "lines, defaults (12 stations, reach 6)": S_.params("lines"),
                "corner, win 15": S_.params("corner", win=15), "lines, 32 stations, reach 15": S_.params("lines", n_stations=32, reach=15)}
    say("N = %d, %d x %d, max_components %d; median [min, max] of %d rounds x %d calls, HIP events; %s"
        % (N, S, S, CAP, ROUNDS, REPS, torch.cuda.get_device_name(0)))
    for fit in ("rect", "quad"):
        g = Geometry(prob, fit)
        g.geometry()
        torch.cuda.synchronize()
        objects = int(g.counts.clamp(max=CAP).sum().item())
        fns = {"geometry": g.geometry}
        for name, p in variants.items():
            fns[name] = (lambda p=p: g.refine(p))
        med = median_of_rounds(fns)
        say()
        say("fit = %s: %d records in all" % (fit, objects))
        say()
        say("| what | us per call | of the geometry call | vertices flagged | mean iterations / crossings per vertex |")
        say("|---|---|---|---|---|")
        say("| vk_geom_%s (exists without this module) | %.1f [%.1f, %.1f] | | | |" % ("minarearect" if fit == "rect" else "quadrilateral", *med["geometry"]))
        for name, p in variants.items():
            g.out.zero_()
            g.refine(p)
            r = g.records()
            used = r["valid"] == 1
            flagged = int((r["flags"][used] != 0).sum())
            say("| vk_subpix_refine, %s | %.1f [%.1f, %.1f] | %.1f %% | %d of %d | %.1f |"
                % (name, *med[name], 100.0 * med[name][0] / med["geometry"][0], flagged, 4 * int(used.sum()), float(r["iters"][used].mean())))
    if args.write:
        Path(args.write).parent.mkdir(parents=True, exist_ok=True)
        Path(args.write).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
