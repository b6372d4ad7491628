"""profiles/sweep: the threshold sweep (vk.sweep), event-timed on one MI355X; prints the tables of profiles/sweep/README.md
(``--write PATH`` also writes them to a file).

Histogram pass at N = 32, 1 x 512 x 512, for K = 99 (the default grid) and K = 1024, float and uint8 targets, on two inputs:
  saturated  logits of magnitude 8..14 with the sign of a 4 % foreground square (the dataset's statistic),
             0.5 % of the pixels redrawn in [-3, 3] (the edge of the indent): nearly everything lands in an end bin;
  uniform    probabilities uniform in [0, 1]: every pixel in a middle bin, the worst case for the LDS atomics.
Beside it, from the same run: one vk_seg_metrics call at one threshold (the same bytes read: the floor), and K such calls (what a sweep
costs without this module).  GB/s over the algorithmic bytes (8 B per element, 5 B with uint8 targets).  Then the curves pass at N = 32
and N = 512 images."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
SW = vk.sweep

dev = torch.device("cuda:0")
N, S = 32, 512
REPS, ROUNDS = 20, 5


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


def median_of_rounds(fns, reps=REPS):
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            res[k].append(timed(fn, reps))
    return {k: sorted(v)[len(v) // 2] for k, v in res.items()}


def raw_hist(x, t, thr, from_logits):
    """vk_sweep_hist through ctypes on buffers allocated once: the timed call is the library's work alone."""
    lib, L = vk.lib(), vk._lib
    k = int(thr.size)
    hist = torch.empty(N, 1, 2, k + 1, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    thr_d = torch.from_numpy(thr.copy()).to(dev)
    keep.append(thr_d)
    args = (N, S * S, 0, x.data_ptr(), t.data_ptr(), 1 if t.dtype == torch.uint8 else 0, 1 if from_logits else 0, 0, 0, k, thr.ctypes.data,
            thr_d.data_ptr(), 0, hist.data_ptr(), bad.data_ptr())
    return lambda: L.check(lib.vk_sweep_hist(*args, L.current_stream())), hist


def raw_metrics(x, t, from_logits):
    lib, L = vk.lib(), vk._lib
    ws_bytes = lib.vk_seg_metrics_workspace_bytes(N)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(2 + 2 * N, dtype=torch.float32, device=dev)
    return lambda th=0.5: L.check(lib.vk_seg_metrics(N, S * S, x.data_ptr(), t.data_ptr(), 1 if from_logits else 0, th, 1e-7, ws.data_ptr(),
                                                     ws_bytes, out.data_ptr(), L.current_stream()))


keep = []


def inputs():
    g = torch.Generator(device="cpu").manual_seed(0)
    tgt = torch.zeros(N, 1, S, S)
    side = int(round((0.04 * S * S) ** 0.5))
    for i in range(N):
        y0, x0 = (int(v) for v in torch.randint(0, S - side, (2,), generator=g))
        tgt[i, 0, y0:y0 + side, x0:x0 + side] = 1
    mag = 8 + 6 * torch.rand(N, 1, S, S, generator=g)
    logits = torch.where(tgt > 0, mag, -mag)
    edge = torch.rand(N, 1, S, S, generator=g) < 0.005
    logits = torch.where(edge, 6 * torch.rand(N, 1, S, S, generator=g) - 3, logits)
    prob = torch.rand(N, 1, S, S, generator=g)
    tgt_u = (torch.rand(N, 1, S, S, generator=g) < 0.04).float()
    return {"saturated": (logits.to(dev), tgt.to(dev), True), "uniform": (prob.to(dev), tgt_u.to(dev), False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("N = %d, 1 x %d x %d; median of %d rounds x %d calls, HIP events on the stream; %s" % (N, S, S, ROUNDS, REPS, torch.cuda.get_device_name(0)))
    say()
    say("| input | K | target | sweep_hist us | GB/s | seg_metrics x1 us | GB/s | sweep / single | seg_metrics x K us | K calls / sweep | LDS atomics per pixel |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    elems = N * S * S
    for name, (x, t, from_logits) in inputs().items():
        t8 = t.to(torch.uint8)
        for K in (99, 1024):
            thr = SW.DEFAULT_THRESHOLDS if K == 99 else (np.arange(1, K + 1) / (K + 1)).astype(np.float32)
            thr_list = [float(v) for v in thr]
            out_f = SW.sweep_hist(x, t, thr, from_logits)
            out_u = SW.sweep_hist(x, t8, thr, from_logits)
            assert torch.equal(out_f[0], out_u[0])
            mid = out_f[0][..., 1:K].sum().item() / elems
            # the sweep's row at thr[k] is the single-threshold kernel's result
            k = K // 2
            res = SW.sweep_curves(out_f[0], thr)
            one = vk.seg_metrics_device(x, t, from_logits=from_logits, threshold=thr_list[k])
            assert torch.equal(one[:2].cpu(), torch.stack([res.mean_dice[k], res.mean_iou[k]]).cpu())

            thr = np.ascontiguousarray(thr)
            hist_f, hf = raw_hist(x, t, thr, from_logits)
            hist_u, hu = raw_hist(x, t8, thr, from_logits)
            single = raw_metrics(x, t, from_logits)
            hist_f(), hist_u()
            assert torch.equal(hf, out_f[0]) and torch.equal(hu, out_f[0])

            def k_calls():
                for th in thr_list:
                    single(th)

            med = median_of_rounds({"f32": hist_f, "u8": hist_u, "one": single})
            many = median_of_rounds({"k": k_calls}, reps=2 if K > 99 else 4)["k"]
            for dt, b in (("f32", 8.0), ("u8", 5.0)):
                say("| %s | %d | %s | %.1f | %.0f | %.1f | %.0f | %.2f | %.0f | %.0fx | %.4f |" % (
                    name, K, dt, med[dt], b * elems / med[dt] / 1e3, med["one"], 8.0 * elems / med["one"] / 1e3, med[dt] / med["one"], many,
                    many / med[dt], mid))
    say()
    say("| curves pass | N | C | K | groups | us |")
    say("|---|---|---|---|---|---|")
    rng = np.random.default_rng(0)
    for n in (32, 512):
        for K in (99, 1024):
            h = rng.integers(0, 40, (n, 1, 2, K + 1))
            h[..., 0] += 200000
            h[..., -1] += 9000
            hd = torch.from_numpy(h.astype(np.int32)).to(dev)
            thr = SW.DEFAULT_THRESHOLDS if K == 99 else (np.arange(1, K + 1) / (K + 1)).astype(np.float32)
            grp = torch.from_numpy((np.arange(n) // 32).astype(np.int32)).to(dev)
            G = (n + 31) // 32
            med = median_of_rounds({"plain": lambda: SW.sweep_curves(hd, thr), "groups": lambda: SW.sweep_curves(hd, thr, groups=grp, n_groups=G)})
            say("| vk_sweep_curves | %d | 1 | %d | none | %.1f |" % (n, K, med["plain"]))
            say("| vk_sweep_curves | %d | 1 | %d | %d batches of 32 | %.1f |" % (n, K, G, med["groups"]))
    if args.write:
        Path(args.write).parent.mkdir(parents=True, exist_ok=True)
        Path(args.write).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
