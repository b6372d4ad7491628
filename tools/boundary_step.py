"""profiles/boundary: distance maps, surface statistics and the boundary loss (vk.boundary), event-timed on one MI355X.

Three inputs: 32 x 512 x 512 real masks (the eight label masks of tests/golden/real_masks.npz letterboxed to 512, each in its four
mirrorings), one 3072 x 2048 map (real mask 5 letterboxed to 3072 and cropped), and the worst case of the outward search, one site in a
corner, at both sizes.  Reported: edt_sq with the per-row choice and with either form of the row pass forced (interleaved rounds in one process), then signed_distance,
surface_stats and BoundaryLoss forward + backward, each beside the bytes its passes move at the least (source read once, every int32 /
fp32 map written once and read once by the pass that follows) and the time those bytes take at the measured HBM copy rate of 6.29
TB/s."""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import boundary_cases as BC  # noqa: E402

vk = importlib.import_module("vickers-hardness-unet_amd")
B = vk.boundary
dev = torch.device("cuda:0")
REPS, ROUNDS = 10, 5
HBM = 6.29e12
GOLDEN = ROOT / "tests" / "golden"


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


def rounds(fns, reps=REPS):
    """Interleaved: every round times each function once; median (min .. max) per function."""
    v = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, f in enumerate(fns):
            v[i].append(timed(f, reps))
    return [(sorted(x)[len(x) // 2], min(x), max(x)) for x in v]


def fmt(r):
    return f"{r[0]:9.1f} us ({r[1]:.1f} .. {r[2]:.1f})"


def inputs():
    small = []
    for i in range(8):
        m = BC.letterboxed(BC.real_mask(GOLDEN, i), 512)
        small += [m, m[::-1], m[:, ::-1], m[::-1, ::-1]]
    big = BC.letterboxed(BC.real_mask(GOLDEN, 5), 3072)[:, 512:2560]
    c32 = np.zeros((32, 512, 512), np.uint8)
    c32[:, 0, 0] = 1
    c1 = np.zeros((1, 3072, 2048), np.uint8)
    c1[0, 0, 0] = 1
    return {"32 x 512 x 512 real": np.ascontiguousarray(np.stack(small)), "1 x 3072 x 2048 real": np.ascontiguousarray(big[None]),
            "32 x 512 x 512 corner": c32, "1 x 3072 x 2048 corner": c1}


print(f"median (min .. max) of {ROUNDS} interleaved rounds x {REPS} calls; floor = least bytes / {HBM / 1e12:.2f} TB/s")
for name, m in inputs().items():
    t = torch.from_numpy(m).to(dev)
    px = t.numel()
    print(f"{name}: foreground {100.0 * m.mean():.2f} %")
    for sites in ("fg", "bg", "edge"):
        c, a, b = rounds([lambda: B.edt_sq(t, sites), lambda: B.edt_sq(t, sites, rows="search"), lambda: B.edt_sq(t, sites, rows="envelope")],
                         reps=REPS if "real" in name else 3)
        by = px * (1 + 4 * 3)                  # source, g written and read, d2 written
        print(f"  edt_sq {sites:4s}: per row {fmt(c)}  search {fmt(a)}  envelope {fmt(b)}  floor {by / HBM * 1e6:6.1f} us of {by / 1e6:.0f} MB")
        assert torch.equal(B.edt_sq(t, sites), B.edt_sq(t, sites, rows="envelope")) and torch.equal(B.edt_sq(t, sites), B.edt_sq(t, sites, rows="search"))
    if "corner" in name:
        continue
    y = t.float().view(t.shape[0], 1, *t.shape[1:])
    pred = torch.roll(t, shifts=(2, 1), dims=(1, 2))
    logits = torch.randn(y.shape, device=dev, requires_grad=True)
    phi = B.signed_distance(y)
    loss = vk.BoundaryLoss()

    def fwd_bwd():
        logits.grad = None
        loss(logits, dist=phi).backward()

    def fwd_bwd_target():
        logits.grad = None
        loss(logits, y).backward()

    r = rounds([lambda: B.signed_distance(t), lambda: B.surface_stats(pred, t), fwd_bwd, fwd_bwd_target])
    for what, rr, by in (("signed_distance", r[0], px * (2 * 13 + 12)), ("surface_stats", r[1], px * (4 * 13 + 16 + 2 * 8)),
                         ("BoundaryLoss fwd+bwd, phi given", r[2], px * 12), ("BoundaryLoss fwd+bwd from the target", r[3], px * (4 + 2 * 16 + 12 + 12))):
        print(f"  {what:38s} {fmt(rr)}  floor {by / HBM * 1e6:6.1f} us of {by / 1e6:.0f} MB")
    m0 = B.surface_metrics(pred, t)["mean"]
    print(f"  the masks against themselves moved by (2, 1): hd {m0['hd']:.3f} hd95 {m0['hd95']:.3f} assd {m0['assd']:.3f} nsd@1 {m0['nsd'][1]:.3f} "
          f"boundary_iou {m0['boundary_iou']:.3f}", flush=True)
torch.cuda.synchronize()
