"""profiles/averaging: what averaged weights cost.  One process, event-timed, alternating rounds.
  1. the pieces alone on the full resnet34 model's flat buffers: vk_avg_update (12 bytes per element: read average and source, write
     average), vk_avg_swap (16), the whole-buffer AdamW step (28: the yardstick, same access pattern) and the fused step (36 + 12 per
     statistics element), each as achieved bytes per second;
  2. the bf16, bs 32, 512 x 512 training step of bench.py's configuration (loss_and_backward + FusedAdamW.step), in interleaved rounds:
       (p) no average                           what a step has always launched
       (f) ModelEMA attached                    vk_adamw_step_amp_avg: prepare + one update launch
       (s) ModelEMA unattached, ema.update()    vk_adamw_step_amp, then vk_avg_update: four launches
`--rounds R --steps K` size part 2 (default 8 x 20).  `--trace`: 20 calls of every piece of part 1 and nothing else, for a
`rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--trace", action="store_true", help="a few calls of every piece of part 1 only, for a kernel-trace run")
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("averaging_step.py measures on the GPU: none found")
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = vk.Unet(encoder_weights=None).to(dev).train()
x = torch.randn(args.batch, 3, args.size, args.size, device=dev)
y = (torch.rand(args.batch, 1, args.size, args.size, device=dev) > 0.7).float()
LR, WD = 5e-5, 1e-4
n_p, n_b = model.flat_params.numel(), model._flat["bufs"].numel()
print(f"flat parameters {n_p} elements ({n_p * 4 / 1e6:.1f} MB), BatchNorm statistics {n_b} elements")

opts = {k: vk.adamw_for(model, lr=LR, weight_decay=WD) for k in "pfs"}
emas = {"f": vk.ModelEMA(model, decay=0.999, warmup=True).attach(opts["f"]), "s": vk.ModelEMA(model, decay=0.999, warmup=True)}
NAMES = {"p": "no average", "f": "attached (fused step)", "s": "step, then ema.update()"}


def step(k):
    opt = opts[k]
    opt.zero_grad(set_to_none=True)
    model.loss_and_backward(x, y, dtype=torch.bfloat16)
    opt.step()
    if k == "s":
        emas["s"].update()


def timed(fn, steps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def median(v):
    return sorted(v)[len(v) // 2]


# ---------------------------------------------------------------------------------------------- 1. the pieces alone
for k in "pfs":
    step(k)                                 # every optimizer has its state, the gradient buffer is one a backward left
torch.cuda.synchronize()
pieces = {
    "vk_avg_update (params + statistics)": (emas["s"].update, 12.0 * (n_p + n_b)),
    "2 x vk_avg_swap (there and back)": (lambda: (emas["s"]._swap(), emas["s"]._swap()), 32.0 * (n_p + n_b)),
    "FusedAdamW.step, no average": (opts["p"].step, 28.0 * n_p),
    "FusedAdamW.step, average attached": (opts["f"].step, 36.0 * n_p + 12.0 * n_b),
    "FusedAdamW.step + ema.update()": (lambda: (opts["s"].step(), emas["s"].update()), 28.0 * n_p + 12.0 * (n_p + n_b)),
}
if args.trace:                                 # for a rocprofv3 --kernel-trace --stats run of its own: 20 calls of every piece
    for fn, _ in pieces.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    print("trace run done: 20 calls of each piece")
    sys.exit(0)
times = {name: [] for name in pieces}
for rnd in range(9):
    for name, (fn, _) in pieces.items():
        times[name].append(timed(fn, 50, 5))
print("\nthe pieces alone (each figure: 50 back-to-back calls, prepare launches included; median of 9 alternating rounds)")
for name, (_, nbytes) in pieces.items():
    ms = median(times[name])
    print(f"  {name:38s} {ms * 1e3:8.1f} us   spread {min(times[name]) * 1e3:.1f} .. {max(times[name]) * 1e3:.1f} us   "
          f"{nbytes / 1e6:7.1f} MB   {nbytes / (ms * 1e-3) / 1e12:6.3f} TB/s")
upd, adam = median(times["vk_avg_update (params + statistics)"]), median(times["FusedAdamW.step, no average"])
print(f"  rate of vk_avg_update / rate of the whole-buffer AdamW step = {(12.0 * (n_p + n_b) / upd) / (28.0 * n_p / adam):.3f}")
print(f"  fused step - (step + update) = {(median(times['FusedAdamW.step, average attached']) - median(times['FusedAdamW.step + ema.update()'])) * 1e3:+.1f} us")

# ---------------------------------------------------------------------------------------------- 2. the training step
res = {k: [] for k in "pfs"}
for rnd in range(args.rounds):
    for k in ("pfs", "sfp", "fps")[rnd % 3]:
        ms = timed(lambda: step(k), args.steps, 3)
        res[k].append(ms)
        print(f"round {rnd} ({k}) {NAMES[k]:26s} {ms:8.3f} ms/step", flush=True)
print()
for k in "pfs":
    print(f"median ({k}) {NAMES[k]:26s} {median(res[k]):8.3f} ms/step   spread {min(res[k]):.3f} .. {max(res[k]):.3f}")
pairs = [f - s for f, s in zip(res["f"], res["s"])]
print(f"(f) - (s), paired by round: median {median(pairs) * 1e3:+.1f} us, {min(pairs) * 1e3:+.1f} .. {max(pairs) * 1e3:+.1f} us; "
      f"(f) - (p): {(median(res['f']) - median(res['p'])) * 1e3:+.1f} us; (s) - (p): {(median(res['s']) - median(res['p'])) * 1e3:+.1f} us")
print(f"updates counted: attached {emas['f'].updates}, unattached {emas['s'].updates}")
