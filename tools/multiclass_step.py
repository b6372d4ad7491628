"""profiles/multiclass: the bf16, bs 32, 512 x 512 training step (loss_and_backward + FusedAdamW.step) of Unet(classes=C) for
C in {1, 2, 4, 8, 16} x {multilabel, multiclass}, one process, event-timed, alternating rounds, medians.  C = 1 multi-label runs the
binary model's kernels (it is the binary loss).  Also per-tag launch tables of one step at C = 4 and the new kernels' times at C = 4
against their HBM floors."""
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")

dev = torch.device("cuda:0")
N, S = 32, 512
HBM_TBPS = 6.29          # measured copy rate (MI355X_MICROARCH.md)
torch.manual_seed(0)
x = torch.randn(N, 3, S, S, device=dev)
CLASSES = (1, 2, 4, 8, 16)
CASES = [(c, m) for c in CLASSES for m in ("multilabel", "multiclass") if not (c == 1 and m == "multiclass")]
models, opts, targets = {}, {}, {}
for c in CLASSES:
    models[c] = vk.multiclass.Unet(encoder_weights=None, classes=c).to(dev).train()
    opts[c] = vk.adamw_for(models[c], lr=5e-5, weight_decay=1e-4)
    targets[(c, "multilabel")] = (torch.rand(N, c, S, S, device=dev) > 0.7).float()
    if c > 1:
        targets[(c, "multiclass")] = torch.randint(0, c, (N, S, S), device=dev)


def step(c, mode):
    opts[c].zero_grad(set_to_none=True)
    models[c].loss_and_backward(x, targets[(c, mode)], dtype=torch.bfloat16, mode=mode)
    opts[c].step()


def timed(c, mode, steps=10, warm=3):
    for _ in range(warm):
        step(c, mode)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step(c, mode)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


res = {k: [] for k in CASES}
for rnd in range(3):
    for k in CASES:
        ms = timed(*k)
        res[k].append(ms)
        print(f"round {rnd} C={k[0]:2d} {k[1]:10s} {ms:8.3f} ms/step", flush=True)
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
base = med[(1, "multilabel")]
print("\nmedian ms/step (bf16, bs 32, 512^2, loss_and_backward + FusedAdamW.step)")
for k in CASES:
    print(f"  C={k[0]:2d} {k[1]:10s} {med[k]:8.3f} ms  (+{med[k] - base:6.3f} ms over C=1)")

L = vk.lib()
floors = {                   # bytes each kernel must move at C = 4 (bf16 activations, fp32 logits / dlogits / targets, int64 labels)
    "head_fwd_multi": N * S * S * (32 + 16),
    "head_bwd_multi": N * S * S * (32 + 16 + 32),
    "multilabel_loss": N * S * S * 4 * (4 + 4 + 4 + 4 + 4),
    "multiclass_loss": N * S * S * (2 * (4 * 4 + 8) + 4 * 4),
}
for mode in ("multilabel", "multiclass"):
    step(4, mode)
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    step(4, mode)
    torch.cuda.synchronize()
    L.vk_prof_enable(0)
    tab = vk._lib.prof_collect()
    print(f"\nper-tag launches of one step, C=4 {mode}: {sum(v['n'] for v in tab.values())} launches, "
          f"{sum(v['ms'] for v in tab.values()):.3f} ms summed")
    for tag, v in sorted(tab.items(), key=lambda kv: -kv[1]["ms"]):
        line = f"  {tag:44s} {v['n']:5d} {v['ms']:9.3f} ms"
        if tag in floors:
            fl = floors[tag] / (HBM_TBPS * 1e12) * 1e3
            line += f"   HBM floor {fl:.3f} ms -> {fl / v['ms'] * 100:5.1f} % of the floor's rate"
        print(line)
