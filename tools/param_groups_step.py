"""profiles/param_groups: the training step with param groups and gradient clipping, bf16, bs 32, 512 x 512, one process:
loss_and_backward + (clip) + FusedAdamW.step, event-timed, alternating rounds.
  (a) vk.adamw_for(model, lr, wd)                                   the default: whole-buffer kernel
  (b) three groups (encoder at 0.2 lr / decoder + head / no-decay 1-D tensors)   vk_adamw_step_groups
  (c) (b) + optimizer.clip_grad_norm_(max_norm)                     vk_grad_norm_segments, coefficient folded into the step
  (d) (a) + torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)   what worked before: foreach kernels over 140 views
  (e) (a) with the encoder frozen                                   one group over a partial set: vk_adamw_step_groups, group table of zeros
Also the clip call and the optimizer step alone.  `--trace [letters]`: a few steps of each listed round only ((c) when none is given), for
a rocprofv3 --kernel-trace --stats run of its own."""
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")

dev = torch.device("cuda:0")
torch.manual_seed(0)
model = vk.Unet(encoder_weights=None).to(dev).train()
x = torch.randn(32, 3, 512, 512, device=dev)
y = (torch.rand(32, 1, 512, 512, device=dev) > 0.7).float()
LR, WD, MAX_NORM = 5e-5, 1e-4, 1.0


def three_groups():
    fg = vk.finetune_groups(model, LR, encoder_lr_scale=0.2, weight_decay=WD, decay_norm_and_bias=False)
    nodecay = [p for g in fg if g["weight_decay"] == 0.0 for p in g["params"]]
    return [g for g in fg if g["weight_decay"] != 0.0] + [dict(params=nodecay, lr=LR, weight_decay=0.0)]


opts = {"a": vk.adamw_for(model, lr=LR, weight_decay=WD),
        "b": vk.adamw_for(model, lr=LR, weight_decay=WD, groups=three_groups()),
        "c": vk.adamw_for(model, lr=LR, weight_decay=WD, groups=three_groups()),
        "d": vk.adamw_for(model, lr=LR, weight_decay=WD),
        "e": vk.adamw_for(model, lr=LR, weight_decay=WD)}
NAMES = {"a": "default", "b": "three groups", "c": "three groups + clip_grad_norm_", "d": "default + torch clip_grad_norm_",
         "e": "default, frozen encoder"}
params = list(model.parameters())
print(f"params {sum(p.numel() for p in params)} in {len(params)} tensors, flat buffer {model.flat_grads.numel() * 4 / 1e6:.1f} MB, "
      f"groups {[len(g['params']) for g in opts['b'].param_groups]}")


def select(k):
    model.encoder.requires_grad_(k != "e")       # outside the timed region


def step(k):
    opt = opts[k]
    opt.zero_grad(set_to_none=True)
    model.loss_and_backward(x, y, dtype=torch.bfloat16)
    if k == "c":
        opt.clip_grad_norm_(MAX_NORM)
    elif k == "d":
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    opt.step()


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


if "--trace" in sys.argv:
    at = sys.argv.index("--trace") + 1
    which = sys.argv[at] if at < len(sys.argv) else "c"
    for k in which:
        select(k)
        for _ in range(6):
            step(k)
    torch.cuda.synchronize()
    print(f"trace run done: 6 steps of each of ({which})")
    sys.exit(0)

res = {k: [] for k in opts}
for rnd in range(4):
    for k in opts:
        select(k)
        ms = timed(lambda: step(k), 10, 3)
        res[k].append(ms)
        print(f"round {rnd} ({k}) {NAMES[k]:32s} {ms:8.3f} ms/step", flush=True)
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
for k in opts:
    print(f"median ({k}) {NAMES[k]:32s} {med[k]:8.3f} ms/step   spread {min(res[k]):.3f} .. {max(res[k]):.3f}")
print(f"(b) - (a) = {med['b'] - med['a']:+.3f} ms   (c) - (b) = {med['c'] - med['b']:+.3f} ms   (d) - (a) = {med['d'] - med['a']:+.3f} ms   "
      f"(c) - (d) = {med['c'] - med['d']:+.3f} ms")

select("a")
# the pieces alone, back to back on a gradient buffer left by one backward (so it is as cache-resident as 98 MB can be)
step("c")
torch.cuda.synchronize()
print(f"optimizer.clip_grad_norm_ alone:            {timed(lambda: opts['c'].clip_grad_norm_(MAX_NORM), 50, 5):.4f} ms (two launches)")
print(f"torch.nn.utils.clip_grad_norm_ alone:       {timed(lambda: torch.nn.utils.clip_grad_norm_(params, MAX_NORM), 20, 3):.4f} ms")
for k in ("a", "b", "e"):
    select(k)
    step(k)
    print(f"optimizer.step() alone, ({k}) {NAMES[k]:14s} {timed(opts[k].step, 50, 5):.4f} ms (prepare + update launches)")

L = vk.lib()
for k in ("a", "c", "e"):
    select(k)
    step(k)
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    step(k)
    torch.cuda.synchronize()
    L.vk_prof_enable(0)
    tab = vk._lib.prof_collect()
    print(f"\nper-tag launches of one step ({k}) {NAMES[k]}: {sum(v['n'] for v in tab.values())} launches")
    for tag, v in sorted(tab.items(), key=lambda kv: -kv[1]["ms"]):
        if "adamw" in tag or "grad_norm" in tag:
            print(f"  {tag:44s} {v['n']:5d} {v['ms']:9.4f} ms  {v['bytes'] / max(v['ms'], 1e-9) / 1e9:8.1f} TB/s of algorithmic bytes")
