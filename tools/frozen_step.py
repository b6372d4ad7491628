"""profiles/frozen: Full vs encoder-frozen training step, bf16, bs 32, 512 x 512, one process: loss_and_backward + FusedAdamW.step, event-timed,
alternating rounds.  Also the AdamW launch alone (whole buffer vs the decoder-only segment set) and per-tag launch tables."""
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
opt_full = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)                            # whole-buffer kernel, one counter
opt_frozen = vk.FusedAdamW(model.parameters(), lr=5e-5, weight_decay=1e-4).attach(model)   # per-tensor kernel
n_dec = sum(p.numel() for n, p in model.named_parameters() if not n.startswith("encoder."))
print(f"params {sum(p.numel() for p in model.parameters())}, decoder+head {n_dec}")


def set_frozen(frozen):
    model.encoder.requires_grad_(not frozen)


def step(opt):
    opt.zero_grad(set_to_none=True)
    model.loss_and_backward(x, y, dtype=torch.bfloat16)
    opt.step()


def timed(frozen, steps=10, warm=3):
    set_frozen(frozen)
    opt = opt_frozen if frozen else opt_full
    for _ in range(warm):
        step(opt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step(opt)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


res = {False: [], True: []}
for rnd in range(4):
    for frozen in (False, True):
        ms = timed(frozen)
        res[frozen].append(ms)
        print(f"round {rnd} {'frozen-encoder' if frozen else 'full          '} {ms:8.3f} ms/step", flush=True)
full = sorted(res[False])[len(res[False]) // 2]
frz = sorted(res[True])[len(res[True]) // 2]
print(f"median full {full:.3f} ms, frozen-encoder {frz:.3f} ms, ratio {frz / full:.3f} (target <= 0.75)")


def adamw_ms(frozen, reps=50):
    set_frozen(frozen)
    opt = opt_frozen if frozen else opt_full
    step(opt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        opt.step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


for frozen in (False, True):
    print(f"AdamW step alone ({'decoder+head segments' if frozen else 'whole buffer'}): {adamw_ms(frozen):.4f} ms (optimizer.step(), "
          f"prepare + update launches)")

L = vk.lib()
for frozen in (False, True):
    set_frozen(frozen)
    opt = opt_frozen if frozen else opt_full
    step(opt)
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    step(opt)
    torch.cuda.synchronize()
    L.vk_prof_enable(0)
    tab = vk._lib.prof_collect()
    print(f"\nper-tag launches of one step, {'encoder frozen' if frozen else 'full'}: {sum(v['n'] for v in tab.values())} launches, "
          f"{sum(v['ms'] for v in tab.values()):.3f} ms summed")
    for tag, v in sorted(tab.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"  {tag:44s} {v['n']:5d} {v['ms']:9.3f} ms")
