"""profiles/bn_frozen: frozen BatchNorm statistics and the input gradient, one process on one MI355X, HIP-event timed, alternating rounds.
  * the bf16 bs 32 512 x 512 fused step (loss_and_backward + FusedAdamW.step) in three settings: all train, encoder BatchNorm in eval mode
    (weights trainable), encoder frozen in weights and statistics; per-tag launch tables of one step each;
  * an eval-mode saliency pass (forward + backward to x, every parameter frozen) at bs 16, 512 x 512, fp32 and bf16;
  * the stem data gradient alone (vk_stem_dgrad, bf16, bs 32, 512 x 512, both operand forms) against its HBM roofline."""
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")

dev = torch.device("cuda:0")
L = vk.lib()
torch.manual_seed(0)
model = vk.Unet(encoder_weights=None).to(dev).train()
x = torch.randn(32, 3, 512, 512, device=dev)
y = (torch.rand(32, 1, 512, 512, device=dev) > 0.7).float()
opt_full = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
opt_sub = vk.FusedAdamW(model.parameters(), lr=5e-5, weight_decay=1e-4).attach(model)
SETTINGS = ("all-train", "encoder-bn-eval", "encoder-frozen")


def setting(name):
    model.train()
    model.requires_grad_(True)
    if name != "all-train":
        model.encoder.eval()
    if name == "encoder-frozen":
        model.encoder.requires_grad_(False)
    return opt_sub if name == "encoder-frozen" else opt_full


def step(opt):
    opt.zero_grad(set_to_none=True)
    model.loss_and_backward(x, y, dtype=torch.bfloat16)
    opt.step()


def timed(fn, steps=10, warm=3):
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


res = {k: [] for k in SETTINGS}
for rnd in range(4):
    for name in SETTINGS:
        opt = setting(name)
        ms = timed(lambda: step(opt))
        res[name].append(ms)
        print(f"round {rnd} {name:16s} {ms:8.3f} ms/step", flush=True)
base = median(res["all-train"])
for name in SETTINGS:
    print(f"median {name:16s} {median(res[name]):8.3f} ms  ({median(res[name]) / base:.3f} x all-train)")


def table(fn, title):
    fn()
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    L.vk_prof_enable(0)
    tab = vk._lib.prof_collect()
    print(f"\nper-tag launches, {title}: {sum(v['n'] for v in tab.values())} launches, {sum(v['ms'] for v in tab.values()):.3f} ms summed")
    for tag, v in sorted(tab.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"  {tag:44s} {v['n']:5d} {v['ms']:9.3f} ms")


for name in SETTINGS:
    opt = setting(name)
    table(lambda: step(opt), f"one step, {name}")
del opt_full, opt_sub

# ---- saliency: forward + backward to x, every parameter frozen, every BatchNorm in eval mode
model.eval()
model.requires_grad_(False)
xs = x[:16].clone()
bce = torch.nn.BCEWithLogitsLoss()


def saliency(dtype):
    xr = xs.clone().requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
    with ctx:
        lg = model(xr)
    bce(lg.float(), y[:16]).backward()
    return xr.grad


sal = {torch.float32: [], torch.bfloat16: []}
for rnd in range(3):
    for dt in sal:
        sal[dt].append(timed(lambda: saliency(dt), steps=5, warm=2))
for dt, v in sal.items():
    print(f"saliency bs 16 512^2 {str(dt):15s} median {median(v):8.3f} ms (forward + backward to x), rounds {[round(t, 3) for t in v]}")
    table(lambda: saliency(dt), f"saliency {dt}")

# ---- the stem data gradient alone
N, H, W = 32, 512, 512
g = torch.randn(N, H // 2, W // 2, 64, device=dev).to(torch.bfloat16)
z = torch.randn(N, H // 2, W // 2, 64, device=dev).to(torch.bfloat16)
coef = torch.randn(3, 64, device=dev)
w = torch.randn(64, 7, 7, 3, device=dev) * 0.05
dx = torch.empty(N, 3, H, W, device=dev)
st = vk._lib.current_stream()
for form, zz, cc in (("dz", None, None), ("bna", z.data_ptr(), coef.data_ptr())):
    def run():
        vk._lib.check(L.vk_stem_dgrad(1, N, H, W, g.data_ptr(), zz, cc, w.data_ptr(), dx.data_ptr(), st))
    ms = timed(run, steps=20, warm=5)
    nbytes = g.numel() * 2 * (2 if zz else 1) + dx.numel() * 4
    print(f"stem dgrad bf16 bs 32 512^2 ({form}): {ms:.4f} ms, {nbytes / 1e9:.3f} GB -> {nbytes / ms / 1e9:.2f} TB/s "
          f"({nbytes / 8e12 * 1e3:.4f} ms at 8 TB/s: {nbytes / 8e12 * 1e3 / ms * 100:.0f} % of the HBM roofline)")
