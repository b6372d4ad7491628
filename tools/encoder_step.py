"""profiles/encoders: the encoders of vk.encoders on one MI355X.

  --ab      same-box A/B of the pointwise kernels (vk_conv1x1_fwd / its data gradient / vk_conv1x1_wgrad) against the generic tap-by-tap
            path (vk_conv_fwd / vk_conv_wgrad with R = S = 1, what resnet34's downsamples run on) at resnet50's layer shapes, bs 32 of
            512 x 512, bf16; alternating rounds, median of event-timed loops, and each kernel's fraction of its HBM / MFMA floor.
  --steps   the bf16, bs 32, 512 x 512 training step (loss_and_backward + FusedAdamW.step) per encoder, alternating rounds, medians,
            and the per-tag launch table of one resnet50 step (vk_prof).
Run under `rocprofv3 --kernel-trace --stats` with `--steps --encoders resnet50 --rounds 1` for the kernel table."""
import argparse
import ctypes as C
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib

dev = torch.device("cuda:0")
HBM = 6.29e12            # measured copy rate, bytes/s (MI355X_MICROARCH.md)
MFMA_BF16 = 2.5e15       # dense bf16 matrix peak, FLOP/s
N = 32
# (name, H, W of the input, C, K, stride): resnet50 at 512 x 512
SHAPES = [("layer1 conv3 / ds 64->256 @128", 128, 128, 64, 256, 1), ("layer1 conv1 256->64 @128", 128, 128, 256, 64, 1),
          ("layer4 conv1 2048->512 @16", 16, 16, 2048, 512, 1), ("layer4 conv3 512->2048 @16", 16, 16, 512, 2048, 1),
          ("layer2.0 ds 256->512 s2 @128", 128, 128, 256, 512, 2), ("layer3.0 ds 512->1024 s2 @64", 64, 64, 512, 1024, 2),
          ("layer4.0 ds 1024->2048 s2 @32", 32, 32, 1024, 2048, 2)]


def st():
    return torch.cuda.current_stream().cuda_stream


def time_ms(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(rounds):
    L = vk.lib()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    null = L_.vk_src(None, 0, 0, None, None, 0)
    print(f"A/B, bf16, N={N}: median ms of {rounds} alternating rounds (new 1x1 kernel / generic tap-by-tap kernel), floor = "
          f"max(bytes / {HBM / 1e12:.2f} TB/s, FLOP / {MFMA_BF16 / 1e15:.1f} PF/s)")
    for name, H, W, Cc, K, s in SHAPES:
        Ho, Wo = H // s, W // s
        x = torch.randn(N, H, W, Cc, device=dev).to(torch.bfloat16)
        w = (torch.randn(K, Cc, device=dev) / Cc ** 0.5).to(torch.bfloat16)
        wt = w.t().contiguous()
        sc = (0.5 + torch.rand(Cc, device=dev))
        sh = 0.1 * torch.randn(Cc, device=dev)
        y = torch.empty(N, Ho, Wo, K, device=dev, dtype=torch.bfloat16)
        dz = torch.randn(N, Ho, Wo, K, device=dev).to(torch.bfloat16)
        dx = torch.empty(N, H, W, Cc, device=dev, dtype=torch.bfloat16)
        dw = torch.zeros(K, Cc, device=dev)
        stats = torch.zeros(32, 2, K, dtype=torch.float64, device=dev)
        src = L_.vk_src(x.data_ptr(), Cc, 0, sc.data_ptr(), sh.data_ptr(), 1)
        d = L_.vk_conv_desc(L_.VK_BF16, N, H, W, Ho, Wo, K, 1, 1, s, 0, 0, src, null)
        dd = L_.vk_conv_desc(L_.VK_BF16, N, Ho, Wo, H, W, Cc, 1, 1, s, 0, 1, L_.vk_src(dz.data_ptr(), K, 0, None, None, 0), null)
        M, Mi = N * Ho * Wo, N * H * W
        flops = 2.0 * M * Cc * K
        kinds = {
            "fwd": (lambda: L.vk_conv1x1_fwd(C.byref(d), w.data_ptr(), y.data_ptr(), 0, stats.data_ptr(), st()),
                    lambda: L.vk_conv_fwd(C.byref(d), w.data_ptr(), y.data_ptr(), None, 0, 0, stats.data_ptr(), st()),
                    (M * Cc + M * K + K * Cc) * 2.0),
            "dgrad": (lambda: L.vk_conv1x1_fwd(C.byref(dd), wt.data_ptr(), dx.data_ptr(), 0, None, st()),
                      lambda: L.vk_conv_fwd(C.byref(dd), wt.data_ptr(), dx.data_ptr(), None, 0, 0, None, st()),
                      (M * K + Mi * Cc + K * Cc) * 2.0),
            "wgrad": (lambda: L.vk_conv1x1_wgrad(C.byref(d), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), st()),
                      lambda: L.vk_conv_wgrad(C.byref(d), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), st()),
                      (M * K + M * Cc) * 2.0 + K * Cc * 8.0),
        }
        for kind, (new, old, nbytes) in kinds.items():
            assert new() == 0 and old() == 0, (name, kind, L.vk_last_error_string())
            tn, to = [], []
            for _ in range(rounds):
                tn.append(time_ms(new))
                to.append(time_ms(old))
            mn, mo = sorted(tn)[len(tn) // 2], sorted(to)[len(to) // 2]
            floor = max(nbytes / HBM, flops / MFMA_BF16) * 1e3
            bound = "HBM" if nbytes / HBM >= flops / MFMA_BF16 else "MFMA"
            print(f"  {name:32s} {kind:5s} new {mn:7.4f} ms  generic {mo:7.4f} ms  speed-up {mo / mn:5.2f}x   floor {floor:7.4f} ms ({bound})"
                  f"  -> new at {floor / mn * 100:5.1f} % of it, generic at {floor / mo * 100:5.1f} %", flush=True)
        del x, w, wt, y, dz, dx


def steps(encoders, rounds, nsteps):
    torch.manual_seed(0)
    S = 512
    x = torch.randn(N, 3, S, S, device=dev)
    yt = (torch.rand(N, 1, S, S, device=dev) > 0.7).float()
    models, opts = {}, {}
    for e in encoders:
        models[e] = vk.encoders.Unet(encoder_name=e, encoder_weights=None).to(dev).train()
        opts[e] = vk.adamw_for(models[e], lr=5e-5, weight_decay=1e-4)

    def step(e):
        opts[e].zero_grad(set_to_none=True)
        models[e].loss_and_backward(x, yt, dtype=torch.bfloat16)
        opts[e].step()

    res = {e: [] for e in encoders}
    for rnd in range(rounds):
        for e in encoders:
            ms = time_ms(lambda: step(e), iters=nsteps, warm=3)
            res[e].append(ms)
            print(f"round {rnd} {e:9s} {ms:8.3f} ms/step", flush=True)
    print(f"\nmedian ms/step (bf16, bs {N}, {S}^2, loss_and_backward + FusedAdamW.step)")
    for e in encoders:
        print(f"  {e:9s} {sorted(res[e])[len(res[e]) // 2]:8.3f} ms  ({N / sorted(res[e])[len(res[e]) // 2] * 1e3:7.1f} images/s)")
    if "resnet50" in encoders:
        L = vk.lib()
        step("resnet50")
        torch.cuda.synchronize()
        L_.prof_collect()
        L.vk_prof_enable(1)
        step("resnet50")
        torch.cuda.synchronize()
        L.vk_prof_enable(0)
        tab = L_.prof_collect()
        print(f"\nper-tag launches of one resnet50 step: {sum(v['n'] for v in tab.values())} launches, "
              f"{sum(v['ms'] for v in tab.values()):.3f} ms summed (event-bracketed, so launch gaps are not in it)")
        for tag, v in sorted(tab.items(), key=lambda kv: -kv[1]["ms"]):
            fl = max(v["bytes"] / HBM, v["flops"] / MFMA_BF16) * 1e3
            print(f"  {tag:44s} {v['n']:5d} {v['ms']:9.3f} ms   floor {fl:8.3f} ms -> {fl / max(v['ms'], 1e-9) * 100:5.1f} %")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--encoders", default="resnet18,resnet34,resnet50")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nsteps", type=int, default=10)
    a = ap.parse_args()
    if a.ab:
        ab(a.rounds)
    if a.steps:
        steps(a.encoders.split(","), a.rounds, a.nsteps)
