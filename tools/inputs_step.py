"""profiles/inputs: the training step of vk.inputs.Unet(in_channels = 1, 3, 4) and vk_input_mix, event-timed on one MI355X.

The step: bs 32, 512 x 512, bf16, loss_and_backward + FusedAdamW, interleaved rounds in one process (the stem reads the same NHWC4 input
whatever in_channels is, so the three are expected to be equal; what differs is the input transform's read, the stem weight gradient's
epilogue and the size of its reduce).  The mix: 32 x 512 x 512 to 1..4 planes, beside the time its bytes (3 planes read, cout written,
33.5 MB each) take at the HBM copy rate recorded in profiles/tiling."""
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

vk = importlib.import_module("vickers-hardness-unet_amd")
dev = torch.device("cuda:0")
N, S = 32, 512
REPS, ROUNDS = 10, 5
HBM = 6.29e12


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
    v = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, f in enumerate(fns):
            v[i].append(timed(f, reps))
    return [(sorted(x)[len(x) // 2], min(x), max(x)) for x in v]


def fmt(r):
    return f"{r[0]:9.1f} us ({r[1]:.1f} .. {r[2]:.1f})"


def stepper(cin):
    vk.seed_everything(42)
    m = vk.inputs.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=cin, classes=1, activation=None).to(dev).train()
    opt = vk.adamw_for(m, lr=5e-5, weight_decay=1e-4)
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(N, cin, S, S, generator=g).to(dev)
    y = (torch.rand(N, 1, S, S, generator=g) > 0.7).float().to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        m.loss_and_backward(x, y, dtype=torch.bfloat16)
        opt.step()

    return step


print(f"median (min .. max) of {ROUNDS} interleaved rounds x {REPS} calls")
chans = (1, 3, 4)
res = rounds([stepper(c) for c in chans])
for c, r in zip(chans, res):
    print(f"train step bs {N} {S}x{S} bf16, in_channels={c}: {fmt(r)}  ({N / r[0] * 1e6:.1f} images/s)")

x3 = torch.randn(N, 3, S, S, device=dev)
ident = torch.nn.Identity()
adapters = [vk.inputs.ChannelAdapter(ident, mode="luma")] + [
    vk.inputs.ChannelAdapter(ident, matrix=[[0.5, 0.25, 0.25]] * c, bias=[0.1] * c) for c in (2, 3, 4)]
res = rounds([(lambda a=a: a.mix(x3)) for a in adapters], reps=50)
for a, r in zip(adapters, res):
    by = N * S * S * 4 * (3 + a.cout)
    print(f"vk_input_mix {N} x {S} x {S} -> {a.cout} plane(s) (with the output's allocation): {fmt(r)}  floor {by / HBM * 1e6:6.1f} us of {by / 1e6:.1f} MB")
