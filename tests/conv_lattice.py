"""Integer-lattice cases for the convolution kernels and their float64 reference (no GPU needed; tests/test_conv_lattice_cpu.py checks
this module, tests/test_conv_sweep_gpu.py runs the kernels on its cases).

The method.  Every convolution kernel takes operands that are exact in its element type and accumulates in fp32 (MFMA with fp32
accumulators, fp32 split-K partial tiles, fp32 per-tile statistics followed by fp64 atomics).  With small integers as inputs, weights from
{-1, 0, 1}, prologue scales from {0.5, 1, 2} and integer shifts, every partial sum of every kernel is an integer (or a half) far below
2^24, whatever the order it is formed in: the kernel's result must EQUAL the float64 reference, in f32, bf16 and f16 alike, on every
path, split count and atomics order.  One dropped 8-channel vector, one wrong tap on a ragged tile column, one element read with a
neighbouring channel's scale is then a bit difference rather than a few percent of sigma under a max-norm bound.

`build(case)` restates the operation with F.conv2d / autograd in float64 on the operands the kernel is given (formulas: include/vk_unet.h):
    V[n][c][h][w] = act(src[n][c][h >> up][w >> up] * scale[c] + shift[c]),  sources concatenated along c
    fwd    y = conv2d(V, w, stride, pad);  stats = sum / sum of squares of y per output channel
    dgrad  dx = d conv2d(x, wf) / dx applied to dz  (the kernels' transposed = 1 form), then on its first part (channels [0, split), or all):
           pool2: 2 x 2 sums;  bnr: g = (dx [+ old]) * [z * scale + shift > 0  |  mask > 0],  sums = sum g, sum g * z;
           with accumulate the remaining channels (y1) are added to what y1 held (old1), unmasked
    wgrad  dw = d conv2d(V, w) / dw applied to dz
`check(b)` asserts the exactness conditions on that reference alone (never on a kernel's output), for every element of every case:
  1. every stored output and every prologue value is held exactly by each tested type: |v| <= 256 (bf16) / 2048 (f16) / 2^24 (f32) and
     a round trip through the type returns it;
  2. conv(|V|, |w|), the largest partial sum any order of accumulation can meet, is below 2^24;
  3. the fp32 statistics partial of one 128-pixel tile, 128 x the largest square (or product g * z), is below 2^24;
  4. with `accumulate`, 2 x the result still meets 1;
  5. the streaming kernels keep their fp32 statistics over a whole strip (16 columns, up to 256 rows, starting at any multiple of 8 rows):
     twice the largest sum of squares (or of |g|, |g z|) over an aligned 256 x 16 window, which covers every such strip, is below 2^24.
The per-channel tables have coprime periods (scale 3 / 9, shift 7 / 5, mask pair 3 x 7), so a thread that reads another channel group's
coefficients is off by a multiple of 8 channels and is seen unless that offset is a multiple of 21 (168 channels)."""
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LIM = {"f32": 2.0 ** 24, "bf16": 256.0, "f16": 2048.0}          # integers up to here are exact in the type
TWO24 = 2.0 ** 24
TILE_PIX = 128                                                   # pixels of one output tile: the span of an fp32 statistics partial
VAR_BUDGET = 1100.0                                              # variance of an output at full density (sigma 33: 6 sigma < 200 < 256)


@dataclass(frozen=True)
class Src:
    C: int
    up: int = 0
    pro: bool = False          # BatchNorm scale / shift + ReLU prologue on this source


@dataclass(frozen=True)
class Case:
    """kind fwd / wgrad: H, W = the virtual input map, srcs = the gather, K output channels.
    kind dgrad: H, W = the map of the gradient that is written (dx), srcs[0].C = channels of dz (the reduction), K = channels of dx."""
    name: str
    kind: str
    N: int
    H: int
    W: int
    srcs: tuple
    K: int
    R: int = 3
    stride: int = 1
    pad: int = 1
    split: int = 0             # dgrad: channels [0, split) -> y, [split, K) -> y1
    pool2: int = 0
    bnr: str = ""              # "", "affine" (scale + shift) or "mask" (external mask)
    accumulate: int = 0        # dgrad: y += result; with bnr: vk_bnr.accumulate
    density: float = 0.0       # share of non-zero weights; 0 = derived from the reduction length (see density())
    types: tuple = ("f32", "bf16", "f16")
    seed: int = 0

    @property
    def C(self):
        return sum(s.C for s in self.srcs)

    @property
    def out_hw(self):
        """fwd / wgrad: the output map.  dgrad: the map of dz."""
        return ((self.H + 2 * self.pad - self.R) // self.stride + 1, (self.W + 2 * self.pad - self.R) // self.stride + 1)


def density(case):
    """Non-zero share of the ternary weights, from arithmetic on the case alone: an output is a sum of R*R*C*density terms v * (+-1) with
    E[v^2] = 2 for integers uniform in [-2, 2] and at most 9 behind the prologue (relu(2 * 2 + 3) = 7, mostly far less); its variance is
    kept at VAR_BUDGET, divided by 4 where the stored value is a 2 x 2 sum or is doubled by `accumulate`."""
    if case.density:
        return case.density
    if case.kind == "wgrad":
        return 1.0                                               # no weights; dz is dense
    ev2 = 9.0 if any(s.pro for s in case.srcs) else 2.0
    budget = VAR_BUDGET / (4.0 if case.pool2 else 1.0) / (4.0 if case.accumulate else 1.0)
    return min(1.0, budget / (case.R * case.R * case.C * ev2))


def lat_scale(C, k):
    """{0.5, 1, 2} by channel; k picks the base-3 digit, so tables with different k are independent (periods 3, 9)."""
    c = torch.arange(C)
    return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[(c // 3 ** k) % 3]


def lat_int(C, mul, mod):
    """Integers in [-(mod // 2), mod // 2] by channel, period mod (mul coprime to mod)."""
    c = torch.arange(C)
    return ((c * mul) % mod - mod // 2).double()


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def ternary(shape, dens, g):
    w = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return w * (torch.rand(shape, generator=g) < dens)


def virtual_input(b):
    """V of include/vk_unet.h from the raw sources of a built case: affine + ReLU, nearest x2, concat."""
    parts = []
    for s, x, sc, sh in zip(b.case.srcs, b.x, b.scale, b.shift):
        v = x
        if s.pro:
            v = torch.relu(v * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        if s.up:
            v = F.interpolate(v, scale_factor=2, mode="nearest")
        parts.append(v)
    return torch.cat(parts, 1)


def build(case):
    """Operands (float64, NCHW / OIHW, on the CPU) and the expected results of one case."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    b = SimpleNamespace(case=case, x=[], scale=[], shift=[])
    Ho, Wo = case.out_hw
    if case.kind in ("fwd", "wgrad"):
        for i, s in enumerate(case.srcs):
            assert not s.up or (case.H % 2 == 0 and case.W % 2 == 0)
            b.x.append(ints((case.N, s.C, case.H >> s.up, case.W >> s.up), -2, 2, g))
            b.scale.append(lat_scale(s.C, i) if s.pro else None)
            b.shift.append(lat_int(s.C, 3 if i == 0 else 2, 7 if i == 0 else 5) if s.pro else None)
        b.V = virtual_input(b)
    if case.kind == "fwd":
        b.w = ternary((case.K, case.C, case.R, case.R), density(case), g)
        b.y = F.conv2d(b.V, b.w, stride=case.stride, padding=case.pad)
        b.absdot = F.conv2d(b.V.abs(), b.w.abs(), stride=case.stride, padding=case.pad)
        b.stats = torch.stack([b.y.sum(dim=(0, 2, 3)), (b.y * b.y).sum(dim=(0, 2, 3))])
    elif case.kind == "wgrad":
        b.dz = ints((case.N, case.K, Ho, Wo), -2, 2, g)
        wv = torch.zeros(case.K, case.C, case.R, case.R, dtype=torch.float64, requires_grad=True)
        F.conv2d(b.V, wv, stride=case.stride, padding=case.pad).backward(b.dz)
        b.dw = wv.grad
        wa = torch.zeros_like(wv, requires_grad=True)
        F.conv2d(b.V.abs(), wa, stride=case.stride, padding=case.pad).backward(b.dz.abs())
        b.absdot = wa.grad
    else:
        assert case.kind == "dgrad" and len(case.srcs) == 1 and not case.srcs[0].up and not case.srcs[0].pro
        Kred = case.srcs[0].C
        b.dz = ints((case.N, Kred, Ho, Wo), -2, 2, g)
        b.x, b.scale, b.shift = [b.dz], [None], [None]
        b.V = b.dz
        b.wf = ternary((Kred, case.K, case.R, case.R), density(case), g)          # the forward convolution's weights [K_fwd][C_fwd]
        b.w = b.wf.permute(1, 0, 2, 3).contiguous()                              # as the kernel indexes them: [out][red][R][S]
        xin = torch.zeros(case.N, case.K, case.H, case.W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, b.wf, stride=case.stride, padding=case.pad).backward(b.dz)
        b.dx = xin.grad
        xa = torch.zeros_like(xin, requires_grad=True)
        F.conv2d(xa, b.wf.abs(), stride=case.stride, padding=case.pad).backward(b.dz.abs())
        b.absdot = xa.grad
        k0 = case.split or case.K
        first = b.dx[:, :k0]
        b.y1 = b.dx[:, k0:] if case.split else None
        if case.pool2:
            assert case.H % 2 == 0 and case.W % 2 == 0
            first = F.avg_pool2d(first, 2) * 4.0
        b.old = b.z = b.mask = b.bn_scale = b.bn_shift = b.sums = None
        if case.accumulate:
            b.old = ints(tuple(first.shape), -2, 2, g)
            first = first + b.old
        b.pre = first                                                            # what the epilogue holds before the mask
        if case.bnr:
            b.z = ints(tuple(first.shape), -3, 3, g)
            if case.bnr == "affine":
                b.bn_scale, b.bn_shift = lat_scale(k0, 0), lat_int(k0, 3, 7)
                keep = (b.z * b.bn_scale.view(1, -1, 1, 1) + b.bn_shift.view(1, -1, 1, 1)) > 0
            else:
                b.mask = torch.relu(ints(tuple(first.shape), -2, 2, g))           # a block's stored output: about 3 in 5 are zero
                keep = b.mask > 0
            first = first * keep
            b.sums = torch.stack([first.sum(dim=(0, 2, 3)), (first * b.z).sum(dim=(0, 2, 3))])
        b.y = first
        b.old1 = None
        if case.accumulate and case.split:                                       # the kernels add into the skip part too (no mask there)
            b.old1 = ints(tuple(b.y1.shape), -2, 2, g)
            b.y1 = b.y1 + b.old1
    return b


def exact_in(t, dtn):
    return bool((t.abs() <= LIM[dtn]).all()) and bool((t.to(TDT[dtn]).double() == t).all())


def strip_partial(t, rows=256, cols=16):
    """Upper bound of sum |t| over any strip of at most `rows` rows and `cols` aligned columns: such a strip lies inside two vertically
    adjacent aligned windows."""
    t = t.abs()
    N, Cc, H, W = t.shape
    t = F.pad(t, (0, -W % cols, 0, -H % rows))
    return 2.0 * t.view(N, Cc, t.shape[2] // rows, rows, t.shape[3] // cols, cols).sum(dim=(3, 5)).max().item()


def check(b):
    """The exactness conditions 1-4 of the module docstring, on the reference alone.  Returns the figures it checked."""
    c = b.case
    fig = {"max_absdot": b.absdot.max().item()}
    assert fig["max_absdot"] < TWO24, f"{c.name}: conv(|V|, |w|) reaches {fig['max_absdot']}"
    if c.kind == "wgrad":
        stored = [b.dw]
        types_out = ("f32",)                                     # weight gradients are fp32 in every element type
    else:
        stored = [b.y] + ([b.y1] if getattr(b, "y1", None) is not None else [])
        if c.kind == "dgrad":
            stored += [b.dx, b.pre]                              # before pooling / masking: what the epilogue holds
        types_out = c.types
    fig["max_out"] = max(t.abs().max().item() for t in stored)
    fig["max_v"] = b.V.abs().max().item()
    mult = 2.0 if (c.accumulate and not c.bnr) else 1.0
    for dtn in c.types:
        assert exact_in(b.V, dtn), f"{c.name}: a prologue value is not exact in {dtn} (max {fig['max_v']})"
        for extra in ("old", "old1", "z", "mask"):
            t = getattr(b, extra, None)
            assert t is None or exact_in(t, dtn)
    for dtn in types_out:
        for t in stored:
            assert exact_in(t * mult, dtn), f"{c.name}: an output is not exact in {dtn} (max {fig['max_out']} x {mult})"
    if c.kind == "fwd":
        assert TILE_PIX * fig["max_out"] ** 2 < TWO24, f"{c.name}: statistics partial 128 x {fig['max_out']}^2"
        fig["strip"] = strip_partial(b.y * b.y)
        assert fig["strip"] < TWO24, f"{c.name}: statistics partial of a strip reaches {fig['strip']}"
    if c.kind == "dgrad" and c.bnr:
        gz = (b.y * b.z).abs().max().item()
        assert TILE_PIX * max(gz, fig["max_out"]) < TWO24
        fig["strip"] = max(strip_partial(b.y * b.z), strip_partial(b.y))
        assert fig["strip"] < TWO24, f"{c.name}: BN-backward partial of a strip reaches {fig['strip']}"
    return fig


def flip_changes(case, what):
    """Sensitivity of the reference: the expected output after one input element, one weight or one channel's scale is changed."""
    b = build(case)
    base = (b.dw if case.kind == "wgrad" else b.y).clone()
    if what == "input":
        b.x[0][0, 1, 0, 0] = 1.0 if b.x[0][0, 1, 0, 0] == 2.0 else 2.0       # channel 1: scale 1, shift 0, so relu keeps the change
    elif what == "weight":
        b.w[0, 1, 1, 1] = 1.0 - b.w[0, 1, 1, 1]                   # -1 -> 2, 0 -> 1, 1 -> 0: always a change (channel 1, centre tap)
    else:
        b.scale[0][0] = 4.0
    V = virtual_input(b)
    if case.kind == "fwd":
        new = F.conv2d(V, b.w, stride=case.stride, padding=case.pad)
    else:
        wv = torch.zeros_like(b.dw, requires_grad=True)
        F.conv2d(V, wv, stride=case.stride, padding=case.pad).backward(b.dz)
        new = wv.grad
    return base, new


# ------------------------------------------------------------------------------------------------ the case lists of the sweep
def S(C, up=0, pro=False):
    return Src(C, up, pro)


# extents around the 8 x 16 pixel tile and the 128-pixel tile, both orientations, images that end inside a tile
EDGE_MAPS = [(1, 1, 1), (2, 1, 2), (1, 2, 15), (3, 3, 16), (1, 7, 17), (2, 8, 31), (1, 9, 33), (1, 17, 130), (5, 3, 2), (1, 130, 7),
             (3, 17, 9), (2, 16, 8), (1, 33, 15)]
# even extents for the forms that halve or double the map (up, pool2, stride 2)
EVEN_MAPS = [(1, 2, 2), (3, 2, 16), (1, 8, 18), (2, 6, 34), (1, 18, 130), (5, 4, 2), (1, 34, 6), (2, 16, 32), (1, 130, 8)]


def fwd_cases():
    cs = []
    for i, (N, H, W) in enumerate(EDGE_MAPS):
        Cc, K = [(64, 64), (32, 48), (128, 128), (64, 80), (96, 144), (32, 32), (192, 192)][i % 7]
        cs.append(Case(f"edge_n{N}_{H}x{W}_c{Cc}k{K}", "fwd", N, H, W, (S(Cc, 0, i % 2 == 0),), K, seed=i))
    for i, (N, H, W) in enumerate(EDGE_MAPS[::2]):               # the small-channel decoder layers (streaming kernels, 16-bit types)
        Cc, K = [(16, 16), (32, 32), (16, 16), (32, 32)][i % 4]
        cs.append(Case(f"dec_n{N}_{H}x{W}_c{Cc}k{K}", "fwd", N, H, W, (S(Cc, 0, True),), K, seed=20 + i))
    for i, (N, H, W) in enumerate(EVEN_MAPS):                    # decoder conv1: upsampled source (+ skip)
        srcs = [(S(64, 1, True), S(32)), (S(32, 1, True),), (S(128, 1, True), S(64, 0, True)), (S(32, 1, True),)][i % 4]
        K = [32, 16, 64, 16][i % 4]
        cs.append(Case(f"up_n{N}_{H}x{W}_c{sum(s.C for s in srcs)}k{K}", "fwd", N, H, W, tuple(srcs), K, seed=40 + i))
    for i, (N, H, W) in enumerate(EVEN_MAPS):                    # stride 2: 3x3 (the K >= 128 tile kernel and the tap kernel) and 1x1
        Cc, K = [(64, 128), (128, 256), (32, 64), (64, 192)][i % 4]
        cs.append(Case(f"s2_n{N}_{H}x{W}_c{Cc}k{K}", "fwd", N, H, W, (S(Cc, 0, i % 2 == 1),), K, stride=2, seed=60 + i))
        if i % 3 == 0:
            cs.append(Case(f"s2_1x1_n{N}_{H}x{W}_c{Cc}k{K}", "fwd", N, H, W, (S(Cc),), K, R=1, stride=2, pad=0, seed=80 + i))
    cs += [  # the network's deep layers and concat sums at their own (small) maps, non-square
        Case("l3_256_12x20", "fwd", 1, 12, 20, (S(256, 0, True),), 256, seed=90),
        Case("l4_512_5x9", "fwd", 2, 5, 9, (S(512, 0, True),), 512, seed=91),
        Case("dec0_768_10x6", "fwd", 1, 10, 6, (S(512, 1, True), S(256, 0, True)), 256, seed=92),
        Case("dec1_384_12x18", "fwd", 1, 12, 18, (S(256, 1, True), S(128)), 128, seed=93),
        Case("c320_k192_9x21", "fwd", 1, 9, 21, (S(320),), 192, seed=94),
    ]
    return cs


# channel counts outside what include/vk_unet.h and the dispatch document: a call refuses (outputs untouched) or is exact
def outside_cases():
    cs = []
    for i, (Cc, K) in enumerate([(8, 16), (24, 32), (40, 64), (64, 8), (32, 24), (64, 40), (16, 24)]):
        cs.append(Case(f"out_c{Cc}k{K}", "fwd", 2, 9, 17, (S(Cc, 0, i % 2 == 0),), K, seed=100 + i))
        cs.append(Case(f"out_c{Cc}k{K}", "wgrad", 2, 9, 17, (S(Cc, 0, i % 2 == 0),), K, seed=110 + i))
        cs.append(Case(f"out_c{K}k{Cc}", "dgrad", 2, 9, 17, (S(K),), Cc, seed=120 + i))
    # 48 channels: a multiple of the fp32 tile kernels' chunk (16) but not of the 32 every entry point asks for first
    cs.append(Case("out_c48k48", "fwd", 2, 7, 19, (S(48),), 48, seed=95))
    cs.append(Case("out_c48k48", "wgrad", 2, 7, 19, (S(48),), 48, seed=96))
    cs.append(Case("out_k48c32", "dgrad", 2, 7, 19, (S(48),), 32, seed=97))                # the gradient of a K = 48 layer reduces over 48 channels
    cs.append(Case("out_up_odd", "fwd", 1, 9, 17, (S(32, 0),), 32, seed=130))              # run with up = 1 on an odd map by the GPU test
    return cs


def splitk_cases():
    return [Case("sk_256_9x17", "fwd", 1, 9, 17, (S(256, 0, True),), 256, seed=140),
            Case("sk_512_7x5", "fwd", 1, 7, 5, (S(512, 0, True),), 512, seed=141),
            Case("sk_768_8x14", "fwd", 1, 8, 14, (S(512, 1), S(256, 0, True)), 256, seed=142),
            Case("sk_64_17x33", "fwd", 1, 17, 33, (S(64, 0, True),), 64, seed=143),
            Case("sk_128_n2_3x130", "fwd", 2, 3, 130, (S(128, 0, True),), 128, seed=144),
            Case("sk_320_k80_1x16", "fwd", 1, 1, 16, (S(320),), 80, seed=145)]


def dgrad_cases():
    cs = []
    for i, (N, H, W) in enumerate(EDGE_MAPS):                    # stride 1, plain and accumulating
        Kred, K = [(64, 64), (96, 48), (128, 128), (96, 80), (160, 96), (16, 32), (192, 192), (32, 16)][i % 8]
        cs.append(Case(f"s1_n{N}_{H}x{W}_k{Kred}c{K}", "dgrad", N, H, W, (S(Kred),), K, accumulate=i % 2, seed=200 + i))
    for i, (N, H, W) in enumerate(EVEN_MAPS):                    # stride 2: 3x3 and 1x1 (parity classes, the tile data-gradient kernel)
        Kred, K = [(128, 64), (256, 128), (64, 32), (192, 64)][i % 4]
        cs.append(Case(f"s2_n{N}_{H}x{W}_k{Kred}c{K}", "dgrad", N, H, W, (S(Kred),), K, stride=2, accumulate=(i // 2) % 2, seed=220 + i))
        if i % 2 == 0:
            cs.append(Case(f"s2_1x1_n{N}_{H}x{W}_k{Kred}c{K}", "dgrad", N, H, W, (S(Kred),), K, R=1, stride=2, pad=0, seed=240 + i))
    cs.append(Case("s2_odd_1x1_7x17", "dgrad", 1, 7, 17, (S(128),), 64, R=1, stride=2, pad=0, seed=250))
    cs.append(Case("s2_odd_3x3_9x15", "dgrad", 2, 9, 15, (S(128),), 64, stride=2, seed=251))
    for i, (N, H, W) in enumerate(EDGE_MAPS[2::3]):              # concat gradient: split at several k1
        Kred, K, k1 = [(64, 192, 128), (32, 96, 64), (128, 384, 256), (64, 48, 32)][i % 4]
        cs.append(Case(f"split{k1}_n{N}_{H}x{W}_k{Kred}c{K}", "dgrad", N, H, W, (S(Kred),), K, split=k1, seed=260 + i))
    return cs


def fused_cases():
    """vk_conv_dgrad_pool2 / vk_conv_dgrad_fused: every combination the header allows of pool2, bnr (affine or mask), bnr.accumulate, split.
    (The external mask does not combine with pool2.)"""
    cs = []
    combos = [(p, b, a, s) for p in (0, 1) for b in ("", "affine", "mask") for a in (0, 1) for s in (0, 1)
              if not (b == "mask" and p) and not (a and not b) and (p or b)]
    maps = [(1, 8, 18), (2, 6, 34), (3, 2, 16), (1, 18, 130), (5, 4, 2), (1, 34, 6), (1, 2, 2), (2, 16, 32)]
    chans = [(64, 192, 128), (32, 48, 32), (128, 192, 128), (16, 32, 16), (64, 96, 64), (32, 32, 16), (16, 16, 0)]
    for i, (p, bn, a, s) in enumerate(combos):
        for j in range(2):
            N, H, W = maps[(i + 3 * j) % len(maps)]
            Kred, K, k1 = chans[(i + 2 * j) % len(chans)]
            if not s or not k1:
                K, k1 = (k1 or K), 0
            cs.append(Case(f"p{p}_{bn or 'nobn'}_a{a}_split{k1}_n{N}_{H}x{W}_k{Kred}c{K}", "dgrad", N, H, W, (S(Kred),), K, split=k1, pool2=p,
                           bnr=bn, accumulate=a, seed=300 + 2 * i + j))
    # the streaming kernels' launches (16-bit): d(dec4.conv2) 16 -> 16, d(dec3.conv2) 32 -> 32 with bnr; d(dec4.conv1) 16 -> 32 pooled
    for i, (N, H, W) in enumerate([(1, 8, 18), (2, 34, 6), (1, 18, 130), (3, 2, 16)]):
        cs.append(Case(f"str_k16c16_n{N}_{H}x{W}", "dgrad", N, H, W, (S(16),), 16, bnr="affine", seed=360 + i))
        cs.append(Case(f"str_k32c32_n{N}_{H}x{W}", "dgrad", N, H, W, (S(32),), 32, bnr="affine", seed=364 + i))
        cs.append(Case(f"str_k16c32_pool_n{N}_{H}x{W}", "dgrad", N, H, W, (S(16),), 32, pool2=1, bnr="affine", seed=368 + i))
    cs.append(Case("pool_odd_9x17", "dgrad", 1, 9, 17, (S(64),), 64, seed=380))             # run with pool2 = 1 on an odd map by the GPU test
    return cs


def wgrad_cases():
    cs = []
    for i, (N, H, W) in enumerate(EDGE_MAPS):
        Cc, K = [(64, 64), (32, 48), (128, 128), (32, 16), (96, 144), (32, 32), (16, 16), (64, 80)][i % 8]
        cs.append(Case(f"edge_n{N}_{H}x{W}_c{Cc}k{K}", "wgrad", N, H, W, (S(Cc, 0, i % 2 == 0),), K, seed=400 + i))
    for i, (N, H, W) in enumerate(EVEN_MAPS):
        srcs = [(S(64, 1, True), S(64)), (S(32, 1, True),), (S(128, 1), S(64, 0, True)), (S(32, 1, True),)][i % 4]
        K = [64, 16, 64, 32][i % 4]
        cs.append(Case(f"up_n{N}_{H}x{W}_c{sum(s.C for s in srcs)}k{K}", "wgrad", N, H, W, tuple(srcs), K, seed=420 + i))
        Cc, K = [(64, 128), (32, 64), (128, 256)][i % 3]
        cs.append(Case(f"s2_n{N}_{H}x{W}_c{Cc}k{K}", "wgrad", N, H, W, (S(Cc, 0, True),), K, stride=2, seed=440 + i))
        if i % 3 == 0:
            cs.append(Case(f"s2_1x1_n{N}_{H}x{W}_c{Cc}k{K}", "wgrad", N, H, W, (S(Cc),), K, R=1, stride=2, pad=0, seed=460 + i))
    cs += [Case("l3_256_12x20", "wgrad", 1, 12, 20, (S(256, 0, True),), 256, seed=470),
           Case("l4_512_5x9", "wgrad", 2, 5, 9, (S(512),), 512, seed=471),
           Case("dec1_384_12x18", "wgrad", 1, 12, 18, (S(256, 1, True), S(128)), 128, seed=472)]
    return cs


def batch_layers():
    """Layers of the class vk_conv_wgrad_batch runs (16-bit, 3x3 stride 1, K >= 64, sources multiples of 64 channels), ragged and non-square."""
    return [Case("b0", "wgrad", 2, 9, 33, (S(64, 0, True),), 64, seed=480), Case("b1", "wgrad", 1, 17, 15, (S(128),), 128, seed=481),
            Case("b2", "wgrad", 3, 2, 16, (S(128, 1, True), S(64)), 64, seed=482), Case("b3", "wgrad", 1, 7, 130, (S(64),), 192, seed=483),
            Case("b4", "wgrad", 5, 3, 2, (S(192),), 64, seed=484)]


def conv1x1_cases():
    cs = []
    for i, (N, H, W) in enumerate(EDGE_MAPS[::2] + EVEN_MAPS[::3]):
        Cc, K = [(64, 256), (40, 24), (256, 64), (24, 136), (512, 128)][i % 5]
        for s in (1, 2):
            cs.append(Case(f"n{N}_{H}x{W}_c{Cc}k{K}_s{s}", "fwd", N, H, W, (S(Cc, 0, i % 2 == 0),), K, R=1, stride=s, pad=0, seed=500 + 2 * i + s))
            cs.append(Case(f"n{N}_{H}x{W}_k{K}c{Cc}_s{s}", "dgrad", N, H, W, (S(K),), Cc, R=1, stride=s, pad=0, accumulate=i % 2, seed=530 + 2 * i + s))
            cs.append(Case(f"n{N}_{H}x{W}_c{Cc}k{K}_s{s}", "wgrad", N, H, W, (S(Cc, 0, i % 2 == 1),), K, R=1, stride=s, pad=0, seed=560 + 2 * i + s))
    return cs


def large_cases():
    """One case per kernel family at a full-network layer shape (batch cut to what a float64 reference on the host does in about a
    second), so grid-stride and persistent loops take more than one trip on the 256 compute units: the number of 8 x 16 pixel tiles
    (times output-channel tiles) is 4096 (dec4), 2048 (dec3), 1024 (l1), 512 (l2), 512 (up + concat), 512 (stride 2, output tiles),
    and the 1x1 and stem kernels see 32768 and 131072 output pixels."""
    return [Case("large_dec4_c16_512x512", "fwd", 2, 512, 512, (S(16, 0, True),), 16, types=("bf16",), seed=600),
            Case("large_dec3_c32_256x256", "fwd", 4, 256, 256, (S(32, 0, True),), 32, density=0.1, types=("f16",), seed=601),          # thinner: condition 5 on 256-row strips
            Case("large_l1_c64_128x128", "fwd", 8, 128, 128, (S(64, 0, True),), 64, types=("bf16",), seed=602),
            Case("large_l2_c128_64x64", "fwd", 16, 64, 64, (S(128),), 128, types=("bf16",), seed=603),
            Case("large_up_dec2_c192_128x128", "fwd", 4, 128, 128, (S(128, 1, True), S(64)), 64, types=("bf16",), seed=608),
            Case("large_s2_l2_c64k128_128x128", "fwd", 16, 128, 128, (S(64, 0, True),), 128, stride=2, types=("f16",), seed=609),
            Case("large_d_dec4_512x512", "dgrad", 2, 512, 512, (S(16),), 16, bnr="affine", types=("bf16",), seed=604),
            Case("large_d_l1_128x128", "dgrad", 8, 128, 128, (S(64),), 64, types=("f16",), seed=605),
            Case("large_w_dec3_256x256", "wgrad", 2, 256, 256, (S(32, 0, True),), 32, types=("bf16",), seed=606),
            Case("large_w_l1_128x128", "wgrad", 8, 128, 128, (S(64),), 64, types=("bf16",), seed=607)]


def large_conv1x1_cases():
    """The pointwise kernels at a resnet50 layer1 shape: 8 x 64 x 64 pixels, 256 <-> 64 channels."""
    return [Case("large_1x1_c256k64", "fwd", 8, 64, 64, (S(256, 0, True),), 64, R=1, pad=0, types=("bf16",), seed=610),
            Case("large_1x1_k64c256", "dgrad", 8, 64, 64, (S(64),), 256, R=1, pad=0, types=("f16",), seed=611),
            Case("large_1x1_c256k64", "wgrad", 8, 64, 64, (S(256),), 64, R=1, pad=0, types=("bf16",), seed=612)]


def all_cases():
    return (fwd_cases() + outside_cases() + splitk_cases() + dgrad_cases() + fused_cases() + wgrad_cases() + batch_layers() +
            conv1x1_cases() + large_cases() + large_conv1x1_cases())
