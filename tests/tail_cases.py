"""Cases and float64 references for the tail of a training step: the segmentation head (binary and multi-class), the fused inference tail
vk_dec4_tail_eval, BCE+Dice, AdamW and the GradScaler kernels (no GPU needed; tests/test_tail_cases_cpu.py checks this module,
tests/test_tail_sweep_gpu.py runs the kernels on its cases).  Same method as tests/conv_lattice.py.

EXACT tier.  The head kernels accumulate in fp32 (packed FMAs, MFMA with fp32 accumulators, fp32 per-workgroup partials or fp32 atomics,
fp32 BatchNorm-backward partials followed by fp64 atomics).  With small integers as activations, filter, bias and dlogits, prologue scales
from {0.5, 1, 2} and integer shifts, every product and partial sum is an integer or a half far below 2^24 in any order, and the values
the matrix-core route rounds to the 16-bit type (relu(bn(z)), the filter, dlogits, the stored dy) survive that rounding: the result must
EQUAL float64 in f32, bf16 and f16, on every route, workspace size and atomics order.  AdamW has its own exact tier: with
beta1 = 1/2, beta2 = 3/4, eps = 0, lr = 2^-10, weight_decay = 2^-3, zero moments, p on the 1/16 grid in [-4, 4] and integer gradients
times a power of two, the first step is m = g/2, v = g^2/4, p' = p (1 - 2^-13) - 2^-10 sign(g), every intermediate exact in fp32 whether
or not the compiler contracts to FMA.

The references are written from the formulas of include/vk_unet.h and torch/optim/adam.py as explicit sums (no convolution operator, no
optimizer class), so that tests/test_tail_cases_cpu.py can hold each against an independent twin: F.conv2d autograd, torch.optim.AdamW
on float64 tensors, the oracle's DiceLoss plus torch's BCE.

ROUNDED tier.  Bounds are formulas of this module (sum_bound, loss_bounds, loss_grad_bound, adamw_bounds) counted from the kernels'
chains of fp32 operations; their only measured input is K_FUNC."""
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv_lattice import LIM, TDT, TWO24, exact_in, ints, lat_int, lat_scale, ternary

U32 = 2.0 ** -24            # unit round-off of fp32
TINY = 2.0 ** -149          # spacing of the fp32 subnormals: the most an operation that underflows can lose
P_FLOOR = 2.0 ** -126       # 1 / (1 + expf(-x)) is 0 where expf(-x) overflows (x < -88.72), in place of a value below 2^-127
# Error of the device's expf / log1pf / division inside log1pf(expf(-|x|)) and 1 / (1 + expf(-x)).  No table of it exists, so it is
# measured once with tools/ulp_probe.hip on 2^25 arguments in [-104, 104] (profiles/tailsweep/README.md has the figures): expf 1.00,
# the softplus expression 1.61, the sigmoid expression 2.56 ulp where expf(-x) is finite.  The grid is not exhaustive, hence twice the
# measured maximum; one ulp is at most 2 x 2^-24 of the value, so in units of 2^-24 relative to the result the function error is
# K_FUNC = 2 x 2 x 2.5634.
K_ULP_MEASURED = 2.5634
K_FUNC = 2.0 * 2.0 * K_ULP_MEASURED


# ================================================================================================ segmentation head
@dataclass(frozen=True)
class HeadCase:
    """C = 0: the binary head (vk_head_fwd / vk_head_bwd / vk_head_bwd_fused); C >= 1: vk_head_fwd_multi / vk_head_bwd_multi with C classes.
    affine: src->scale / shift given (else NULL).  relu: src->relu.  bnr: "" (none), "own" (the head's source tensor and coefficients: what
    the training plan asks for, the matrix-core route in the 16-bit types), "other" (another tensor with its own scale and shift) or
    "own_z" (the head's source tensor with coefficients of its own, for a source without an affine)."""
    name: str
    N: int
    H: int
    W: int
    C: int = 0
    relu: int = 1
    affine: bool = True
    bnr: str = "own"
    types: tuple = ("f32", "bf16", "f16")
    seed: int = 0

    @property
    def classes(self):
        return max(self.C, 1)

    @property
    def tiles(self):
        return self.N * ((self.H + 15) // 16) * ((self.W + 15) // 16)


def head_density(case):
    """Ternary filter of the multi-class head: dy is a sum of 9 C products |dl| |w| <= 2, at most 18 C; it must stay an integer below
    256 (bf16), so above 8 classes half of the filter is zero (144 at the very most)."""
    return 1.0 if case.classes <= 8 else 0.5


def taps(xp, H, W):
    """The nine shifted views of a map padded by one pixel: view (r, s) holds xp[.., y + r, x + s]."""
    return [(r, s, xp[:, :, r:r + H, s:s + W]) for r in range(3) for s in range(3)]


def head_build(case):
    """Operands (float64, NCHW, filter [C][16][3][3]) and expected results of one case, from the formulas of include/vk_unet.h:
        a      = z * scale + shift, then max(., 0) when relu (only with scale / shift: a source without them is read as it is)
        logits = bias[c] + sum_{r, s, ch} w[c][ch][r][s] a[n][ch][y + r - 1][x + s - 1]
        dy     = sum_{c, r, s} w[c][ch][r][s] dl[n][c][y + 1 - r][x + 1 - s];  g = dy * [bz * bscale + bshift > 0] with bnr
        dw     = sum_{n, y, x} dl[n][c][y][x] a[n][ch][y + r - 1][x + s - 1];  db = sum dl
        sums   = sum g, sum g * bz per channel"""
    g = torch.Generator().manual_seed(5000 + case.seed)
    N, H, W, Cc = case.N, case.H, case.W, case.classes
    b = SimpleNamespace(case=case)
    b.z = ints((N, 16, H, W), -2, 2, g)
    b.scale = lat_scale(16, 0) if case.affine else None
    b.shift = lat_int(16, 3, 7) if case.affine else None
    a = b.z
    if case.affine:
        a = a * b.scale.view(1, -1, 1, 1) + b.shift.view(1, -1, 1, 1)
        if case.relu:
            a = torch.relu(a)
    b.a = a
    b.w = ints((1, 16, 3, 3), -2, 2, g) if case.C == 0 else ternary((Cc, 16, 3, 3), head_density(case), g)
    b.bias = ints((Cc,), -3, 3, g)
    b.dl = ints((N, Cc, H, W), -2, 2, g)
    b.dw0 = ints((Cc, 16, 3, 3), -3, 3, g)                    # dw / dbias accumulate: they start from integers of their own
    b.db0 = ints((Cc,), -3, 3, g)
    ap, dlp = F.pad(a, (1, 1, 1, 1)), F.pad(b.dl, (1, 1, 1, 1))
    b.logits = b.bias.view(1, -1, 1, 1).expand(N, Cc, H, W).clone()
    b.absdot = b.bias.abs().view(1, -1, 1, 1).expand(N, Cc, H, W).clone()
    b.dw = torch.zeros(Cc, 16, 3, 3, dtype=torch.float64)
    b.dw_abs = torch.zeros_like(b.dw)
    for r, s, v in taps(ap, H, W):
        b.logits += torch.einsum("nchw,kc->nkhw", v, b.w[:, :, r, s])
        b.absdot += torch.einsum("nchw,kc->nkhw", v.abs(), b.w[:, :, r, s].abs())
        b.dw[:, :, r, s] = torch.einsum("nkhw,nchw->kc", b.dl, v)
        b.dw_abs[:, :, r, s] = torch.einsum("nkhw,nchw->kc", b.dl.abs(), v.abs())
    b.dy = torch.zeros(N, 16, H, W, dtype=torch.float64)
    b.dy_abs = torch.zeros_like(b.dy)
    for r, s, v in taps(dlp, H, W):                            # view (2 - r', 2 - s') of dl is dl[y + 1 - r', x + 1 - s']
        b.dy += torch.einsum("nkhw,kc->nchw", v, b.w[:, :, 2 - r, 2 - s])
        b.dy_abs += torch.einsum("nkhw,kc->nchw", v.abs(), b.w[:, :, 2 - r, 2 - s].abs())
    b.db = b.dl.sum(dim=(0, 2, 3))
    b.bz = b.bscale = b.bshift = b.sums = None
    b.g = b.dy
    if case.bnr:
        if case.bnr == "own":
            assert case.affine
            b.bz, b.bscale, b.bshift = b.z, b.scale, b.shift
        else:
            b.bz = b.z if case.bnr == "own_z" else ints((N, 16, H, W), -3, 3, g)
            b.bscale, b.bshift = lat_scale(16, 1), lat_int(16, 2, 5)
        keep = (b.bz * b.bscale.view(1, -1, 1, 1) + b.bshift.view(1, -1, 1, 1)) > 0
        b.g = b.dy * keep
        b.sums = torch.stack([b.g.sum(dim=(0, 2, 3)), (b.g * b.bz).sum(dim=(0, 2, 3))])
    return b


def head_check(b):
    """The exactness conditions, on the reference alone.  Returns the figures it checked."""
    c = b.case
    fig = {"max_a": b.a.abs().max().item(), "max_dy": b.dy_abs.max().item(), "max_logit_absdot": b.absdot.max().item(),
           "max_dw_absdot": b.dw_abs.max().item()}
    for dtn in c.types:
        # stored values and staged operands: z, relu(bn(z)) (staged as the element type by the matrix-core route), the filter and dlogits
        # (rounded to it there), dy before and after the mask; sum |dl| |w| bounds every partial sum of the data gradient
        for nm in ("z", "a", "w", "dl", "dy", "g", "bz"):
            t = getattr(b, nm)
            assert t is None or exact_in(t, dtn), f"{c.name}: {nm} is not exact in {dtn} (max {t.abs().max().item()})"
        assert fig["max_dy"] <= LIM[dtn], f"{c.name}: sum |dl| |w| reaches {fig['max_dy']} in {dtn}"
    assert fig["max_logit_absdot"] < TWO24 and exact_in(b.logits, "f32")
    # dw / dbias accumulate onto integers of their own: what was there plus every partial sum stays exact
    assert fig["max_dw_absdot"] + b.dw0.abs().max().item() < TWO24, f"{c.name}: sum |dl| |a| reaches {fig['max_dw_absdot']}"
    assert exact_in(2.0 * (b.dw0 + b.dw), "f32") and exact_in(2.0 * (b.db0 + b.db), "f32")
    assert b.dl.abs().sum().item() + b.db0.abs().max().item() < TWO24
    if b.sums is not None:
        fig["sum_abs_g"] = b.g.abs().sum(dim=(0, 2, 3)).max().item()
        fig["sum_abs_gz"] = (b.g * b.bz).abs().sum(dim=(0, 2, 3)).max().item()
        assert fig["sum_abs_g"] < TWO24 and fig["sum_abs_gz"] < TWO24, f"{c.name}: BN-backward sums reach {fig}"
    return fig


def head_twin(b):
    """The same quantities from F.conv2d autograd in float64."""
    a = b.a.clone().requires_grad_(True)
    w = b.w.clone().requires_grad_(True)
    bias = b.bias.clone().requires_grad_(True)
    out = F.conv2d(a, w, bias, padding=1)
    out.backward(b.dl)
    return out.detach(), a.grad, w.grad, bias.grad


HEAD_MAPS = [(1, 1, 2), (2, 2, 1), (3, 15, 16), (1, 16, 15), (5, 17, 33), (2, 33, 17), (1, 1, 33), (3, 33, 1), (2, 16, 17), (1, 17, 16),
             (2, 15, 2), (1, 2, 15), (5, 16, 33), (3, 17, 15)]
# (relu, affine, bnr)
HEAD_VARIANTS = [(1, True, "own"), (0, True, "own"), (1, True, ""), (1, True, "other"), (0, True, "other"), (1, False, "other"),
                 (0, False, ""), (1, False, "own_z")]


def vname(relu, affine, bnr):
    return f"relu{relu}_{'aff' if affine else 'noaff'}_{bnr or 'nobnr'}"


def head_cases():
    """Every variant on four maps (both orientations of a ragged two-tile map, a one-pixel-high map, a map of whole tiles plus one
    column), and one variant, in rotation, on each of the other maps."""
    cs = []
    full = [(5, 17, 33), (2, 33, 17), (1, 1, 33), (2, 16, 17)]
    for i, (N, H, W) in enumerate(HEAD_MAPS):
        vs = HEAD_VARIANTS if (N, H, W) in full else [HEAD_VARIANTS[i % len(HEAD_VARIANTS)]]
        for j, (relu, aff, bnr) in enumerate(vs):
            cs.append(HeadCase(f"n{N}_{H}x{W}_{vname(relu, aff, bnr)}", N, H, W, 0, relu, aff, bnr, seed=10 * i + j))
    return cs


def head_multi_cases():
    cs = []
    for i, (N, H, W) in enumerate(HEAD_MAPS):
        Cc = [1, 2, 3, 8, 16][i % 5]
        relu, aff, bnr = HEAD_VARIANTS[(i * 3) % len(HEAD_VARIANTS)]
        cs.append(HeadCase(f"c{Cc}_n{N}_{H}x{W}_{vname(relu, aff, bnr)}", N, H, W, Cc, relu, aff, bnr, seed=200 + i))
    for i, Cc in enumerate([1, 2, 3, 8, 16]):                  # every class count on the ragged two-tile map, both bnr routes
        cs.append(HeadCase(f"c{Cc}_n2_33x17_relu1_aff_own", 2, 33, 17, Cc, 1, True, "own", seed=220 + i))
        cs.append(HeadCase(f"c{Cc}_n3_17x33_relu0_aff_other", 3, 17, 33, Cc, 0, True, "other", seed=230 + i))
    return cs


def head_large_cases():
    """Tile counts past the launch caps (k_head_dgrad 2,048 workgroups; k_head_wgrad, k_head_bwd_mfma and k_head_bwd_multi 1,024), so
    that the persistent loops with their double-buffered dlogits staging take a second trip: 513 images of 17 x 17 are 2,052 ragged
    tiles at 148 k pixels; 2 images of 368 x 368 are 1,058 full tiles."""
    return [HeadCase("ragged_2052_tiles_own", 513, 17, 17, 0, 1, True, "own", seed=300),
            HeadCase("ragged_2052_tiles_other", 513, 17, 17, 0, 1, True, "other", seed=301),
            HeadCase("full_1058_tiles_own", 2, 368, 368, 0, 1, True, "own", types=("f32", "bf16"), seed=302),
            HeadCase("c3_ragged_2052_tiles_own", 513, 17, 17, 3, 1, True, "own", seed=303),
            HeadCase("c2_full_1058_tiles_other", 2, 368, 368, 2, 1, True, "other", types=("f16",), seed=304)]


def all_head_cases():
    return head_cases() + head_multi_cases() + head_large_cases()


# ================================================================================================ vk_dec4_tail_eval
@dataclass(frozen=True)
class TailCase:
    name: str
    N: int
    H: int
    W: int
    d1: float = 0.04           # share of non-zero weights of conv1 (288 products per output)
    d2: float = 0.05           # and of conv2 (144)
    types: tuple = ("bf16", "f16")
    seed: int = 0


def half_or_one(Cn, k):
    """{0.5, 1} by channel with period 2 (k = 0) or 4 (k = 1): scales that never widen the range."""
    c = torch.arange(Cn)
    return torch.tensor([1.0, 0.5], dtype=torch.float64)[(c // 2 ** k) % 2]


def tail_build(case):
    """Decoder block 4 + head in eval mode on a three-stage lattice (formulas: include/vk_unet.h, vk_dec4_tail_eval):
        V0 = up2(relu(x * s0 + h0))          x: 32 channels at half resolution, even integers, s0 from {0.5, 1, 2}: V0 is an integer <= 7
        z1 = conv3x3(V0, w1)                 ternary, density d1;  stored in the element type by the separate calls
        a1 = relu(z1 * s1 + h1)              s1 from {0.5, 1}: a1 is a multiple of 1/2
        z2 = conv3x3(a1, w2)                 ternary, density d2: a multiple of 1/2
        a2 = relu(z2 * s2 + h2)              s2 from {0.5, 1}: a multiple of 1/4
        logits = head(a2)                    ternary head filter, integer bias
    Every intermediate must survive rounding to bf16 (8 significant bits) and f16; tail_check proves it for each case."""
    g = torch.Generator().manual_seed(7000 + case.seed)
    N, H, W = case.N, case.H, case.W
    b = SimpleNamespace(case=case)
    b.x = 2.0 * ints((N, 32, (H + 1) // 2, (W + 1) // 2), -1, 1, g)     # (an odd extent, outside the documented set, reads h >> 1 too)
    b.s0, b.h0 = lat_scale(32, 0), lat_int(32, 3, 7)
    b.V0 = F.interpolate(torch.relu(b.x * b.s0.view(1, -1, 1, 1) + b.h0.view(1, -1, 1, 1)), scale_factor=2, mode="nearest")[:, :, :H, :W]
    b.w1 = ternary((16, 32, 3, 3), case.d1, g)
    b.s1, b.h1 = half_or_one(16, 0), lat_int(16, 3, 7)
    b.w2 = ternary((16, 16, 3, 3), case.d2, g)
    b.s2, b.h2 = half_or_one(16, 1), lat_int(16, 2, 5)
    b.hw = ternary((1, 16, 3, 3), 0.5, g)
    b.hb = ints((1,), -3, 3, g)

    def conv(v, w):
        vp, out, absd = F.pad(v, (1, 1, 1, 1)), 0.0, 0.0
        for r, s, t in taps(vp, H, W):
            out = out + torch.einsum("nchw,kc->nkhw", t, w[:, :, r, s])
            absd = absd + torch.einsum("nchw,kc->nkhw", t.abs(), w[:, :, r, s].abs())
        return out, absd

    b.z1, b.abs1 = conv(b.V0, b.w1)
    b.a1 = torch.relu(b.z1 * b.s1.view(1, -1, 1, 1) + b.h1.view(1, -1, 1, 1))
    b.z2, b.abs2 = conv(b.a1, b.w2)
    b.a2 = torch.relu(b.z2 * b.s2.view(1, -1, 1, 1) + b.h2.view(1, -1, 1, 1))
    lg, b.abs3 = conv(b.a2, b.hw)
    b.logits = lg + b.hb.view(1, -1, 1, 1)
    return b


def tail_check(b):
    c = b.case
    fig = {nm: getattr(b, nm).abs().max().item() for nm in ("V0", "z1", "a1", "z2", "a2", "logits")}
    for dtn in c.types:
        for nm in ("x", "V0", "w1", "z1", "a1", "w2", "z2", "a2", "hw"):
            assert exact_in(getattr(b, nm), dtn), f"{c.name}: {nm} is not exact in {dtn} (max {fig.get(nm)})"
        # every partial sum of the two convolutions, in any order, stays on the same grid below the type's exact range: also a kernel
        # that kept an intermediate accumulator in the element type would be exact
        assert b.abs1.max().item() <= LIM[dtn] / 2 and b.abs2.max().item() <= LIM[dtn] / 2
    assert b.abs3.max().item() + 3.0 < TWO24 and exact_in(b.logits, "f32")
    return fig


def tail_twin(b):
    z1 = F.conv2d(b.V0, b.w1, padding=1)
    a1 = torch.relu(z1 * b.s1.view(1, -1, 1, 1) + b.h1.view(1, -1, 1, 1))
    z2 = F.conv2d(a1, b.w2, padding=1)
    a2 = torch.relu(z2 * b.s2.view(1, -1, 1, 1) + b.h2.view(1, -1, 1, 1))
    return F.conv2d(a2, b.hw, b.hb, padding=1)


def tail_outside_cases():
    """Outside what include/vk_unet.h documents (H, W multiples of 16; 16-bit types): refused with the logits untouched, or exact."""
    return [TailCase("odd_17x16", 1, 17, 16, seed=20), TailCase("odd_16x24", 1, 16, 24, seed=21), TailCase("f32_16x16", 1, 16, 16, types=("f32",), seed=22)]


def tail_cases():
    return [TailCase(f"n{N}_{H}x{W}", N, H, W, seed=i) for i, (N, H, W) in
            enumerate([(1, 16, 48), (3, 48, 16), (1, 32, 80), (3, 16, 16), (1, 16, 16), (3, 32, 80)])]


# ================================================================================================ BCE + Dice
def loss_ref(x, y, w_bce, w_dice):
    """x, y: fp32 tensors.  float64 of include/vk_unet.h's vk_bce_dice_loss: mean BCE-with-logits + batch-global binary Dice (smooth 0,
    eps 1e-7, masked to 0 for an empty target), and its gradient with respect to the logits."""
    x, y = x.double().flatten(), y.double().flatten()
    count = x.numel()
    sp = torch.log1p(torch.exp(-x.abs()))
    p = 1.0 / (1.0 + torch.exp(-x))
    r = SimpleNamespace(count=count, p=p)
    r.bce_terms = torch.clamp(x, min=0.0) - x * y + sp
    r.bce_mag = torch.clamp(x, min=0.0) + (x * y).abs() + sp            # what the three fp32 operations of a term are relative to
    r.sums = [r.bce_terms.sum().item(), (p * y).sum().item(), p.sum().item(), y.sum().item()]
    S0, I, P, T = r.sums
    r.bce = S0 / count
    card = P + T
    r.card, r.I = card, I
    r.clamped = not card > 1e-7
    denom = card if card > 1e-7 else 1e-7
    r.mask = 1.0 if T > 0.0 else 0.0
    r.dice = (1.0 - 2.0 * I / denom) * r.mask
    r.total = w_bce * r.bce + w_dice * r.dice
    r.ky = 0.0 if r.clamped else -2.0 * w_dice * r.mask / card          # multiplies y_i
    r.k0 = 0.0 if r.clamped else 2.0 * w_dice * r.mask * I / (card * card)
    r.invc = w_bce / count
    r.grad = (p - y) * r.invc + (r.ky * y + r.k0) * p * (1.0 - p)
    r.y = y
    return r


def loss_terms_per_thread(count, vec):
    """Most fp32 terms one thread of k_loss_reduce adds up: 2,048 x 256 threads walk count / 4 vectors (vec) or count elements."""
    work = (count + 3) // 4 if vec else count
    threads = 256 * min(max((work + 255) // 256, 1), 2048)
    if vec:
        return 4 * (-(-(count // 4) // threads)) + 1                  # vectors of 4, then at most one element of the scalar tail
    return -(-count // threads)


def sum_bound(n_thread, extra, mag, count, floor=0.0):
    """A thread adds n_thread fp32 terms (n_thread roundings, each relative to a partial sum of at most sum |terms|) that each carry a
    relative error of (K_FUNC + extra) x 2^-24 (the function and `extra` fp32 operations of the term); a term in the subnormal range
    carries that error as a multiple of the spacing TINY instead, and each of the `count` terms of the whole sum may (all logits at
    -100: every BCE term is expf(-100) = 3.7e-44);
    the partial sums then go on in fp64 (2^-53 per addition: 1e-12 relative covers 2^22 of them).  floor: absolute error of all terms
    together that is not relative to them (the sigmoid where expf overflows)."""
    return (n_thread + K_FUNC + extra) * U32 * mag * (1.0 + 1e-6) + 1e-12 * mag + count * (K_FUNC + extra + 1.0) * TINY + floor


def loss_bounds(r, vec, w_bce, w_dice, soft):
    """Bounds of sums[0..3] and loss_out[0..2] against loss_ref."""
    n = loss_terms_per_thread(r.count, vec)
    bd = SimpleNamespace()
    bd.s0 = sum_bound(n, 3, r.bce_mag.sum().item(), r.count)                     # max, product, two additions: 3 roundings besides log1pf(expf)
    bd.s1 = sum_bound(n, 1, r.sums[1], r.count, r.count * P_FLOOR)               # p * y
    bd.s2 = sum_bound(n, 0, r.sums[2], r.count, r.count * P_FLOOR)
    bd.s3 = sum_bound(n, 0, r.sums[3], r.count) if soft else 0.0                 # 0 / 1 targets: integers below 2^24 per thread, exact
    bd.bce = bd.s0 / r.count + U32 * abs(r.bce)
    dcard = bd.s2 + bd.s3
    bd.dcard, bd.dI = dcard, bd.s1
    if r.clamped or r.mask == 0.0:
        bd.dice = 0.0
    else:
        lo = r.card - dcard
        bd.dice = 2.0 * bd.s1 / lo + 2.0 * r.I * dcard / (r.card * lo) + U32 * abs(r.dice)
    bd.total = w_bce * bd.bce + w_dice * bd.dice + U32 * abs(r.total)
    return bd


def loss_grad_bound(r, bd, w_dice):
    """Elementwise bound of dlogits / grad_scale against loss_ref.grad, counted along k_loss_bwd:
        p = 1 / (1 + expf(-x))                         K_FUNC x 2^-24 relative (P_FLOOR absolute where expf overflows)
        t1 = (p - y) * invc                            subtraction, invc rounded to fp32, product: 3 roundings
        c = ky * y + k0                                ky, k0 rounded to fp32 from fp64 sums that carry bd.dI, bd.dcard; product, addition
        t2 = c * p * (1 - p)                           subtraction and two products
        g = t1 + t2; dlogits = g * grad_scale          two more roundings (none when contracted or for a power of two: not relied on)"""
    p, y = r.p, r.y
    ep = K_FUNC * U32 * p + P_FLOOR
    t1 = (p - y) * r.invc
    e_t1 = abs(r.invc) * (ep + U32 * (p - y).abs()) + 2.0 * U32 * t1.abs()
    if r.clamped or r.mask == 0.0:
        dky = dk0 = 0.0
    else:
        lo = r.card - bd.dcard
        dky = abs(r.ky) * bd.dcard / lo + U32 * abs(r.ky)
        dk0 = 2.0 * w_dice * (bd.dI / (lo * lo) + 2.0 * r.I * bd.dcard / (lo * lo * lo)) + U32 * abs(r.k0)
    c = r.ky * y + r.k0
    e_c = dky * y.abs() + dk0 + U32 * (r.ky * y).abs() + U32 * c.abs()
    q = 1.0 - p
    e_q = ep + U32 * q
    t2 = c * p * q
    e_t2 = e_c * p * q + c.abs() * (ep * q + p * e_q) + 2.0 * U32 * t2.abs()
    g = t1 + t2
    return (e_t1 + e_t2 + 2.0 * U32 * g.abs()) * (1.0 + 1e-6) + 4.0 * TINY


LOSS_COUNTS = [1, 3, 4, 5, 1023, 1025, 2 ** 21 + 5]       # 2^21 + 5: past the 2,048 x 256 x 4 cap of the vector route and 4,096 x 256 of k_loss_bwd
LOSS_SCALAR_LARGE = 2 ** 19 + 3                           # past the 2,048 x 256 cap of the scalar route


def loss_inputs(count, kind, seed):
    """kind "hard": y in {0, 1}; "soft": y in (0, 1).  Logits: seeded normal x 3 with some exact zeros."""
    g = torch.Generator().manual_seed(9000 + seed)
    x = torch.randn(count, generator=g) * 3.0
    x[torch.rand(count, generator=g) < 0.05] = 0.0
    if kind == "hard":
        y = (torch.rand(count, generator=g) > 0.7).float()
    else:
        y = torch.rand(count, generator=g) * 0.98 + 0.01
    return x, y


# ================================================================================================ AdamW
EXACT_HP = dict(lr=2.0 ** -10, beta1=0.5, beta2=0.75, eps=0.0, wd=2.0 ** -3)
DEFAULT_HP = dict(lr=5e-5, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4)
ADAMW_SIZES = [1, 2, 3, 255, 257, 4097, 2 ** 20 + 3]


def f32(v):
    """A Python float as the fp32 value the C ABI receives."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def adamw_ref(p, g, m, v, hp, t, factor):
    """One step of torch/optim/adam.py's single-tensor AdamW in float64 on fp32 state: p, g, m, v fp32 tensors, hyper-parameters as the
    fp32 values the kernel receives, gradient multiplied by `factor` first (inv_scale / grad_scale).  Returns float64 (p', m', v')."""
    lr, b1, b2, eps, wd = (f32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    p, g, m, v = p.double(), g.double() * factor, m.double(), v.double()
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def adamw_bounds(p, g, m, v, hp, t, factor):
    """Elementwise bounds of (p', m', v') against adamw_ref, counted along adamw_elem (csrc/optim.hip) WITHOUT contraction (a fused
    multiply-add rounds once where this counts twice); sqrtf and / are correctly rounded under csrc/Makefile's flags.  u = 2^-24.
        gi = g * factor                              1 rounding, and factor itself (inv_scale / grad_scale to fp32): 2 u |gi|
        d = gi - m; e = d * (1 - beta1); m' = m + e  (1 - beta1) in fp32 is 1 more: (1 - beta1)(2 u |gi| + u |d|) + 2 u |e| + u |m'|
        v' = v * beta2 + ((1 - beta2) * gi) * gi     u |v beta2| + (1 + 2 + 4) u (1 - beta2) gi^2 + u |v'|
        s = sqrtf(v') / bc2_sqrt + eps               |sqrt a - sqrt b| <= min(sqrt |a - b|, |a - b| / sqrt b); bc2_sqrt rounded to fp32
        r = m' / s; p' = p * (1 - lr * wd) - step_size * r      step_size rounded to fp32
    TINY is added wherever an operation can underflow."""
    lr, b1, b2, eps, wd = (f32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    u = U32
    pr, mr, vr = adamw_ref(p, g, m, v, hp, t, factor)
    p, m, v = p.double(), m.double(), v.double()
    gi = g.double() * factor
    d = gi - m
    e = d * (1.0 - b1)
    bm = (1.0 - b1) * (2.0 * u * gi.abs() + u * d.abs()) + 2.0 * u * e.abs() + u * mr.abs() + 3.0 * TINY
    bv = u * (v * b2).abs() + 7.0 * u * (1.0 - b2) * gi * gi + u * vr.abs() + 4.0 * TINY
    bc1, bc2s = 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5
    sq = vr.sqrt()
    ds = torch.minimum(bv.sqrt(), bv / sq.clamp_min(1e-300)) + u * sq
    s = sq / bc2s + eps
    dsd = ds / bc2s + 2.0 * u * sq / bc2s + u * s + TINY
    lo = (s - dsd).clamp_min(1e-300)
    r = mr / s
    # where the denominator is not known to better than itself (v' = 0 with eps = 0) the quotient is only defined for m' = 0
    dr = bm / lo + mr.abs() * dsd / (s * lo) + u * r.abs() + TINY
    dr = torch.where((mr == 0) & (bm <= 3.0 * TINY), torch.zeros_like(dr), dr)
    step = lr / bc1
    bp = p.abs() * (2.0 * u + u * lr * wd) + step * dr + 2.0 * u * (step * r).abs() + u * pr.abs() + 2.0 * TINY
    return bp * (1.0 + 1e-6), bm, bv


def exact_adamw_inputs(n, seed, zero_grad=False):
    """p on the 1/16 grid in [-4, 4]; non-zero integer gradients in [-2047, 2047] (their squares fit fp32), or all zero."""
    g = torch.Generator().manual_seed(11000 + seed)
    p = torch.randint(-64, 65, (n,), generator=g).float() / 16.0
    if zero_grad:
        return p, torch.zeros(n)
    gr = torch.randint(1, 2048, (n,), generator=g).float() * (torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0)
    return p, gr


def exact_adamw_expected(p, gr):
    """Closed form of the first EXACT_HP step, in float64: m = g / 2, v = g^2 / 4, p' = p (1 - 2^-13) - 2^-10 sign(g) (pure decay for g = 0)."""
    p, gr = p.double(), gr.double()
    return p * (1.0 - 2.0 ** -13) - 2.0 ** -10 * torch.sign(gr), gr / 2.0, gr * gr / 4.0


def rounded_adamw_grad(n, seed):
    """Seeded normal gradients holding zeros, 1e-30 (its square underflows), 1e-20 (v becomes a subnormal) and 1e18 (v near 1e33: finite)."""
    g = torch.Generator().manual_seed(12000 + seed)
    gr = torch.randn(n, generator=g)
    k = torch.arange(n)
    gr[k % 11 == 3] = 0.0
    gr[k % 97 == 5] = 1e-30
    gr[k % 97 == 6] = -1e-20
    gr[k % 97 == 7] = 1e18
    return gr


SEGMENT_LENGTHS = [1, 2, 255, 256, 257, 4095, 4096, 4097, 12289]


def ragged_segments(lengths, first=3, gaps=(1, 2, 3, 5, 7)):
    """[(begin, end)] with begins that are no multiples of 4 wherever the gap pattern allows, and a gap before every segment."""
    out, at = [], first
    for i, ln in enumerate(lengths):
        if at % 4 == 0:
            at += 1
        out.append((at, at + ln))
        at += ln + gaps[i % len(gaps)]
    return out, at + 4
