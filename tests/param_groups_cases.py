"""Cases and float64 references for param groups and global-norm clipping of the fused AdamW (vk_adamw_step_groups,
vk_grad_norm_segments, FusedAdamW with a list of param-group dicts, clip_grad_norm_).  No GPU needed: tests/test_param_groups_cpu.py checks
this module and the host side, tests/test_param_groups_gpu.py runs the kernels on its cases.  AdamW arithmetic, its exact tier and its
rounding bounds are those of tests/tail_cases.py.

Norm, EXACT tier.  The kernels square and add in double.  With integer gradients |g| <= 2047 and n <= 2^25 every partial sum of squares is
an integer below 2^22 * 2^25 = 2^47 < 2^53: exact in double in ANY order, so sqrt(S) is the correctly rounded root of the true sum and the
fp32 result can differ from the float64 reference by the last rounding only; a perfect square gives the integer root itself.  The max norm
is a selection: always exact.

Norm, ROUNDED tier.  A sum of n non-negative doubles in any order is off by at most (n - 1) 2^-53 relative (each addition rounds once, every
term is positive): 2^-28 for n <= 2^25, on the device and in the reference alike.  The root halves it and the product with |inv_scale| adds
2^-53.  An fp32 ulp of x is at least 2^-24 x, so both sums together stay below 2^-4 ulp; the rounding to fp32 adds half an ulp: the bound of
the tests is ONE ulp of the reference.  (Two float64 summation orders of a 24.4 M-element normal vector differed by 1.8e-16 relative and
rounded to the same fp32.)"""
import math

import torch

from tail_cases import (ADAMW_SIZES, DEFAULT_HP, EXACT_HP, SEGMENT_LENGTHS, adamw_bounds, adamw_ref, exact_adamw_expected,  # noqa: F401
                        exact_adamw_inputs, f32, ragged_segments, rounded_adamw_grad)

MAX_GROUPS = 8                       # VK_ADAMW_MAX_GROUPS
CHUNK = 4096                         # VK_ADAMW_SEGMENT_CHUNK
LARGE = 2 ** 20 + 3                  # 257 chunks: crosses the 256-thread stride of the norm's finalize
NORM_L2, NORM_INF = 0, 1
SENTINEL = 77.0

# eight hyper-parameter sets that differ in every field; among them the default, lr = 0, weight_decay = 0 and tail_cases' exact setting
HP_SETS = [
    DEFAULT_HP,
    dict(lr=0.0, beta1=0.8, beta2=0.99, eps=1e-6, wd=1e-2),
    dict(lr=1e-3, beta1=0.85, beta2=0.995, eps=1e-7, wd=0.0),
    dict(lr=3e-4, beta1=0.95, beta2=0.9999, eps=1e-5, wd=5e-2),
    dict(lr=1e-5, beta1=0.0, beta2=0.9, eps=1e-3, wd=1e-3),
    dict(lr=2e-2, beta1=0.7, beta2=0.98, eps=1e-4, wd=2e-4),
    EXACT_HP,
    dict(lr=7e-4, beta1=0.99, beta2=0.95, eps=1e-9, wd=3e-3),
]
GROUP_COUNTS = [2, 3, 8]


def layout():
    """[(begin, end)] of tail_cases' ragged segments plus one of LARGE elements (begins that are no multiples of 4, a gap before each),
    and the length of the buffer that holds them."""
    return ragged_segments(SEGMENT_LENGTHS + [LARGE])


def group_index(i, G):
    """Segment i belongs to group i % G: neighbours differ."""
    return i % G


def fused_factor(inv_scale, grad_scale=None, clip=None):
    """The gradient factor of vk_adamw_step_groups as the fp32 value the kernel forms (returned as a Python float): operands are the
    fp32 values the C ABI receives, the arithmetic is double, the result is rounded once — except without a clip coefficient and
    without grad_scale, where it is inv_scale itself."""
    a = f32(inv_scale)
    if grad_scale is not None:
        a = a / f32(grad_scale)
    if clip is not None:
        a = a * f32(clip)
    return f32(a)


def ulp32(x):
    """Spacing of fp32 at |x| (a float64 value)."""
    x = abs(float(x))
    if x == 0.0 or x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.frexp(x)[1] - 1 - 23)


def int_sum_squares(g):
    """Sum of squares of an integer-valued tensor in Python integers."""
    return sum(int(v) * int(v) for v in g.to(torch.int64).tolist())


def norm_ref(parts, kind, inv_scale=1.0):
    """float64 total norm of inv_scale * (the concatenation of `parts`), as vk_grad_norm_segments defines it: the root of the sum of
    squares, or the largest |g| with a NaN kept (torch.linalg.vector_norm), times |inv_scale|."""
    g = torch.cat([p.reshape(-1).double() for p in parts])
    if kind == NORM_L2:
        n = math.sqrt(float((g * g).sum()))
    else:
        n = float("nan") if bool(torch.isnan(g).any()) else float(g.abs().max())
    return n * abs(f32(inv_scale))


def coef_ref(total, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient in float64: max_norm / (total + 1e-6), clamped to at most 1, a NaN kept."""
    c = f32(max_norm) / (total + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def lattice_grad(n, seed):
    """Non-zero integer gradients in [-2047, 2047] (tail_cases.exact_adamw_inputs)."""
    return exact_adamw_inputs(n, seed)[1]


def threes(n, seed):
    """All +-3: the sum of squares is 9 n, a perfect square for n a square."""
    g = torch.Generator().manual_seed(13000 + seed)
    return (torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0) * 3.0


THREES_LENGTHS = [1, 4, 256, 4096, 2 ** 20]        # roots 3, 6, 48, 192, 3072


# ---------------------------------------------------------------------------------------------- model-level helpers
def ref_copies(m):
    return [p.detach().clone().requires_grad_(True) for p in m.parameters()]


def feed(ref, m, inv_scale=1.0):
    for r, p in zip(ref, m.parameters()):
        r.grad = None if p.grad is None else p.grad.detach().float() * inv_scale


def resync(ref, m):
    """Each step is compared from the same parameters: the bar is one step's rounding."""
    with torch.no_grad():
        for r, p in zip(ref, m.parameters()):
            r.copy_(p)


def three_groups(vk, m, lr, weight_decay=1e-4, encoder_lr_scale=0.2):
    """Index lists of three groups over m.parameters() and their settings, from vk.finetune_groups: the encoder's decayed tensors at
    encoder_lr_scale * lr, the decayed tensors of decoder and head at lr, and every 1-D tensor (both no-decay groups merged) at lr with
    weight_decay 0."""
    fg = vk.finetune_groups(m, lr, encoder_lr_scale=encoder_lr_scale, weight_decay=weight_decay, decay_norm_and_bias=False)
    index = {id(p): i for i, p in enumerate(m.parameters())}
    enc, rest, nodecay = [], [], []
    for g in fg:
        ids = [index[id(p)] for p in g["params"]]
        if g["weight_decay"] == 0.0:
            nodecay += ids
        elif g["lr"] == lr * encoder_lr_scale:
            enc += ids
        else:
            rest += ids
    return [(enc, dict(lr=lr * encoder_lr_scale, weight_decay=weight_decay)), (rest, dict(lr=lr, weight_decay=weight_decay)),
            (sorted(nodecay), dict(lr=lr, weight_decay=0.0))]


def as_param_groups(spec, params):
    params = list(params)
    return [dict(params=[params[i] for i in ids], **kw) for ids, kw in spec]
