"""Cases, exact tiers and rounding bounds for vk.averaging (vk_avg_update, vk_avg_swap, vk_adamw_step_amp_avg, ModelEMA / SWA).  No GPU
needed: tests/test_averaging_cpu.py proves the claims made here, tests/test_vk_averaging_gpu.py runs the kernels on these cases.
The bit-level restatement of the rule is tests/averaging_ref.py.

EXACT tier (the style of tail_cases.EXACT_HP: no operation rounds, so float64 evaluation of a + w (p - a) is the truth).
  EMA: p and a integer multiples of 2^-8 with magnitude below 8, decay = 0.75 (w = 2^-2), a fresh lattice p per update.  After update k the
  average is a multiple of 2^-(8 + 2k) below 8: 3 + 8 + 2k <= 21 bits for k <= 5; the difference p - a is a multiple of 2^-(6 + 2k) below
  16: 4 + 6 + 2k <= 20 bits.  Five consecutive updates stay inside fp32's 24 bits.
  SWA: w = 1 / t is a power of two for t = 1, 2, 4, 8, i.e. counters preset to 0, 1, 3, 7; one update of lattice values is then exact
  (a multiple of 2^-11 below 8).

ROUNDED tier, against torch.  u = 2^-24, d = p - a, r = a + w (p - a) in float64 with this rule's fp32 weight w.
  this rule      d rounded (u |d|, scaled by w), the fused multiply-add rounded once:             w u |d| + u |r|
  torch.lerp(a, p, wt), wt = fp32(1 - decay) of the Python double decay:
      wt < 0.5   a + wt (p - a): difference, product, sum                                        2 wt u |d| + u |r|
      wt >= 0.5  p - (p - a)(1 - wt): 1 - wt, difference, product, sum                           3 (1 - wt) u |d| + u |r|
  torch's SWA    a + (p - a) / t: difference, quotient (correctly rounded), sum                  2 u |d| / t + u |r|
  the weights    this rule rounds decay to fp32 first (u decay), then 1 - decay once (u w); torch rounds 1 - decay once (u wt); SWA's
                 1 / t is rounded once here (u / t) and never formed by torch:                   |w - wt| <= u (decay + w + wt)
  The sum of a line of this rule, a line of torch's, |w - wt| |d| and 4 TINY (each operation may underflow) bounds the difference of
  ONE update from equal averages.  Over several updates the averages themselves differ by E: the next difference is at most
  (1 - w) E plus the one-update bound taken with |d| + E and |r| + E (step_bound below, accumulated by ema_bound_steps)."""
import math

import numpy as np
import torch

import averaging_ref as R

U32 = 2.0 ** -24
TINY = 2.0 ** -149
SENTINEL = 77.0

SIZES = [1, 2, 3, 255, 257, 4097, 2 ** 20 + 3]
# k_avg_ranges runs 2,048 workgroups x 256 threads x one 16-byte vector at most: 2^21 elements per grid stride.  This size is past it.
PAST_VECTOR_STRIDE = 2 ** 21 + 261
FUSED_SIZES = [3, 257, 2 ** 20 + 3]

EXACT_DECAY = 0.75
EXACT_UPDATES = 5
SWA_PRESETS = [0, 1, 3, 7]


def lattice(n, seed):
    """fp32 integer multiples of 2^-8 with magnitude below 8."""
    g = torch.Generator().manual_seed(31000 + seed)
    return torch.randint(-2047, 2048, (n,), generator=g).float() / 256.0


def rounded_pair(n, seed, special=True):
    """(a, p) fp32: seeded normal data; p holds exact zeros, elements equal to a, and (special) +inf, -inf and one NaN; a holds exact zeros
    and stays finite, so no operation creates a NaN of its own (the sign of a created NaN differs between processors)."""
    g = torch.Generator().manual_seed(32000 + seed)
    a = torch.randn(n, generator=g)
    p = a + 0.1 * torch.randn(n, generator=g)
    k = torch.arange(n)
    p[k % 11 == 3] = 0.0
    a[k % 13 == 4] = 0.0
    p[k % 17 == 9] = a[k % 17 == 9]
    p[k % 19 == 8] = 1e-30 * (1.0 + (k[k % 19 == 8] % 7).float())       # differences near the bottom of the normal range
    a[k % 19 == 8] = 3e-38
    if special:
        p[k % 97 == 5] = math.inf
        p[k % 97 == 6] = -math.inf
        if n > 7:
            p[7] = math.nan
    return a, p


def bits(t):
    """The bit patterns of an fp32 tensor or array, as a numpy int32 array."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ weights, hand-computed
# decay = 0.999 is 0.99900001287460327 in fp32.  With warmup, update t uses min(decay, (1 + t) / (10 + t)):
#   t = 1: 2/11, w = 9/11;  t = 2: 3/12, w = 3/4;  t = 10: 11/20, w = 9/20;  t = 1000: 1001/1010, w = 9/1010.
# (1 + t) / (10 + t) > decay  <=>  t > (10 decay - 1) / (1 - decay) = 8990.116 for the fp32 decay: t = 8990 still takes the ramp (8991 / 9000
# = 0.999 exactly in the rationals, below the fp32 decay), t = 8991 is the first that takes decay itself, w = 1 - 0.99900001287460327
# = 0.00099998712539673 (exact in double, 2^-24 * 16777 in fp32).
WARMUP_DECAY = 0.999
WARMUP_WEIGHTS = {            # t -> (the rational w before its rounding to fp32, as numerator / denominator), or None: w = 1 - fp32(decay)
    1: (9, 11),
    2: (3, 4),
    10: (9, 20),
    1000: (9, 1010),
    8990: (9, 9000),
    8991: None,
    100000: None,
}
WARMUP_FIRST_FULL_DECAY = 8991
SWA_WEIGHTS = {1: (1, 1), 2: (1, 2), 3: (1, 3)}


# ------------------------------------------------------------------------------------------------ float64 references and bounds
def ema_ref64(a, p, w):
    """a + w (p - a) in float64 (a, p: float64 or fp32 tensors; w: the fp32 weight as a Python float)."""
    a, p = a.double(), p.double()
    return a + w * (p - a)


def step_bound(a64, p, w, wt, torch_form, t=1, E=None):
    """Elementwise bound of |this rule - torch's form| after one update whose incoming averages differ by at most E (a tensor or None)
    around the float64 average a64; see the module docstring.  torch_form: "lerp" or "swa".  Returns (bound, bound of this rule alone,
    bound of torch's form alone), the last two from equal averages."""
    a64, p = a64.double(), p.double()
    E = torch.zeros_like(a64) if E is None else E
    d = (p - a64).abs() + E
    r = ema_ref64(a64, p, w).abs() + E
    ours = w * U32 * d + U32 * r + 2.0 * TINY
    if torch_form == "lerp":
        theirs = (2.0 * wt * U32 * d if wt < 0.5 else 3.0 * (1.0 - wt) * U32 * d) + U32 * r + 2.0 * TINY
    else:
        theirs = 2.0 * U32 * d / t + U32 * r + 2.0 * TINY
    dw = abs(w - wt) * d
    return ((1.0 - w) * E + ours + theirs + dw) * (1.0 + 1e-6), ours * (1.0 + 1e-6), (theirs + dw) * (1.0 + 1e-6)


def ema_bound_steps(a0, ps, decay):
    """float64 trajectory and accumulated bound of ModelEMA(decay, warmup=False) against torch.lerp(a, p, 1 - decay) over the updates
    ps (a list of fp32 tensors) from the fp32 start a0.  Returns (a64 after the last update, bound)."""
    w = float(R.avg_weight(R.EMA, decay, False, 1))
    wt = float(np.float32(1.0 - decay))
    a64, E = a0.double(), None
    for p in ps:
        E = step_bound(a64, p, w, wt, "lerp", E=E)[0]
        a64 = ema_ref64(a64, p, w)
    return a64, E


def weight_slack(decay):
    """The derived bound on |w - wt| for ModelEMA without warmup: u (decay + w + wt)."""
    w = float(R.avg_weight(R.EMA, decay, False, 1))
    wt = float(np.float32(1.0 - decay))
    return U32 * (decay + w + wt), abs(w - wt)
