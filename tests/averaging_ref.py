"""numpy restatement of the averaging rule of csrc/optim.hip (avg_elem, avg_prepare), bit for bit.  No GPU.

    w == 1      : a' = p
    otherwise   : d  = p - a            one fp32 rounding
                  a' = fma(d, w, a)     one rounding

The fused multiply-add has to round ONCE.  float64 ``d * w + a`` followed by a cast rounds twice (to 53 bits, then to 24) and is wrong on
ties.  Two forms are given and tests/test_averaging_cpu.py holds the first to the second:
  fma32          vectorised: d * w is exact in float64 (24 + 24 bits), the sum with a is formed with an error-free TwoSum and rounded to
                 ODD (a sticky last bit), after which the cast to fp32 is the single correct rounding (53 >= 24 + 2).
  fma32_exact    one triple in Python integers: the exact sum as an integer over a power of two, rounded to nearest-even at 24 bits
                 (or at the fp32 subnormal spacing 2^-149).
The weight: avg_weight / avg_prepare, the double arithmetic of the device written in Python floats (which are doubles)."""
import math

import numpy as np

EMA, SWA = 0, 1                     # VK_AVG_EMA, VK_AVG_SWA


def f32(v):
    """A Python float as the fp32 value the C ABI receives (returned as a Python float)."""
    return float(np.float32(v))


def avg_weight(kind, decay, warmup, t):
    """w of update t (1-based) as np.float32: formed in double from the fp32 decay, rounded once."""
    if kind == SWA:
        return np.float32(1.0 / float(t))
    d = f32(decay)
    if warmup:
        d = min(d, (1.0 + float(t)) / (10.0 + float(t)))
    return np.float32(1.0 - d)


def avg_prepare(kind, decay, warmup, count, found_inf=None):
    """(count', w): a found_inf that is not None and != 0 (1, -1 and NaN alike) skips: (count, None)."""
    if found_inf is not None and found_inf != 0.0:
        return count, None
    t = count + 1
    return t, avg_weight(kind, decay, warmup, t)


def fma32(d, w, a):
    """Correctly rounded fp32 fma(d, w, a) of fp32 arrays (w: array or scalar), through float64 with round-to-odd."""
    d, a = np.asarray(d, dtype=np.float32), np.asarray(a, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(all="ignore"):
        x = d.astype(np.float64) * w.astype(np.float64)          # exact: 48 significant bits at most
        y = a.astype(np.float64)
        s = x + y
        bb = s - x                                               # TwoSum (Knuth): s + e == x + y exactly
        e = (x - (s - bb)) + (y - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)            # the odd one of the two doubles around the exact sum
        return s.astype(np.float32)


def _ratio(x):
    n, den = float(x).as_integer_ratio()
    return n, den.bit_length() - 1                               # x == n / 2^k


def fma32_exact(d, w, a):
    """fma(d, w, a) of three finite fp32 values in integer arithmetic, rounded once to fp32 (nearest, ties to even)."""
    d, w, a = float(np.float32(d)), float(np.float32(w)), float(np.float32(a))
    nd, kd = _ratio(d)
    nw, kw = _ratio(w)
    na, ka = _ratio(a)
    k = max(kd + kw, ka)
    N = nd * nw * (1 << (k - kd - kw)) + na * (1 << (k - ka))    # the exact value is N / 2^k
    if N == 0:
        prod_negative = (math.copysign(1.0, d) * math.copysign(1.0, w)) < 0
        both_negative = prod_negative and math.copysign(1.0, a) < 0
        exact_cancel = (nd * nw != 0)                            # x + (-x) is +0 in round-to-nearest
        return np.float32(-0.0 if (both_negative and not exact_cancel) else 0.0)
    sign, N = (-1.0, -N) if N < 0 else (1.0, N)
    e = max(N.bit_length() - k - 24, -149)                       # quantum 2^e: 24 significant bits, or the subnormal spacing
    shift = k + e
    if shift <= 0:
        q = N << (-shift)
    else:
        q, rem, half = N >> shift, N & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
    v = math.ldexp(float(q), e)                                  # q <= 2^24: exact
    return np.float32(sign * (v if v < 2.0 ** 128 else math.inf))


def avg_elem(a, p, w):
    """a' of fp32 arrays a, p and the fp32 weight w."""
    a, p = np.asarray(a, dtype=np.float32), np.asarray(p, dtype=np.float32)
    w = np.float32(w)
    if w == np.float32(1.0):
        return p.copy()
    with np.errstate(all="ignore"):
        d = p - a                                                # fp32 arrays: one IEEE rounding
    return fma32(d, w, a)


def avg_update(a, p, kind, decay, warmup, count, found_inf=None):
    """(a', count') of one vk_avg_update."""
    count2, w = avg_prepare(kind, decay, warmup, count, found_inf)
    if w is None:
        return np.asarray(a, dtype=np.float32).copy(), count
    return avg_elem(a, p, w), count2
