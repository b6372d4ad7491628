"""vk.averaging, the parts that need no GPU: the numpy restatement of the rule (tests/averaging_ref.py) and its correctly rounded fused
multiply-add, the exactness of the lattice cases and the bounds against torch (tests/averaging_cases.py), the weight rule against
hand-computed values, the argument checks of vk_avg_update / vk_avg_swap / vk_adamw_step_amp_avg, and the host side of ModelEMA / SWA."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import averaging_cases as AC
import averaging_ref as R


# ------------------------------------------------------------------------------------------------ the fused multiply-add
def test_fast_fma_equals_the_exact_one_on_seeded_triples():
    rng = np.random.default_rng(20240)
    n = 100_000
    d = rng.standard_normal(n).astype(np.float32)
    a = rng.standard_normal(n).astype(np.float32)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    # a spread of magnitudes: products far below the addend, far above it, cancelling sums, subnormal results
    scale = np.float32(2.0) ** rng.integers(-40, 41, n).astype(np.float32)
    d = (d * scale).astype(np.float32)
    a[: n // 10] = (-d[: n // 10] * w[: n // 10]).astype(np.float32)            # near-total cancellation
    d[n // 10: n // 5] *= np.float32(2.0 ** -100)
    a[n // 10: n // 5] *= np.float32(2.0 ** -126)                               # subnormal sums
    fast = R.fma32(d, w, a)
    exact = np.array([R.fma32_exact(x, y, z) for x, y, z in zip(d.tolist(), w.tolist(), a.tolist())], dtype=np.float32)
    assert np.array_equal(AC.bits(fast), AC.bits(exact))
    twice = (d.astype(np.float64) * w.astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    assert np.count_nonzero(AC.bits(twice) != AC.bits(exact)) < n // 1000     # the double rounding is right almost everywhere ...


def test_fast_fma_on_built_midpoints():
    """... and wrong exactly here: the exact sum is an fp32 midpoint plus or minus something below float64's resolution of it, so float64
    lands on the midpoint and its cast rounds to even, while one rounding goes to the side of the small term."""
    a = np.float32(1.0 + 2.0 ** -23)                       # odd last bit: ties-to-even moves it
    cases = [(np.float32(2.0 ** -12), np.float32(2.0 ** -12), a)]              # a + 2^-24: the midpoint itself, a true tie
    for k, sign in [(30, 1.0), (30, -1.0), (35, 1.0), (35, -1.0)]:              # the midpoint + sign 2^-k, through the product
        cases.append((np.float32(2.0 ** -12), np.float32(2.0 ** -12 + sign * 2.0 ** (12 - k)), a))
    # an addend far below the product: the product is a midpoint of the RESULT's spacing, the addend decides the side
    for k, sign in [(40, 1.0), (60, -1.0), (100, 1.0), (140, -1.0)]:
        d, w = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)     # d w = 1 + 2^-11 + 2^-24: a midpoint above 1 + 2^-11
        cases.append((d, w, np.float32(sign * 2.0 ** -k)))
    for d, w, a in cases:
        got = R.fma32(np.array([d]), w, np.array([a]))[0]
        want = R.fma32_exact(d, w, a)
        assert AC.bits(np.array([got]))[0] == AC.bits(np.array([want]))[0], (d, w, a)
        exact = Fraction(float(d)) * Fraction(float(w)) + Fraction(float(a))
        assert abs(Fraction(float(want)) - exact) <= Fraction(R.f32(np.spacing(np.float32(abs(float(want)))))) / 2
    # the second family really separates one rounding from two
    d = w = np.float32(1.0 + 2.0 ** -12)
    up = R.fma32_exact(d, w, np.float32(2.0 ** -60))
    down = R.fma32_exact(d, w, np.float32(-2.0 ** -60))
    assert float(up) == 1.0 + 2.0 ** -11 + 2.0 ** -23 and float(down) == 1.0 + 2.0 ** -11
    twice = np.float32(np.float64(d) * np.float64(w) + np.float64(2.0 ** -60))
    assert float(twice) == 1.0 + 2.0 ** -11                      # float64 drops the addend and the tie goes to even: the wrong side
    assert float(R.fma32(np.array([d]), w, np.array([np.float32(2.0 ** -60)]))[0]) == float(up)


def test_exact_fma_special_results():
    assert AC.bits(np.array([R.fma32_exact(1.0, 1.0, -1.0)]))[0] == 0                        # x + (-x) = +0
    assert AC.bits(np.array([R.fma32_exact(-0.0, 1.0, -0.0)]))[0] == np.int32(-2 ** 31)       # (-0) + (-0) = -0
    assert AC.bits(np.array([R.fma32_exact(0.0, 1.0, -0.0)]))[0] == 0
    assert math.isinf(float(R.fma32_exact(3e38, 2.0, 3e38)))
    assert float(R.fma32_exact(2.0 ** -100, 2.0 ** -49, 0.0)) == 2.0 ** -149
    assert float(R.fma32_exact(2.0 ** -100, 2.0 ** -50, 0.0)) == 0.0                         # half the smallest subnormal: ties to even
    assert float(R.fma32_exact(3 * 2.0 ** -100, 2.0 ** -50, 0.0)) == 2.0 ** -148             # 1.5 spacings: up to the even 2


def test_restatement_of_the_rule():
    a, p = AC.rounded_pair(4097, 1)
    a, p = a.numpy(), p.numpy()
    assert np.array_equal(AC.bits(R.avg_elem(a, p, 1.0)), AC.bits(p))                         # w == 1: a copy, bit for bit
    out = R.avg_elem(a, p, np.float32(0.25))
    assert np.isposinf(out[5]) and np.isneginf(out[6]) and np.isnan(out[7]) and AC.bits(out)[7] == AC.bits(p)[7]
    same = np.nonzero(p == a)[0]
    assert same.size and np.array_equal(AC.bits(out[same]), AC.bits(a[same]))                 # d = 0: the average stays
    # skip rule of the restatement
    for fi in (1.0, -1.0, math.nan):
        got, cnt = R.avg_update(a, p, R.EMA, 0.9, False, 4, fi)
        assert cnt == 4 and np.array_equal(AC.bits(got), AC.bits(a))
    for fi in (None, 0.0, -0.0):
        got, cnt = R.avg_update(a, p, R.EMA, 0.75, False, 4, fi)
        assert cnt == 5 and np.array_equal(AC.bits(got), AC.bits(out))


# ------------------------------------------------------------------------------------------------ the weight
def _f32_of(fr):
    return np.float32(float(Fraction(*fr)))


def test_weight_rule_against_hand_computed_values():
    d32 = R.f32(AC.WARMUP_DECAY)
    assert d32 == 0.99900001287460327148 and Fraction(d32) == Fraction(16760439, 2 ** 24)
    full = np.float32(1.0 - d32)
    assert float(full) == 16777 * 2.0 ** -24                                                   # 1 - decay is exact here
    for t, fr in AC.WARMUP_WEIGHTS.items():
        w = R.avg_weight(R.EMA, AC.WARMUP_DECAY, True, t)
        assert w.dtype == np.float32
        assert w == (full if fr is None else _f32_of(fr)), t
        assert R.avg_weight(R.EMA, AC.WARMUP_DECAY, False, t) == full                          # without warmup: decay at every t
    # the first update that takes decay itself
    ramp = lambda t: Fraction(1 + t, 10 + t)
    first = next(t for t in range(1, 20000) if ramp(t) > Fraction(d32))
    assert first == AC.WARMUP_FIRST_FULL_DECAY and ramp(first - 1) == Fraction(999, 1000) < Fraction(d32)
    for t, fr in AC.SWA_WEIGHTS.items():
        assert R.avg_weight(R.SWA, 0.0, False, t) == _f32_of(fr)
    assert R.avg_weight(R.SWA, 0.0, False, 1) == np.float32(1.0)
    assert R.avg_weight(R.EMA, 0.0, False, 7) == np.float32(1.0)                               # decay 0: a copy
    assert float(R.avg_weight(R.EMA, AC.EXACT_DECAY, False, 3)) == 0.25
    # the skip rule: a flag that is not zero leaves the counter and yields no weight
    for fi in (1.0, -1.0, math.nan, math.inf, 1e-45):
        assert R.avg_prepare(R.EMA, 0.9, True, 6, fi) == (6, None)
    for fi in (None, 0.0, -0.0):
        cnt, w = R.avg_prepare(R.EMA, 0.9, True, 6, fi)
        assert cnt == 7 and w == np.float32(1.0 - 8.0 / 17.0)


# ------------------------------------------------------------------------------------------------ exact tier
def test_lattice_updates_are_exact_in_fp32():
    n = 4097
    a = AC.lattice(n, 0)
    assert bool((a * 256 == (a * 256).round()).all()) and a.abs().max().item() < 8
    a64, a32 = a.double(), a.numpy().copy()
    w = float(R.avg_weight(R.EMA, AC.EXACT_DECAY, False, 1))
    assert w == 0.25
    count = 0
    for k in range(1, AC.EXACT_UPDATES + 1):
        p = AC.lattice(n, k)
        d = p.double() - a64
        assert torch.equal(d.float().double(), d)                                  # the difference does not round
        a64 = a64 + w * d
        assert torch.equal(a64.float().double(), a64)                              # nor does the result
        assert bool(((a64 * 2.0 ** (8 + 2 * k)) == (a64 * 2.0 ** (8 + 2 * k)).round()).all()) and a64.abs().max().item() < 8
        a32, count = R.avg_update(a32, p.numpy(), R.EMA, AC.EXACT_DECAY, False, count)
        assert np.array_equal(a32.astype(np.float64), a64.numpy())                 # the restatement reproduces the truth
    assert count == AC.EXACT_UPDATES
    # a sixth update may round: the tier stops where its proof does
    assert 3 + 8 + 2 * AC.EXACT_UPDATES <= 24 < 3 + 8 + 2 * (AC.EXACT_UPDATES + 4)


def test_swa_is_exact_at_powers_of_two():
    n = 4097
    a, p = AC.lattice(n, 10), AC.lattice(n, 11)
    for preset in AC.SWA_PRESETS:
        t = preset + 1
        assert t & (t - 1) == 0
        w = R.avg_weight(R.SWA, 0.0, False, t)
        assert float(w) == 1.0 / t
        want = a.double() + (p.double() - a.double()) / t
        assert torch.equal(want.float().double(), want)
        got, cnt = R.avg_update(a.numpy(), p.numpy(), R.SWA, 0.0, False, preset)
        assert cnt == t and np.array_equal(got.astype(np.float64), want.numpy())
    got, _ = R.avg_update(a.numpy(), p.numpy(), R.SWA, 0.0, False, 0)
    assert np.array_equal(AC.bits(got), AC.bits(p))                                # the first sample replaces the starting copy


# ------------------------------------------------------------------------------------------------ bounds against torch
@pytest.mark.parametrize("decay", [0.999, 0.9, 0.75, 0.3, 0.0])
def test_float64_lies_within_the_bound_against_torch_lerp(decay):
    slack, gap = AC.weight_slack(decay)
    assert gap <= slack
    w = float(R.avg_weight(R.EMA, decay, False, 1))
    wt = float(np.float32(1.0 - decay))
    for n, seed in [(257, 2), (4097, 3), (2 ** 20 + 3, 4)]:
        a, p = AC.rounded_pair(n, seed, special=False)
        r = AC.ema_ref64(a, p, w)
        bound, ours_b, theirs_b = AC.step_bound(a, p, w, wt, "lerp")
        ours = torch.from_numpy(R.avg_elem(a.numpy(), p.numpy(), np.float32(w))).double()
        theirs = torch.lerp(a, p, 1.0 - decay).double()
        assert bool(((ours - r).abs() <= ours_b).all())
        assert bool(((theirs - r).abs() <= theirs_b).all())
        assert bool(((ours - theirs).abs() <= bound).all())


def test_float64_lies_within_the_bound_against_torch_swa():
    for t in (1, 2, 3, 7, 100):
        w = float(R.avg_weight(R.SWA, 0.0, False, t))
        assert abs(w - 1.0 / t) <= AC.U32 / t
        a, p = AC.rounded_pair(4097, 20 + t, special=False)
        r = AC.ema_ref64(a, p, w)
        bound, ours_b, theirs_b = AC.step_bound(a, p, w, 1.0 / t, "swa", t=t)
        ours = torch.from_numpy(R.avg_elem(a.numpy(), p.numpy(), np.float32(w))).double()
        theirs = (a + (p - a) / t).double()                                        # torch.optim.swa_utils.get_swa_avg_fn
        assert bool(((ours - r).abs() <= ours_b).all())
        assert bool(((theirs - r).abs() <= theirs_b).all())
        assert bool(((ours - theirs).abs() <= bound).all())


def test_accumulated_bound_covers_three_updates():
    decay = 0.9
    a0, _ = AC.rounded_pair(4097, 40, special=False)
    ps = [AC.rounded_pair(4097, 41 + k, special=False)[1] for k in range(3)]
    a64, bound = AC.ema_bound_steps(a0, ps, decay)
    ours, theirs, cnt = a0.numpy(), a0.clone(), 0
    for p in ps:
        ours, cnt = R.avg_update(ours, p.numpy(), R.EMA, decay, False, cnt)
        theirs = torch.lerp(theirs, p, 1.0 - decay)
    assert cnt == 3
    diff = (torch.from_numpy(ours).double() - theirs.double()).abs()
    assert bool((diff <= bound).all())
    assert bool(((torch.from_numpy(ours).double() - a64).abs() <= bound).all())
    assert bound.max().item() < 1e-5                                               # a bound that tests something: a few ulps of O(1) values


# ------------------------------------------------------------------------------------------------ the C ABI's argument checks
def test_c_entry_points_refuse_bad_arguments_before_any_launch(vk):
    L = vk.lib()
    buf = (C.c_double * 64)()               # any non-null address: a refused call touches neither it nor a device
    a = C.addressof(buf)
    Rg, Rule = vk._lib.vk_avg_range, vk._lib.vk_avg_rule
    good_rule = Rule(vk._lib.VK_AVG_EMA, 0.9, 0)
    one = (Rg * 1)(Rg(a, a + 64, 8))

    def update(n=1, ranges=one, rule=good_rule, count=a, scratch=a):
        return L.vk_avg_update(n, ranges, rule, count, None, scratch, None)

    for n in (0, -1, 5, 100):
        assert update(n) == -1 and b"ranges" in L.vk_last_error_string()
        assert L.vk_avg_swap(n, one, None) == -1 and b"ranges" in L.vk_last_error_string()
    assert update(1, None) == -1 and L.vk_avg_swap(1, None, None) == -1
    assert update(count=None) == -1 and update(scratch=None) == -1
    for bad in ((Rg * 1)(Rg(None, a, 8)), (Rg * 1)(Rg(a, None, 8)), (Rg * 1)(Rg(a + 2, a + 64, 8)), (Rg * 1)(Rg(a, a + 65, 8)),
                (Rg * 2)(Rg(a, a + 64, 8), Rg(None, a, 1))):
        assert update(len(bad), bad) == -1 and b"range" in L.vk_last_error_string()
        assert L.vk_avg_swap(len(bad), bad, None) == -1
    for decay in (1.0, 1.5, -0.1, -1e-30, math.nan, math.inf, -math.inf):
        assert update(rule=Rule(vk._lib.VK_AVG_EMA, decay, 0)) == -1 and b"decay" in L.vk_last_error_string(), decay
        assert update(rule=Rule(vk._lib.VK_AVG_SWA, decay, 0)) == -1
    for kind in (-1, 2, 7):
        assert update(rule=Rule(kind, 0.5, 0)) == -1 and b"kind" in L.vk_last_error_string()

    names = ("param", "grad", "m", "v", "steps", "scratch4", "avg", "avg_count", "avg_scratch")

    def fused(n=64, rule=good_rule, extra=(a, a, 4), **null):
        q = {k: a for k in names}
        q.update({k: None for k in null})
        return L.vk_adamw_step_amp_avg(n, q["param"], q["grad"], q["m"], q["v"], 1e-3, 0.9, 0.999, 1e-8, 0.0, q["steps"], 1.0, None, None,
                                       q["scratch4"], None, 0, q["avg"], q["avg_count"], rule, q["avg_scratch"], extra[0], extra[1],
                                       extra[2], None)

    assert fused(0) == -1
    for k in names:
        assert fused(**{k: True}) == -1, k
    assert fused(extra=(None, a, 4)) == -1 and fused(extra=(a, None, 4)) == -1
    for decay in (1.0, -0.5, math.nan):
        assert fused(rule=Rule(vk._lib.VK_AVG_EMA, decay, 1)) == -1 and b"decay" in L.vk_last_error_string()
    assert fused(rule=Rule(3, 0.5, 0)) == -1 and b"kind" in L.vk_last_error_string()


# ------------------------------------------------------------------------------------------------ the Python front end, host side
def test_front_end_without_a_device(vk):
    assert vk.averaging.ModelEMA is vk.ModelEMA and vk.averaging.SWA is vk.SWA
    m = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.ModelEMA(m, decay=0.999)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.SWA(m)
    for decay in (1.0, -0.1, math.nan, 2.0):
        with pytest.raises(ValueError):
            vk.ModelEMA(m, decay=decay)
    with pytest.raises(vk.VkError):
        vk.ModelEMA(torch.nn.Linear(2, 2))
    opt = vk.adamw_for(m, lr=1e-3)
    assert opt._average is None                     # an optimizer without an average: the step's own path
    assert vk._lib.VK_AVG_EMA == R.EMA and vk._lib.VK_AVG_SWA == R.SWA and vk._lib.VK_AVG_MAX_RANGES == 4
    assert C.sizeof(vk._lib.vk_avg_rule) == 12 and C.sizeof(vk._lib.vk_avg_range) == 24
