"""tests/tail_cases.py on the CPU: every exact-tier case of the head / dec4-tail / AdamW sweep meets the conditions under which a kernel
must EQUAL float64, and every float64 reference agrees with an independent twin (F.conv2d autograd, torch.optim.AdamW on float64
tensors, the oracle's DiceLoss plus torch's BCE).  Nothing here touches a kernel: the conditions are asserted on the references alone."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import tail_cases as TC
from conv_lattice import exact_in


@functools.lru_cache(maxsize=2)
def head(case):
    return TC.head_build(case)


HEAD = TC.all_head_cases()


@pytest.mark.parametrize("case", HEAD, ids=[c.name for c in HEAD])
def test_head_case_meets_exactness_conditions(case):
    fig = TC.head_check(head(case))
    print(case.name, fig)


@pytest.mark.parametrize("case", HEAD, ids=[c.name for c in HEAD])
def test_head_reference_equals_conv2d_autograd(case):
    b = head(case)
    logits, dy, dw, db = TC.head_twin(b)
    assert torch.equal(b.logits, logits) and torch.equal(b.dy, dy) and torch.equal(b.dw, dw) and torch.equal(b.db, db)
    if case.bnr:        # the mask is taken from the bnr tensor and coefficients, whatever src->relu says
        keep = (b.bz * b.bscale.view(1, -1, 1, 1) + b.bshift.view(1, -1, 1, 1)) > 0
        assert torch.equal(b.g, dy * keep) and torch.equal(b.sums[1], (dy * keep * b.bz).sum(dim=(0, 2, 3)))
        assert 0.05 < keep.double().mean().item() < 0.95


def test_head_case_list_covers_what_the_sweep_claims():
    cs = TC.head_cases() + TC.head_multi_cases()
    assert {c.H for c in cs} >= {1, 2, 15, 16, 17, 33} and {c.W for c in cs} >= {1, 2, 15, 16, 17, 33}
    assert all(c.H != c.W for c in cs) and {c.N for c in cs} == {1, 2, 3, 5}
    assert {(c.H, c.W) for c in cs} >= {(w, h) for c in cs for h, w in [(c.H, c.W)] if (w, h) != (33, 16) and (w, h) != (15, 17)}
    assert {c.C for c in TC.head_multi_cases()} == {1, 2, 3, 8, 16}
    for fam in (TC.head_cases(), TC.head_multi_cases()):
        assert {c.relu for c in fam} == {0, 1} and {c.affine for c in fam} == {True, False}
        assert {c.bnr for c in fam} >= {"", "own", "other"}
    large = TC.head_large_cases()
    assert any(c.C == 0 and c.tiles > 2048 and c.H % 16 for c in large) and any(c.C > 0 and c.tiles > 2048 for c in large)
    assert any(c.tiles > 1024 and c.H % 16 == 0 and c.W % 16 == 0 for c in large)
    names = [c.name for c in TC.all_head_cases()]
    assert len(names) == len(set(names))


def test_head_reference_is_sensitive_to_one_element():
    c = TC.head_cases()[4]
    b = TC.head_build(c)
    b2 = TC.head_build(c)
    assert torch.equal(b.logits, b2.logits)                  # deterministic
    a = b.a.clone()
    a[0, 1, 0, 0] += 1.0
    assert not torch.equal(F.conv2d(a, b.w, b.bias, padding=1), b.logits)


TAIL = TC.tail_cases()


@pytest.mark.parametrize("case", TAIL, ids=[c.name for c in TAIL])
def test_tail_case_is_exact_in_both_types_and_equals_conv2d(case):
    b = TC.tail_build(case)
    fig = TC.tail_check(b)
    print(case.name, fig)
    assert torch.equal(b.logits, TC.tail_twin(b))
    assert fig["a2"] > 0 and b.logits.abs().max().item() > 3.0        # the chain is alive: the logits are not the bias alone
    assert {(c.H, c.W) for c in TAIL} >= {(16, 48), (48, 16), (32, 80), (16, 16)} and {c.N for c in TAIL} == {1, 3}


# ------------------------------------------------------------------------------------------------ BCE + Dice
def oracle_loss(x, y, wb, wd):
    from oracle import unet_oracle as O
    xv = x.double().view(1, 1, -1).requires_grad_(True)
    yv = y.double().view(1, 1, -1)
    bce = F.binary_cross_entropy_with_logits(xv, yv)
    dice = O.DiceLoss()(xv, yv)
    (wb * bce + wd * dice).backward()
    return bce.item(), dice.item(), xv.grad.flatten()


@pytest.mark.parametrize("wb,wd", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("kind", ["hard", "soft"])
@pytest.mark.parametrize("count", [1, 5, 1025, 40003])
def test_loss_reference_equals_oracle_dice_plus_torch_bce(count, kind, wb, wd):
    x, y = TC.loss_inputs(count, kind, count)
    r = TC.loss_ref(x, y, wb, wd)
    bce, dice, grad = oracle_loss(x, y, wb, wd)
    assert r.bce == pytest.approx(bce, rel=1e-12, abs=1e-15) and r.dice == pytest.approx(dice, rel=1e-12, abs=1e-15)
    assert (r.grad - grad).abs().max().item() <= 1e-12 * max(grad.abs().max().item(), 1e-30) + 1e-300


def test_loss_reference_edges():
    n = 1000
    x, _ = TC.loss_inputs(n, "hard", 1)
    empty = TC.loss_ref(x, torch.zeros(n), 1.0, 1.0)
    assert empty.dice == 0.0 and empty.ky == 0.0 and empty.k0 == 0.0                 # Dice and its gradient vanish for an empty target
    b, d, gr = oracle_loss(x, torch.zeros(n), 0.0, 1.0)
    assert d == 0.0 and float(gr.abs().max()) == 0.0
    clamp = TC.loss_ref(torch.full((n,), -100.0), torch.zeros(n), 1.0, 1.0)
    assert clamp.clamped and clamp.dice == 0.0 and math.isfinite(clamp.total) and bool(torch.isfinite(clamp.grad).all())
    ones = TC.loss_ref(x, torch.ones(n), 1.0, 1.0)
    assert 0.0 < ones.dice < 1.0
    for big in (20.0, 88.0, 100.0):
        xb = torch.tensor([big, -big, big, -big])
        r = TC.loss_ref(xb, torch.tensor([1.0, 1.0, 0.0, 0.0]), 1.0, 1.0)
        assert bool(torch.isfinite(r.grad).all()) and r.bce == pytest.approx(big / 2.0, rel=1e-6)
    # x = 0: p = 1/2 exactly, so the three Dice sums are T/2, count/2 and T and the gradient has a closed form
    y = (torch.arange(n) % 3 == 0).float()
    z = TC.loss_ref(torch.zeros(n), y, 1.0, 1.0)
    T = float(y.sum())
    assert z.sums[1:] == [T / 2.0, n / 2.0, T]
    assert torch.equal(z.grad, (0.5 - y.double()) * z.invc + (z.ky * y.double() + z.k0) * 0.25)


def test_loss_bounds_are_small_and_positive():
    for count, vec in [(1, True), (5, True), (1025, False), (2 ** 21 + 5, True), (TC.LOSS_SCALAR_LARGE, False)]:
        assert TC.loss_terms_per_thread(count, vec) >= 1
    assert TC.loss_terms_per_thread(2 ** 21 + 5, True) == 9 and TC.loss_terms_per_thread(TC.LOSS_SCALAR_LARGE, False) == 2
    assert TC.loss_terms_per_thread(1025, True) == 5 and TC.loss_terms_per_thread(3, True) == 1
    x, y = TC.loss_inputs(4099, "soft", 3)
    r = TC.loss_ref(x, y, 1.0, 1.0)
    bd = TC.loss_bounds(r, True, 1.0, 1.0, True)
    assert 0.0 < bd.total < 1e-5 * abs(r.total) and 0.0 < bd.dice < 1e-5
    gb = TC.loss_grad_bound(r, bd, 1.0)
    assert bool((gb > 0).all()) and gb.max().item() < 1e-5 * r.grad.abs().max().item()
    assert TC.K_FUNC == 4.0 * TC.K_ULP_MEASURED


# ------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("hp", [TC.DEFAULT_HP, dict(TC.DEFAULT_HP, wd=0.0), TC.EXACT_HP], ids=["default", "wd0", "exact"])
@pytest.mark.parametrize("t0", [1, 2, 10, 100000])
def test_adamw_reference_equals_torch_adamw_in_float64(hp, t0):
    n = 1001
    g = torch.Generator().manual_seed(t0)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1 if t0 > 1 else torch.zeros(n)
    v = torch.rand(n, generator=g) * 0.01 if t0 > 1 else torch.zeros(n)
    pr = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.AdamW([pr], lr=TC.f32(hp["lr"]), betas=(TC.f32(hp["beta1"]), TC.f32(hp["beta2"])), eps=TC.f32(hp["eps"]) or 1e-300,
                            weight_decay=TC.f32(hp["wd"]))
    opt.state[pr] = {"step": torch.tensor(float(t0 - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    gr = TC.rounded_adamw_grad(n, t0)
    if hp is TC.EXACT_HP:
        gr = gr.clamp(-10.0, 10.0) + 0.125          # eps = 0: keep the denominator away from zero
    pr.grad = gr.double() * 0.25
    opt.step()
    p1, m1, v1 = TC.adamw_ref(p, gr, m, v, hp, t0, 0.25)
    st = opt.state[pr]
    assert (m1 - st["exp_avg"]).abs().max().item() <= 1e-14 * m1.abs().max().item()
    assert bool(((v1 - st["exp_avg_sq"]).abs() <= 1e-14 * v1.abs() + 1e-300).all())
    assert (p1 - pr.detach()).abs().max().item() <= 1e-13
    bp, bm, bv = TC.adamw_bounds(p, gr, m, v, hp, t0, 0.25)
    assert bool((bp > 0).all()) and bool(torch.isfinite(bp).all()) and bool(torch.isfinite(bv).all())
    assert bp.max().item() <= 1e-6 * max(1.0, p.abs().max().item())     # a bound of a few roundings, nowhere a percent-level tolerance


@pytest.mark.parametrize("zero_grad", [False, True])
def test_adamw_exact_tier_every_intermediate_is_an_fp32_number(zero_grad):
    """The chain of adamw_elem in float64, with and without the gradient factor: each intermediate survives a round trip through fp32, so
    fp32 arithmetic forms it without rounding in any association and with or without fused multiply-adds."""
    n = 100003
    hp = dict(TC.EXACT_HP, eps=2.0 ** -20) if zero_grad else TC.EXACT_HP
    p, gr = TC.exact_adamw_inputs(n, 1, zero_grad)
    for scale_up, factor in [(1.0, 1.0), (2048.0, 2.0 ** -11)]:
        g = gr.double() * scale_up
        assert exact_in(g, "f32")
        gi = g * factor
        keep = 1.0 - hp["lr"] * hp["wd"]
        d = gi - 0.0
        e = d * (1.0 - hp["beta1"])
        m = 0.0 + e
        v = 0.0 * hp["beta2"] + (1.0 - hp["beta2"]) * gi * gi
        bc2s = math.sqrt(1.0 - hp["beta2"])
        step = hp["lr"] / (1.0 - hp["beta1"])
        den = v.sqrt() / bc2s + hp["eps"]
        ratio = m / den
        a, c = p.double() * keep, step * ratio
        out = a - c
        for t in (gi, d, e, m, (1.0 - hp["beta2"]) * gi, v, v.sqrt(), den, ratio, a, c, out, torch.tensor([keep, bc2s, step])):
            assert bool((t.float().double() == t).all())
        pe, me, ve = TC.exact_adamw_expected(p, gr)
        assert torch.equal(out, pe) and torch.equal(m, me) and torch.equal(v, ve)
        rp, rm, rv = TC.adamw_ref(p, (gr.double() * scale_up).float(), torch.zeros(n), torch.zeros(n), hp, 1, factor)
        assert torch.equal(rp, pe) and torch.equal(rm, me) and torch.equal(rv, ve)
        if not zero_grad:
            assert bool((gr != 0).all())


def test_ragged_segments():
    segs, total = TC.ragged_segments(TC.SEGMENT_LENGTHS)
    assert [e - b for b, e in segs] == TC.SEGMENT_LENGTHS and all(b % 4 for b, _ in segs)
    assert segs[0][0] > 0 and all(segs[i + 1][0] > segs[i][1] for i in range(len(segs) - 1)) and total > segs[-1][1]
    assert {1, 4095, 4096, 4097} <= set(TC.SEGMENT_LENGTHS) and max(TC.SEGMENT_LENGTHS) > 3 * 4096
