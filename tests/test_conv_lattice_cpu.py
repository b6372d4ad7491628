"""tests/conv_lattice.py without a GPU: every case of the convolution sweep meets the exactness conditions on its float64 reference alone
(so a case that breaks one fails here before it reaches a device), the reference of each fused form agrees with a naive float64 einsum
written tap by tap from the formulas of include/vk_unet.h, and it reacts to one changed input element, weight or channel scale."""
import pytest
import torch

import conv_lattice as CL

CASES = CL.all_cases()


def test_case_names_are_unique_per_kind():
    names = [(c.kind, c.name) for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", CASES, ids=[f"{c.kind}-{c.name}" for c in CASES])
def test_exactness_conditions_hold_on_the_reference(case):
    """100 % of the elements of every case: outputs and prologue values exact in every tested type, conv(|V|, |w|) < 2^24, the per-tile
    fp32 statistics partial < 2^24, 2 x result exact after accumulate (CL.check asserts each).  Room to spare: the largest stored value
    of a case stays under 3/4 of bf16's 256."""
    fig = CL.check(CL.build(case))
    if case.kind != "wgrad" and "bf16" in case.types:
        assert fig["max_out"] * (2 if case.accumulate and not case.bnr else 1) <= 192, fig


# ------------------------------------------------------------------------------------------------ naive restatement of include/vk_unet.h
def naive_V(b):
    """V[n][c][h][w] = act(src[n][c][h >> up][w >> up] * scale[c] + shift[c]), by index."""
    c = b.case
    parts = []
    for s, x, sc, sh in zip(c.srcs, b.x, b.scale, b.shift):
        hh, ww = torch.arange(c.H) >> s.up, torch.arange(c.W) >> s.up
        v = x[:, :, hh][:, :, :, ww]
        if s.pro:
            v = (v * sc[None, :, None, None] + sh[None, :, None, None]).clamp_min(0)
        parts.append(v)
    return torch.cat(parts, 1)


def naive_conv(V, w, Ho, Wo, R, stride, pad, transposed):
    """transposed 0: y[p] = sum_r V[p * stride - pad + r] w[r];  1: y[p] = sum_r V[(p + pad - r) / stride] w[r] where the division is
    exact and the index inside the map.  w [out][red][R][S]."""
    N, _, H, W = V.shape
    y = torch.zeros(N, w.shape[0], Ho, Wo, dtype=torch.float64)
    for r in range(R):
        for s in range(R):
            for p in range(Ho):
                for q in range(Wo):
                    if transposed:
                        a, bb = p + pad - r, q + pad - s
                        if a % stride or bb % stride:
                            continue
                        a, bb = a // stride, bb // stride
                    else:
                        a, bb = p * stride - pad + r, q * stride - pad + s
                    if 0 <= a < H and 0 <= bb < W:
                        y[:, :, p, q] += torch.einsum("nc,kc->nk", V[:, :, a, bb], w[:, :, r, s])
    return y


def naive_pool2(t):
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


S = CL.S
FORMS = [
    CL.Case("t_s2_a", "dgrad", 2, 6, 4, (S(8),), 8, stride=2, seed=1), CL.Case("t_s2_b", "dgrad", 1, 5, 7, (S(8),), 16, stride=2, seed=2),
    CL.Case("t_s2_1x1", "dgrad", 1, 4, 6, (S(8),), 8, R=1, stride=2, pad=0, seed=3), CL.Case("t_s1", "dgrad", 1, 3, 5, (S(8),), 8, accumulate=1, seed=4),
    CL.Case("upcat_a", "fwd", 2, 4, 6, (S(8, 1, True), S(8, 0, True)), 8, seed=5), CL.Case("upcat_b", "fwd", 1, 2, 8, (S(16, 1), S(8, 0, True)), 16, seed=6),
    CL.Case("s2_fwd", "fwd", 1, 5, 6, (S(8, 0, True),), 8, stride=2, seed=7),
    CL.Case("pool_a", "dgrad", 1, 4, 6, (S(8),), 8, pool2=1, seed=8), CL.Case("pool_b", "dgrad", 2, 2, 4, (S(8),), 24, split=16, pool2=1, seed=9),
    CL.Case("bnr_aff_a", "dgrad", 1, 3, 5, (S(8),), 16, bnr="affine", seed=10), CL.Case("bnr_aff_b", "dgrad", 2, 4, 2, (S(8),), 16, pool2=1, bnr="affine", accumulate=1, seed=11),
    CL.Case("bnr_mask_a", "dgrad", 1, 3, 5, (S(8),), 8, bnr="mask", accumulate=1, seed=12), CL.Case("bnr_mask_b", "dgrad", 2, 2, 3, (S(8),), 16, split=8, bnr="mask", seed=13),
    CL.Case("split_a", "dgrad", 1, 3, 4, (S(8),), 24, split=8, seed=14), CL.Case("split_b", "dgrad", 1, 2, 5, (S(8),), 24, split=16, accumulate=1, seed=15),
]


@pytest.mark.parametrize("case", FORMS, ids=[c.name for c in FORMS])
def test_reference_of_each_fused_form_against_naive_einsum(case):
    b = CL.build(case)
    if case.kind == "fwd":
        V = naive_V(b)
        assert torch.equal(V, b.V)
        Ho, Wo = case.out_hw
        y = naive_conv(V, b.w, Ho, Wo, case.R, case.stride, case.pad, 0)
        assert torch.equal(y, b.y)
        assert torch.equal(torch.stack([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))]), b.stats)
        return
    dx = naive_conv(b.dz, b.w, case.H, case.W, case.R, case.stride, case.pad, 1)
    assert torch.equal(dx, b.dx)
    k0 = case.split or case.K
    first = dx[:, :k0]
    if case.split:
        assert torch.equal(dx[:, k0:] + (b.old1 if case.accumulate else 0.0), b.y1)      # accumulate adds into the skip part too
    if case.pool2:
        first = naive_pool2(first)
    if case.accumulate:
        first = first + b.old
    if case.bnr == "affine":
        first = first * ((b.z * b.bn_scale[None, :, None, None] + b.bn_shift[None, :, None, None]) > 0)
    elif case.bnr == "mask":
        first = first * (b.mask > 0)
    assert torch.equal(first, b.y)
    if case.bnr:
        assert bool((b.y == 0).any()) and bool((b.y != 0).any())         # the mask removes some elements and keeps some
        assert torch.equal(torch.stack([first.sum(dim=(0, 2, 3)), (first * b.z).sum(dim=(0, 2, 3))]), b.sums)


def test_weight_gradient_reference_against_naive_einsum():
    for case in (CL.Case("w_a", "wgrad", 2, 3, 5, (S(8, 0, True),), 8, seed=16), CL.Case("w_up_s2", "wgrad", 1, 4, 6, (S(8, 1, True), S(8)), 8, stride=2, seed=17)):
        b = CL.build(case)
        V = naive_V(b)
        Ho, Wo = case.out_hw
        dw = torch.zeros_like(b.dw)
        for r in range(3):
            for s in range(3):
                for p in range(Ho):
                    for q in range(Wo):
                        a, bb = p * case.stride - 1 + r, q * case.stride - 1 + s
                        if 0 <= a < case.H and 0 <= bb < case.W:
                            dw[:, :, r, s] += torch.einsum("nk,nc->kc", b.dz[:, :, p, q], V[:, :, a, bb])
        assert torch.equal(dw, b.dw)


@pytest.mark.parametrize("what", ["input", "weight", "scale"])
def test_reference_reacts_to_one_changed_operand(what):
    base, new = CL.flip_changes(CL.Case("flip", "fwd", 1, 5, 7, (S(32, 0, True),), 16, seed=18), what)
    assert not torch.equal(base, new)
    if what != "weight":
        base, new = CL.flip_changes(CL.Case("flipw", "wgrad", 1, 5, 7, (S(32, 0, True),), 16, seed=19), what)
        assert not torch.equal(base, new)


def test_lattice_tables_differ_from_channel_to_channel():
    """A thread that leaves its 8-channel group reads other coefficients: the (scale, shift) pair repeats only every 21 channels."""
    sc, sh = CL.lat_scale(168, 0), CL.lat_int(168, 3, 7)
    for off in range(8, 168, 8):
        assert not (torch.equal(sc[off:], sc[:-off]) and torch.equal(sh[off:], sh[:-off])), off
