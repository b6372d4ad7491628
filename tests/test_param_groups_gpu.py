"""Param groups and global-norm clipping of the fused AdamW on the MI355X, on the cases of tests/param_groups_cases.py.

C ABI: vk_adamw_step_groups against vk_adamw_step_amp_segments bit for bit (one group; G groups against G calls; the clip coefficient
against a pre-multiplied inv_scale), against tail_cases' closed form and rounding bounds, and its skip rule; vk_grad_norm_segments
against float64 on the integer lattice (exact sums), on normal gradients (one ulp), with NaN in everything it must not read, and with
inf / NaN inside.  Buffers are sentinel-filled with guard elements either side; segments are ragged (begins that are no multiples of 4)
and one of them has 2^20 + 3 elements (257 chunks).

Python: FusedAdamW with a list of param-group dicts against the plain constructor and against torch.optim.AdamW with the same groups,
through a scheduler, freeze / unfreeze, clip_grad_norm_ against torch.nn.utils.clip_grad_norm_, GradScaler and grad_inv_scale, on
4 x 128 x 128 batches."""
import ctypes as C
import functools
import importlib
import math
from types import SimpleNamespace

import pytest
import torch

import param_groups_cases as PC
import tail_cases as TC

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
SENTINEL = PC.SENTINEL
GUARD = 4                      # guard elements either side of a buffer (keeps the 16-byte alignment of the payload)
TOL = 2e-7                     # the project's figure for one AdamW step against torch: about one ulp of weights of magnitude <= 2


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return vk.lib()


def P_(t):
    return None if t is None else t.data_ptr()


def scalar(v):
    return None if v is None else torch.full((1,), float(v), dtype=torch.float32, device=dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guarded(t, fill=SENTINEL):
    """(whole buffer, payload view) on the device: the payload sits between GUARD sentinel elements either side."""
    full = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=dev())
    v = full[GUARD:GUARD + t.numel()]
    v.copy_(t)
    return full, v


def guards_ok(full, fill=SENTINEL):
    e = torch.full((GUARD,), fill, dtype=full.dtype, device=full.device)
    return same_bits(full[:GUARD], e) and same_bits(full[-GUARD:], e)


def seg_tables(segs):
    """segs: [(begin, end, tensor_index)].  Device tables of the segmented entry points."""
    seg = torch.tensor([list(s) for s in segs], dtype=torch.int64)
    sp = C.cast(seg.data_ptr(), C.POINTER(C.c_int64))
    nb = lib().vk_adamw_segment_blocks(len(segs), sp, None, 0)
    assert nb >= len(segs)
    blocks = torch.empty((nb, 2), dtype=torch.int32)
    assert lib().vk_adamw_segment_blocks(len(segs), sp, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), nb) == nb
    return seg.to(dev()), blocks.to(dev()), nb


@functools.lru_cache(maxsize=None)
def ragged():
    """The ragged layout with tensor_index = position: ([(begin, end, index)], total, mask of the elements inside a segment)."""
    ranges, total = PC.layout()
    segs = [(b, e, i) for i, (b, e) in enumerate(ranges)]
    inside = torch.zeros(total, dtype=torch.bool)
    for b, e, _ in segs:
        inside[b:e] = True
    return segs, total, inside


@functools.lru_cache(maxsize=None)
def host_state(seed, kind="rounded"):
    """Host tensors p0, m0, v0, g over the ragged layout (shared by the tests, never written): sentinels in the gaps of p, m, v and g.
    kind "rounded": normal state and tail_cases' rounded gradients; "exact": tail_cases' exact tier (zero moments, p on the 1/16 grid,
    integer gradients)."""
    segs, total, inside = ragged()
    if kind == "exact":
        p0, gr = PC.exact_adamw_inputs(total, seed)
        m0, v0 = torch.zeros(total), torch.zeros(total)
    else:
        g = torch.Generator().manual_seed(seed)
        p0, m0 = torch.randn(total, generator=g), torch.randn(total, generator=g) * 0.1
        v0 = torch.rand(total, generator=g) * 0.01 + 1e-6           # > 0: with eps = 0 the quotient stays defined
        gr = PC.rounded_adamw_grad(total, seed)
    for t in (p0, m0, v0, gr):
        t[~inside] = SENTINEL
    return SimpleNamespace(p0=p0, m0=m0, v0=v0, g=gr)


class DevState:
    """A device copy of a host state with guard elements, and per-tensor counters."""

    def __init__(self, h, counters):
        self.h = h
        self.P, self.p = guarded(h.p0)
        self.M, self.m = guarded(h.m0)
        self.V, self.v = guarded(h.v0)
        self.G, self.g = guarded(h.g)
        self.cnt = torch.tensor(counters, dtype=torch.int32, device=dev())

    def ptrs(self):
        return self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr()

    def snapshot(self):
        return [t.clone() for t in (self.p, self.m, self.v, self.cnt)]

    def intact_outside(self):
        """Guards, and the gaps between segments, still hold their sentinels; the gradient buffer is unwritten."""
        _, _, inside = ragged()
        out = (~inside).to(dev())
        ok = all(guards_ok(f) for f in (self.P, self.M, self.V, self.G))
        ok = ok and all(bool((t[out] == SENTINEL).all()) for t in (self.p, self.m, self.v))
        return ok and same_bits(self.g, self.h.g.to(dev()))


def hp_struct(hps):
    return (L_.vk_adamw_group * len(hps))(*[L_.vk_adamw_group(h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"]) for h in hps])


def step_groups(s, segs, group_idx, hps, inv_scale, gs=None, fi=None, clip=None):
    seg, blocks, nb = seg_tables(segs)
    sg = torch.tensor(group_idx, dtype=torch.int32, device=dev())
    scratch = torch.zeros(4 + 2 * len(segs), device=dev())
    L_.check(lib().vk_adamw_step_groups(len(segs), seg.data_ptr(), sg.data_ptr(), nb, blocks.data_ptr(), *s.ptrs(), len(hps), hp_struct(hps),
                                        s.cnt.data_ptr(), inv_scale, P_(gs), P_(fi), P_(clip), scratch.data_ptr(), st()),
             "vk_adamw_step_groups")


def step_segments(s, segs, hp, inv_scale, gs=None, fi=None):
    seg, blocks, nb = seg_tables(segs)
    scratch = torch.zeros(4 + 2 * len(segs), device=dev())
    L_.check(lib().vk_adamw_step_amp_segments(len(segs), seg.data_ptr(), nb, blocks.data_ptr(), *s.ptrs(), hp["lr"], hp["beta1"], hp["beta2"],
                                              hp["eps"], hp["wd"], s.cnt.data_ptr(), inv_scale, P_(gs), P_(fi), scratch.data_ptr(), st()),
             "vk_adamw_step_amp_segments")


def assert_same_state(a, b, label):
    torch.cuda.synchronize()
    for nm, x, y in (("p", a.P, b.P), ("exp_avg", a.M, b.M), ("exp_avg_sq", a.V, b.V)):
        if not same_bits(x, y):
            i = int((bits(x) != bits(y)).nonzero()[0]) - GUARD
            raise AssertionError(f"{label}: {nm}[{i}] differs: {x[i + GUARD].item()!r} vs {y[i + GUARD].item()!r}")
    assert torch.equal(a.cnt, b.cnt), (label, a.cnt.tolist(), b.cnt.tolist())
    assert a.intact_outside() and b.intact_outside(), f"{label}: a gap, a guard or the gradient buffer was written"


COUNTERS = [0, 1, 9, 99, 1234, 4, 77, 2, 99999, 6]


# ================================================================================================ C ABI: the grouped step
@pytest.mark.parametrize("grad_scale", [None, 1024.0])
def test_one_group_without_coefficient_equals_the_segmented_kernel(grad_scale):
    segs, _, _ = ragged()
    h = host_state(31)
    a, b = DevState(h, COUNTERS), DevState(h, COUNTERS)
    gs = scalar(grad_scale)
    taken = 0
    for found in (0.0, 1.0, 0.0):
        fi = scalar(found)
        before = a.snapshot()
        step_groups(a, segs, [0] * len(segs), [TC.DEFAULT_HP], 0.5, gs, fi, None)
        step_segments(b, segs, TC.DEFAULT_HP, 0.5, gs, fi)
        assert_same_state(a, b, f"found_inf {found}")
        if found:
            assert all(same_bits(x, y) for x, y in zip(before, a.snapshot()))
        else:
            taken += 1
            assert not same_bits(before[0], a.p)
    assert a.cnt.tolist() == [c + taken for c in COUNTERS]


@pytest.mark.parametrize("G", PC.GROUP_COUNTS)
def test_groups_equal_one_segmented_call_per_group(G):
    segs, _, _ = ragged()
    h = host_state(32)
    hps = PC.HP_SETS[:G]
    gidx = [PC.group_index(i, G) for i in range(len(segs))]
    a, b = DevState(h, COUNTERS), DevState(h, COUNTERS)
    gs = scalar(1024.0)
    for found in (0.0, 1.0, 0.0):
        fi = scalar(found)
        step_groups(a, segs, gidx, hps, 0.5, gs, fi, None)
        for k in range(G):
            step_segments(b, [s for s, gi in zip(segs, gidx) if gi == k], hps[k], 0.5, gs, fi)
        assert_same_state(a, b, f"G = {G}, found_inf {found}")
    assert a.cnt.tolist() == [c + 2 for c in COUNTERS]
    # lr = 0 (HP_SETS[1]): the parameters keep their bits, the moments move; everyone else's parameters move
    p, m, v = a.p.cpu(), a.m.cpu(), a.v.cpu()
    for (b_, e_, _), gi in zip(segs, gidx):
        sl = slice(b_, e_)
        assert same_bits(p[sl], h.p0[sl]) == (hps[gi]["lr"] == 0.0), (b_, gi)
        assert not same_bits(m[sl], h.m0[sl]) and not same_bits(v[sl], h.v0[sl]), (b_, gi)


def test_exact_first_step_through_groups_and_coefficient():
    """EXACT_HP with inv_scale = 2 and clip coefficient 0.5 (factor exactly 1) on zero moments: tail_cases' closed form, exactly, on the
    segments of that group; its neighbours run DEFAULT_HP."""
    segs, _, _ = ragged()
    h = host_state(33, "exact")
    gidx = [PC.group_index(i, 2) for i in range(len(segs))]
    a = DevState(h, [0] * len(segs))
    step_groups(a, segs, gidx, [TC.EXACT_HP, TC.DEFAULT_HP], 2.0, None, scalar(0.0), scalar(0.5))
    torch.cuda.synchronize()
    assert a.intact_outside() and a.cnt.tolist() == [1] * len(segs)
    p, m, v = a.p.cpu(), a.m.cpu(), a.v.cpu()
    for (b_, e_, _), gi in zip(segs, gidx):
        sl = slice(b_, e_)
        if gi == 0:
            pe, me, ve = TC.exact_adamw_expected(h.p0[sl], h.g[sl])
            for nm, got, want in (("p", p[sl], pe), ("exp_avg", m[sl], me), ("exp_avg_sq", v[sl], ve)):
                assert torch.equal(got.double(), want), (nm, b_, e_)
        else:
            assert not same_bits(p[sl], h.p0[sl])


@pytest.mark.parametrize("clip,grad_scale", [(0.37, None), (1.0, None), (2.0 ** -3, None), (2.0 ** -3, 2.0 ** 10)])
def test_clip_coefficient_is_one_rounding_of_the_product(clip, grad_scale):
    """groups(inv_scale, coefficient c) == segments(inv_scale' = fp32(double(inv_scale) * double(c))): a product of two fp32 values is exact in
    double, so both sides round once.  With grad_scale = 2^10 and c = 2^-3 both quotients are exact as well."""
    segs, _, _ = ragged()
    h = host_state(34)
    inv = TC.f32(0.3)
    inv2 = PC.fused_factor(inv, None, clip)
    assert inv2 == TC.f32(inv2) and (clip == 1.0) == (inv2 == inv)
    a, b = DevState(h, COUNTERS), DevState(h, COUNTERS)
    gs = scalar(grad_scale)
    step_groups(a, segs, [0] * len(segs), [TC.DEFAULT_HP], inv, gs, scalar(0.0), scalar(clip))
    step_segments(b, segs, TC.DEFAULT_HP, inv2, gs, scalar(0.0))
    assert_same_state(a, b, f"clip {clip}")
    assert not same_bits(a.p, h.p0.to(dev()))
    if clip != 1.0:                         # and the coefficient was applied at all
        c = DevState(h, COUNTERS)
        step_segments(c, segs, TC.DEFAULT_HP, inv, gs, scalar(0.0))
        torch.cuda.synchronize()
        assert not same_bits(a.m, c.m)


@pytest.mark.parametrize("t", [1, 7])
def test_clipped_step_within_the_rounding_bounds(t):
    segs, _, _ = ragged()
    h = host_state(35 + t)
    factor = PC.fused_factor(2.0 ** -11, None, 0.37)
    gidx = [PC.group_index(i, 2) for i in range(len(segs))]
    a = DevState(h, [t - 1] * len(segs))
    step_groups(a, segs, gidx, [TC.DEFAULT_HP, TC.DEFAULT_HP], 2.0 ** -11, None, None, scalar(0.37))
    torch.cuda.synchronize()
    assert a.intact_outside() and a.cnt.tolist() == [t] * len(segs)
    p, m, v = a.p.cpu(), a.m.cpu(), a.v.cpu()
    for b_, e_, _ in segs:
        sl = slice(b_, e_)
        pr, mr, vr = TC.adamw_ref(h.p0[sl], h.g[sl], h.m0[sl], h.v0[sl], TC.DEFAULT_HP, t, factor)
        bp, bm, bv = TC.adamw_bounds(h.p0[sl], h.g[sl], h.m0[sl], h.v0[sl], TC.DEFAULT_HP, t, factor)
        for nm, got, want, bound in (("p", p[sl], pr, bp), ("exp_avg", m[sl], mr, bm), ("exp_avg_sq", v[sl], vr, bv)):
            err = (got.double() - want).abs()
            i = int((err - bound).argmax())
            assert bool((err <= bound).all()), f"t {t}: segment [{b_}, {e_}): {nm}[{b_ + i}]: error {err[i].item():.3e} > bound {bound[i].item():.3e}"
        assert not same_bits(p[sl], h.p0[sl])


def test_skipped_step_with_a_coefficient_writes_nothing():
    segs, _, _ = ragged()
    h = host_state(31)
    gidx = [PC.group_index(i, 3) for i in range(len(segs))]
    for flag in (1.0, -1.0, float("nan")):
        a = DevState(h, COUNTERS)
        before = a.snapshot()
        step_groups(a, segs, gidx, PC.HP_SETS[:3], 0.5, scalar(1024.0), scalar(flag), scalar(0.37))
        torch.cuda.synchronize()
        assert all(same_bits(x, y) for x, y in zip(before, a.snapshot())), flag
        assert a.intact_outside() and a.cnt.tolist() == COUNTERS


# ================================================================================================ C ABI: the norm
def run_norm(gbuf, segs, kind, inv_scale, max_norm, prefill=None):
    """One call over `segs` of the device buffer gbuf.  Returns (total, coefficient) as fp32 tensors on the host, and the partials."""
    seg, blocks, nb = seg_tables(segs)
    partials = torch.zeros(nb, dtype=torch.float64, device=dev())
    out = torch.zeros(2, dtype=torch.float32, device=dev())
    if prefill is not None:
        partials.fill_(prefill)
        out.fill_(prefill)
    L_.check(lib().vk_grad_norm_segments(len(segs), seg.data_ptr(), nb, blocks.data_ptr(), gbuf.data_ptr(), kind, inv_scale, max_norm,
                                         partials.data_ptr(), out.data_ptr(), st()), "vk_grad_norm_segments")
    torch.cuda.synchronize()
    return out.cpu(), partials.cpu()


def check_norm(out, parts, kind, inv_scale, max_norm, label, exact=False):
    total = PC.norm_ref(parts, kind, inv_scale)
    got = out[0].double().item()
    if exact:
        assert got == total, f"{label}: norm {got!r}, float64 {total!r}"
    else:
        assert abs(got - total) <= PC.ulp32(total), f"{label}: norm {got!r}, float64 {total!r}, ulp {PC.ulp32(total):.3e}"
    c = PC.coef_ref(total, max_norm)
    gc = out[1].double().item()
    assert abs(gc - c) <= PC.ulp32(c), f"{label}: coefficient {gc!r}, float64 {c!r}"
    if total < TC.f32(max_norm) - 1e-6:
        assert gc == 1.0, f"{label}: coefficient {gc!r} for norm {total!r} below max_norm {max_norm!r}"
    if max_norm == 0.0 and total == total:
        assert gc == 0.0, label
    return total


@functools.lru_cache(maxsize=None)
def lattice_on_device(n, begin):
    """A sentinel-filled buffer holding lattice gradients at [begin, begin + n)."""
    g = PC.lattice_grad(n, n)
    host = torch.full((begin + n + 5,), SENTINEL)
    host[begin:begin + n] = g
    full, view = guarded(host)
    return g, full, view


@pytest.mark.parametrize("n", TC.ADAMW_SIZES)
def test_norm_lattice_single_segment(n):
    for begin in (0, 3):                    # a 16-byte aligned begin and one that is not
        g, full, view = lattice_on_device(n, begin)
        segs = [(begin, begin + n, 0)]
        s = PC.int_sum_squares(g)
        root = math.isqrt(s)
        for inv in (1.0, 0.5):
            total = math.sqrt(s) * inv
            for max_norm in (0.5 * total, 2.0 * total + 1.0, 0.0):
                label = f"n {n} begin {begin} inv_scale {inv} max_norm {max_norm}"
                out, _ = run_norm(view, segs, PC.NORM_L2, inv, max_norm)
                check_norm(out, [g], PC.NORM_L2, inv, max_norm, "L2 " + label, exact=(root * root == s and root < 2 ** 24))
                out, _ = run_norm(view, segs, PC.NORM_INF, inv, max_norm)
                check_norm(out, [g], PC.NORM_INF, inv, max_norm, "INF " + label, exact=True)
        assert guards_ok(full)


def test_norm_lattice_ragged_segments():
    segs, total, inside = ragged()
    g = PC.lattice_grad(total, 3)
    host = g.clone()
    host[~inside] = SENTINEL
    full, view = guarded(host)
    parts = [g[b:e] for b, e, _ in segs]
    for inv in (1.0, 0.5):
        ref = PC.norm_ref(parts, PC.NORM_L2, inv)
        for max_norm in (0.5 * ref, 2.0 * ref, 0.0):
            out, partials = run_norm(view, segs, PC.NORM_L2, inv, max_norm)
            check_norm(out, parts, PC.NORM_L2, inv, max_norm, f"L2 ragged inv_scale {inv} max_norm {max_norm}")
            out, _ = run_norm(view, segs, PC.NORM_INF, inv, max_norm)
            check_norm(out, parts, PC.NORM_INF, inv, max_norm, f"INF ragged inv_scale {inv} max_norm {max_norm}", exact=True)
    # every partial is the exact integer sum of its chunk
    want = [float(PC.int_sum_squares(g[b + c * PC.CHUNK:min(b + (c + 1) * PC.CHUNK, e)]))
            for b, e, _ in segs for c in range((e - b + PC.CHUNK - 1) // PC.CHUNK)]
    assert partials.tolist() == want
    assert guards_ok(full)


@pytest.mark.parametrize("n", PC.THREES_LENGTHS)
def test_norm_of_threes_is_the_integer_root(n):
    g = PC.threes(n, n)
    full, view = guarded(torch.cat([torch.full((1,), SENTINEL), g]))
    root = 3.0 * math.sqrt(n)
    assert root == int(root)
    for inv in (1.0, 0.5):
        out, _ = run_norm(view, [(1, 1 + n, 0)], PC.NORM_L2, inv, 1.0)
        assert out[0].item() == root * inv, (n, inv)
        check_norm(out, [g], PC.NORM_L2, inv, 1.0, f"threes {n}", exact=True)
        out, _ = run_norm(view, [(1, 1 + n, 0)], PC.NORM_INF, inv, 100.0)
        assert out[0].item() == 3.0 * inv and out[1].item() == 1.0


def test_norm_of_zero_gradients():
    full, view = guarded(torch.zeros(5000))
    for kind in (PC.NORM_L2, PC.NORM_INF):
        out, _ = run_norm(view, [(3, 4999, 0)], kind, 1.0, 1.0, prefill=float("nan"))
        assert out.tolist() == [0.0, 1.0], kind
        out, _ = run_norm(view, [(3, 4999, 0)], kind, 1.0, 0.0)
        assert out.tolist() == [0.0, 0.0], kind


def test_norm_rounded_within_one_ulp():
    n = PC.LARGE
    g = torch.randn(n, generator=torch.Generator().manual_seed(77))
    full, view = guarded(torch.cat([torch.full((3,), SENTINEL), g]))
    segs = [(3, 3 + n, 0)]
    for inv in (1.0, TC.f32(1.0 / 3.0)):
        ref = PC.norm_ref([g], PC.NORM_L2, inv)
        for max_norm in (0.5 * ref, 2.0 * ref):
            out, _ = run_norm(view, segs, PC.NORM_L2, inv, max_norm)
            check_norm(out, [g], PC.NORM_L2, inv, max_norm, f"normal L2 inv_scale {inv} max_norm {max_norm}")
            out, _ = run_norm(view, segs, PC.NORM_INF, inv, max_norm)
            check_norm(out, [g], PC.NORM_INF, inv, max_norm, f"normal INF inv_scale {inv} max_norm {max_norm}")


def test_norm_reads_listed_segments_only_and_keeps_nothing():
    """NaN in the gaps, in the unlisted segments and in the guards; partials and out prefilled with NaN; two calls: the same bits."""
    segs, total, inside = ragged()
    listed = [s for i, s in enumerate(segs) if i % 2 == 1]          # the large segment is the last, index 9
    g = torch.randn(total, generator=torch.Generator().manual_seed(78))
    mask = torch.zeros(total, dtype=torch.bool)
    for b, e, _ in listed:
        mask[b:e] = True
    host = g.clone()
    host[~mask] = float("nan")
    full, view = guarded(host, fill=float("nan"))
    parts = [g[b:e] for b, e, _ in listed]
    for kind in (PC.NORM_L2, PC.NORM_INF):
        ref = PC.norm_ref(parts, kind, 1.0)
        o1, p1 = run_norm(view, listed, kind, 1.0, 0.5 * ref)
        check_norm(o1, parts, kind, 1.0, 0.5 * ref, f"listed only, kind {kind}")
        o2, p2 = run_norm(view, listed, kind, 1.0, 0.5 * ref, prefill=float("nan"))
        o3, p3 = run_norm(view, listed, kind, 1.0, 0.5 * ref, prefill=1e30)
        assert same_bits(o1, o2) and same_bits(o1, o3), kind
        assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)) and torch.equal(p1.view(torch.int64), p3.view(torch.int64)), kind
    assert same_bits(view, host.to(dev())) and guards_ok(full, float("nan"))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_norm_with_a_non_finite_element(bad):
    segs, total, inside = ragged()
    base = torch.randn(total, generator=torch.Generator().manual_seed(79))
    for where in (segs[0][0], segs[4][1] - 1, segs[9][0] + 200 * PC.CHUNK + 17, segs[9][1] - 1):
        host = base.clone()
        host[where] = bad
        full, view = guarded(host)
        for kind in (PC.NORM_L2, PC.NORM_INF):
            out, _ = run_norm(view, segs, kind, 1.0, 1.0)
            if bad != bad:
                assert math.isnan(out[0].item()) and math.isnan(out[1].item()), (where, kind)
            else:
                assert out[0].item() == float("inf") and out[1].item() == 0.0, (where, kind)


# ================================================================================================ Python level
def build(seed=21):
    from oracle import unet_oracle as O
    O.set_seed(seed)
    return vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev()).train()


def batch(step=0, n=4, s=128):
    from oracle import unet_oracle as O
    x, y = O.synthetic_batch(n, s, seed=300 + step)
    return x.to(dev()), y.to(dev())


def backward(m, opt, step):
    opt.zero_grad(set_to_none=True)
    m.loss_and_backward(*batch(step), dtype=torch.bfloat16)


def compare(m, ref, label, tol=TOL):
    torch.cuda.synchronize()
    for (name, p), r in zip(m.named_parameters(), ref):
        err = (p.detach() - r.detach()).abs().max().item()
        assert err <= tol, (label, name, err)


def owned_norm64(m, inv_scale=1.0):
    return PC.norm_ref([p.grad.detach().cpu() for p in m.parameters() if p.grad is not None], PC.NORM_L2, inv_scale)


def test_one_group_as_a_list_of_dicts_equals_the_plain_constructor():
    a, b = build(), build()
    opt_a = vk.FusedAdamW(a.parameters(), lr=5e-5, weight_decay=1e-4).attach(a)
    opt_b = vk.FusedAdamW([dict(params=b.parameters(), lr=5e-5)], lr=1.0, weight_decay=1e-4).attach(b)
    for step in range(3):
        backward(a, opt_a, step)
        backward(b, opt_b, step)
        opt_a.step()
        opt_b.step()
        torch.cuda.synchronize()
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            assert same_bits(pa.detach(), pb.detach()), (step, n)
    assert opt_b._steps_dev is None and opt_b.step_count == 3       # the whole-buffer kernel ran, as for the plain constructor
    assert same_bits(opt_a._m, opt_b._m) and same_bits(opt_a._v, opt_b._v)


def test_three_groups_match_torch_through_a_cosine_schedule():
    m = build()
    lr = 5e-5
    spec = PC.three_groups(vk, m, lr)
    assert [len(ids) for ids, _ in spec] == [36, 11, 93]
    opt = vk.FusedAdamW(PC.as_param_groups(spec, m.parameters()), lr=lr).attach(m)
    ref = PC.ref_copies(m)
    ref_opt = torch.optim.AdamW(PC.as_param_groups(spec, ref), lr=lr, foreach=False)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4)
    ref_sch = torch.optim.lr_scheduler.CosineAnnealingLR(ref_opt, T_max=4)
    for step in range(4):
        backward(m, opt, step)
        opt.step()
        PC.feed(ref, m)
        ref_opt.step()
        compare(m, ref, step)
        PC.resync(ref, m)
        sch.step()
        ref_sch.step()
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ref_opt.param_groups]
    assert opt.tensor_steps() == [4] * 140


def test_groups_through_freeze_and_unfreeze_count_like_torch():
    m = build()
    lr = 5e-5
    spec = PC.three_groups(vk, m, lr)
    opt = vk.FusedAdamW(PC.as_param_groups(spec, m.parameters()), lr=lr).attach(m)
    ref = PC.ref_copies(m)
    ref_opt = torch.optim.AdamW(PC.as_param_groups(spec, ref), lr=lr, foreach=False)
    for step in range(4):
        m.encoder.requires_grad_(step >= 2)
        backward(m, opt, step)
        opt.step()
        PC.feed(ref, m)
        ref_opt.step()
        compare(m, ref, step)
        PC.resync(ref, m)
        want = [int(ref_opt.state[r]["step"]) if r in ref_opt.state and "step" in ref_opt.state[r] else 0 for r in ref]
        assert opt.tensor_steps() == want, step
    assert sorted(set(opt.tensor_steps())) == [2, 4]


def test_clip_grad_norm_matches_float64_and_torch():
    """eps is set to the median over the tensors of their largest first gradient, so that the update depends on the gradient's scale (with
    the default eps AdamW all but ignores it: at step 1 it is lr g / (|g| + eps)), max_norm to half the step's norm; clipped on steps 0
    and 2 only.  The unclipped reference must leave the clipped one by more than 10 x the tolerance on at least half of the tensors, or
    the comparison shows nothing: with |g| = r eps the two first updates differ by lr r / ((r + 1)(r + 2)), above 2e-6 for lr = 1e-3 and
    r in [0.005, 400]."""
    m = build()
    lr = 1e-3
    spec = PC.three_groups(vk, m, lr)
    opt = vk.FusedAdamW(PC.as_param_groups(spec, m.parameters()), lr=lr).attach(m)
    ref, ref_u = PC.ref_copies(m), PC.ref_copies(m)
    ref_opt = torch.optim.AdamW(PC.as_param_groups(spec, ref), lr=lr, foreach=False)
    ref_u_opt = torch.optim.AdamW(PC.as_param_groups(spec, ref_u), lr=lr, foreach=False)
    for step in range(3):
        backward(m, opt, step)
        total = owned_norm64(m)
        max_norm = TC.f32(0.5 * total)
        if step == 0:
            eps = torch.stack([p.grad.detach().abs().max() for p in m.parameters()]).median().item()
            assert eps > 0.0
            for o in (opt, ref_opt, ref_u_opt):
                for g in o.param_groups:
                    g["eps"] = eps
        PC.feed(ref, m)
        PC.feed(ref_u, m)
        if step != 1:
            got = vk.clip_grad_norm_(opt, max_norm)
            assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
            assert abs(got.double().item() - total) <= PC.ulp32(total), (step, got.item(), total)
            torch.nn.utils.clip_grad_norm_(ref, max_norm, foreach=False)
        opt.step()
        ref_opt.step()
        ref_u_opt.step()
        compare(m, ref, step)
        if step != 1:
            far = sum((a.detach() - b.detach()).abs().max().item() > 10 * TOL for a, b in zip(ref, ref_u))
            assert far >= 70, (step, far)
        PC.resync(ref, m)
        PC.resync(ref_u, m)


def test_coefficient_lifecycle():
    # (a) p.grad keeps its bits, the coefficient applies to exactly one step
    a, b = build(), build()
    opt_a, opt_b = vk.adamw_for(a, lr=5e-5), vk.adamw_for(b, lr=5e-5)
    for step in range(2):
        backward(a, opt_a, step)
        backward(b, opt_b, step)
        total = owned_norm64(a)
        g0 = a.flat_grads.clone()
        if step == 0:
            opt_a.clip_grad_norm_(0.25 * total)
            opt_b.clip_grad_norm_(0.25 * total)
        else:
            opt_b.clip_grad_norm_(1e30)      # coefficient exactly 1: the bits of a step without one
        assert same_bits(a.flat_grads, g0) and all(same_bits(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
        assert (opt_a._clip_coef is not None) == (step == 0)
        opt_a.step()
        opt_b.step()
        assert opt_a._clip_coef is None and opt_b._clip_coef is None
        torch.cuda.synchronize()
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            assert same_bits(pa.detach(), pb.detach()), (step, n)
    # (b) clip; zero_grad; backward; step == an unclipped step
    c, d = build(), build()
    opt_c, opt_d = vk.adamw_for(c, lr=5e-5), vk.adamw_for(d, lr=5e-5)
    backward(c, opt_c, 0)
    opt_c.clip_grad_norm_(1e-3)
    backward(c, opt_c, 0)                    # zero_grad inside: the coefficient is gone
    assert opt_c._clip_coef is None
    opt_c.step()
    backward(d, opt_d, 0)
    opt_d.step()
    torch.cuda.synchronize()
    for (n, pc), pd in zip(c.named_parameters(), d.parameters()):
        assert same_bits(pc.detach(), pd.detach()), n
    assert opt_c._steps_dev is None          # and the default path was never left


_BCE = torch.nn.BCEWithLogitsLoss()
_DICE = vk.DiceLoss(mode="binary")


@pytest.mark.parametrize("scaler_cls", ["vk", "torch"])
def test_amp_unscale_clip_step_update_with_a_forced_overflow(scaler_cls):
    """fp16 + GradScaler in torch's order.  Step 1 overflows (scale 2^60): nothing is written or counted, and its coefficient (0 or NaN)
    is consumed by the skipped step: step 2, which does not clip, matches the unclipped reference."""
    m = build()
    spec = PC.three_groups(vk, m, 5e-5)
    opt = vk.FusedAdamW(PC.as_param_groups(spec, m.parameters()), lr=5e-5).attach(m)
    scaler = vk.GradScaler("cuda", init_scale=2.0 ** 10) if scaler_cls == "vk" else torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    ref = PC.ref_copies(m)
    ref_opt = torch.optim.AdamW(PC.as_param_groups(spec, ref), lr=5e-5, foreach=False)
    taken = 0
    for step in range(4):
        if step in (1, 2):
            scaler.update(new_scale=2.0 ** 60 if step == 1 else 2.0 ** 10)     # step 1: forced overflow (inf fp16 gradients)
        opt.zero_grad(set_to_none=True)
        x, y = batch(step)
        with torch.autocast("cuda", dtype=torch.float16):
            logits = m(x)
        loss = _BCE(logits.float(), y) + _DICE(logits.float(), y)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        finite = all(torch.isfinite(p.grad).all().item() for p in m.parameters())
        assert finite != (step == 1), step
        before = [p.detach().clone() for p in m.parameters()]
        if finite:
            PC.feed(ref, m)                  # unscale_ has already divided the gradients by the scale
        if step != 2:
            total = owned_norm64(m) if finite else float("nan")
            max_norm = TC.f32(0.5 * total) if finite else 1.0
            got = opt.clip_grad_norm_(max_norm)
            if finite:
                assert abs(got.double().item() - total) <= PC.ulp32(total), step
                torch.nn.utils.clip_grad_norm_(ref, max_norm, foreach=False)
            else:
                assert not math.isfinite(got.item())
        scaler.step(opt)
        scaler.update()
        assert opt._clip_coef is None
        if finite:
            taken += 1
            ref_opt.step()
        torch.cuda.synchronize()
        assert opt.tensor_steps() == [taken] * 140, step
        if step == 1:
            assert all(torch.equal(p.detach(), b) for p, b in zip(m.parameters(), before))
        compare(m, ref, step)
        PC.resync(ref, m)
    assert taken == 3


def test_grad_inv_scale_folds_into_norm_and_step():
    """grad_inv_scale = 0.5 by hand: what the data-parallel reducer sets for two ranks."""
    m = build()
    opt = vk.adamw_for(m, lr=5e-5)
    ref = PC.ref_copies(m)
    ref_opt = torch.optim.AdamW(ref, lr=5e-5, weight_decay=1e-4, foreach=False)
    backward(m, opt, 0)
    one = opt.clip_grad_norm_(1.0).clone()
    opt.grad_inv_scale = 0.5
    max_norm = TC.f32(0.25 * owned_norm64(m))                    # half of the halved norm
    half = opt.clip_grad_norm_(max_norm)
    assert half.item() == 0.5 * one.item()
    assert abs(half.double().item() - owned_norm64(m, 0.5)) <= PC.ulp32(owned_norm64(m, 0.5))
    opt.step()
    PC.feed(ref, m, 0.5)
    torch.nn.utils.clip_grad_norm_(ref, max_norm, foreach=False)
    ref_opt.step()
    compare(m, ref, "grad_inv_scale 0.5")
    assert opt.tensor_steps() == [1] * 140
