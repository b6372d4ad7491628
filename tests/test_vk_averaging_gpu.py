"""vk.averaging on the device: vk_avg_update and vk_avg_swap against the numpy restatement (tests/averaging_ref.py) bit for bit, the exact
lattice tier against float64, the skip rule, vk_adamw_step_amp_avg against vk_adamw_step_amp + vk_avg_update, and ModelEMA / SWA on whole
models: attached against separate, within the proved bound of torch.lerp, applied() against the engine's caches, state round trips.
Cases, tiers and bounds: tests/averaging_cases.py (proved without a GPU by tests/test_averaging_cpu.py)."""
import importlib
import io
import math

import numpy as np
import pytest
import torch

import averaging_cases as AC
import averaging_ref as R
import tail_cases as TC

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
SENTINEL = AC.SENTINEL
GUARD = 4                      # guard elements either side of a payload (keeps its 16-byte alignment)


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def P_(t):
    return None if t is None else t.data_ptr()


def scalar(v):
    return None if v is None else torch.full((1,), float(v), dtype=torch.float32, device=dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guarded(t, shift=0):
    """(whole buffer, payload view) on the device: the payload sits `shift` elements past a 16-byte boundary, sentinels either side."""
    full = torch.full((t.numel() + 2 * GUARD + shift,), SENTINEL, dtype=torch.float32, device=dev())
    v = full[GUARD + shift:GUARD + shift + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * (shift % 4)
    return full, v


def guards_ok(full, v):
    lo = (v.data_ptr() - full.data_ptr()) // 4
    rest = torch.cat([full[:lo], full[lo + v.numel():]])
    return same_bits(rest, torch.full_like(rest, SENTINEL))


def rule(kind=R.EMA, decay=0.9, warmup=False):
    return L_.vk_avg_rule(kind, decay, 1 if warmup else 0)


def ranges_of(pairs):
    return (L_.vk_avg_range * len(pairs))(*[L_.vk_avg_range(a.data_ptr() if a.numel() else None, s.data_ptr() if s.numel() else None,
                                                            a.numel()) for a, s in pairs])


def avg_update(pairs, rl, count, fi=None, scratch=None):
    scratch = torch.full((2,), SENTINEL, dtype=torch.float32, device=dev()) if scratch is None else scratch
    vk._lib.check(vk.lib().vk_avg_update(len(pairs), ranges_of(pairs), rl, count.data_ptr(), P_(fi), scratch.data_ptr(), st()),
                  "vk_avg_update")
    return scratch


def avg_swap(pairs):
    vk._lib.check(vk.lib().vk_avg_swap(len(pairs), ranges_of(pairs), st()), "vk_avg_swap")


def counter(v=0):
    return torch.full((1,), v, dtype=torch.int32, device=dev())


# the layouts of one call: [(length, shift of avg, shift of src)]
LAYOUTS = {
    "two": [(4097, 0, 0), (3, 0, 0)],
    "empty_second": [(257, 0, 0), (0, 0, 0)],
    "four": [(255, 0, 0), (1, 0, 0), (4097, 0, 0), (2, 0, 0)],
    "head_and_tail": [(4097, 1, 1)],              # 4-byte but not 16-byte aligned, both alike: scalar head, vectors, scalar tail
    "head_and_tail_3": [(258, 3, 3), (6, 2, 2)],
    "scalar_throughout": [(4097, 1, 2)],          # avg and src at different offsets from a 16-byte boundary
    "shorter_than_head": [(2, 1, 1), (1, 3, 3)],
}
SINGLE = {f"n{n}": [(n, 0, 0)] for n in AC.SIZES + [AC.PAST_VECTOR_STRIDE]}


def build_ranges(layout, seed, maker):
    out = []
    for k, (n, sa, ss) in enumerate(layout):
        a, p = maker(n, seed + k)
        fa, va = guarded(a, sa)
        fp, vp_ = guarded(p, ss)
        out.append(dict(a=a, p=p, fa=fa, va=va, fp=fp, vp=vp_))
    return out


# ================================================================================================ vk_avg_update
@pytest.mark.parametrize("name", list(SINGLE) + list(LAYOUTS))
def test_update_equals_the_restatement_bit_for_bit(name):
    layout = {**SINGLE, **LAYOUTS}[name]
    rs = build_ranges(layout, 100, AC.rounded_pair)
    cnt = counter(4)
    scratch = avg_update([(r["va"], r["vp"]) for r in rs], rule(R.EMA, 0.9, True), cnt)
    torch.cuda.synchronize()
    assert cnt.item() == 5
    w = R.avg_weight(R.EMA, 0.9, True, 5)
    assert scratch[0].item() == 0.0 and scratch[1].item() == float(w)
    for r in rs:
        want, _ = R.avg_update(r["a"].numpy(), r["p"].numpy(), R.EMA, 0.9, True, 4)
        assert np.array_equal(AC.bits(r["va"]), AC.bits(want)), name
        assert same_bits(r["vp"], r["p"].to(dev()))                  # the source is only read
        assert guards_ok(r["fa"], r["va"]) and guards_ok(r["fp"], r["vp"])


def test_first_swa_sample_and_decay_zero_are_copies():
    for rl in (rule(R.SWA, 0.0), rule(R.EMA, 0.0)):
        rs = build_ranges([(4097, 1, 1)], 7, AC.rounded_pair)
        cnt = counter(0)
        avg_update([(rs[0]["va"], rs[0]["vp"])], rl, cnt)
        assert same_bits(rs[0]["va"], rs[0]["p"].to(dev())) and cnt.item() == 1


def test_exact_lattice_over_five_updates():
    n = 2 ** 20 + 3
    a = AC.lattice(n, 0)
    fa, va = guarded(a)
    a64 = a.double()
    cnt = counter(0)
    for k in range(1, AC.EXACT_UPDATES + 1):
        p = AC.lattice(n, k)
        fp, vp_ = guarded(p)
        avg_update([(va, vp_)], rule(R.EMA, AC.EXACT_DECAY), cnt)
        a64 = a64 + 0.25 * (p.double() - a64)
        assert torch.equal(va.double().cpu(), a64), k
    assert cnt.item() == AC.EXACT_UPDATES and guards_ok(fa, va)


@pytest.mark.parametrize("preset", AC.SWA_PRESETS)
def test_swa_is_exact_at_powers_of_two(preset):
    n = 4097
    a, p = AC.lattice(n, 10), AC.lattice(n, 11)
    fa, va = guarded(a, 1)
    fp, vp_ = guarded(p, 1)
    cnt = counter(preset)
    scratch = avg_update([(va, vp_)], rule(R.SWA, 0.0), cnt)
    t = preset + 1
    assert cnt.item() == t and scratch[1].item() == 1.0 / t
    assert torch.equal(va.double().cpu(), a.double() + (p.double() - a.double()) / t)
    assert guards_ok(fa, va)


@pytest.mark.parametrize("t", [1, 2, 10, 1000, AC.WARMUP_FIRST_FULL_DECAY - 1, AC.WARMUP_FIRST_FULL_DECAY])
def test_device_weight_equals_the_restatement(t):
    """The weight is formed in double on the device; the restatement forms it in Python doubles.  Same bits, warmup ramp and SWA."""
    a, p = torch.zeros(1), torch.ones(1)
    for kind, decay, warmup in [(R.EMA, AC.WARMUP_DECAY, True), (R.EMA, AC.WARMUP_DECAY, False), (R.SWA, 0.0, False)]:
        fa, va = guarded(a)
        fp, vp_ = guarded(p)
        cnt = counter(t - 1)
        scratch = avg_update([(va, vp_)], rule(kind, decay, warmup), cnt)
        w = R.avg_weight(kind, decay, warmup, t)
        assert cnt.item() == t and scratch[1].item() == float(w), (kind, warmup)
        assert va.item() == float(w)                             # 0 + w (1 - 0)


@pytest.mark.parametrize("flag", [1.0, -1.0, math.nan, 0.0, None])
def test_skip_rule(flag):
    rs = build_ranges(LAYOUTS["two"], 200, AC.rounded_pair)
    cnt = counter(6)
    scratch = avg_update([(r["va"], r["vp"]) for r in rs], rule(R.EMA, 0.9, True), cnt, scalar(flag))
    taken = flag is None or flag == 0.0
    assert cnt.item() == (7 if taken else 6)
    for r in rs:
        want, _ = R.avg_update(r["a"].numpy(), r["p"].numpy(), R.EMA, 0.9, True, 6, flag)
        assert np.array_equal(AC.bits(r["va"]), AC.bits(want))
        if not taken:
            assert same_bits(r["va"], r["a"].to(dev()))          # every byte of the average is unchanged
        assert guards_ok(r["fa"], r["va"])
    if not taken:
        assert scratch[0].item() == 1.0 and scratch[1].item() == SENTINEL


# ================================================================================================ vk_avg_swap
@pytest.mark.parametrize("name", list(SINGLE) + list(LAYOUTS))
def test_swap_exchanges_and_twice_is_the_identity(name):
    layout = {**SINGLE, **LAYOUTS}[name]
    rs = build_ranges(layout, 300, AC.rounded_pair)
    pairs = [(r["va"], r["vp"]) for r in rs]
    avg_swap(pairs)
    for r in rs:
        assert same_bits(r["va"], r["p"].to(dev())) and same_bits(r["vp"], r["a"].to(dev())), name
        assert guards_ok(r["fa"], r["va"]) and guards_ok(r["fp"], r["vp"])
    avg_swap(pairs)
    for r in rs:
        assert same_bits(r["va"], r["a"].to(dev())) and same_bits(r["vp"], r["p"].to(dev())), name
        assert guards_ok(r["fa"], r["va"]) and guards_ok(r["fp"], r["vp"])


# ================================================================================================ fused = separate, kernel level
def adamw_state(n, seed):
    g = torch.Generator().manual_seed(33000 + seed)
    s = dict(p=torch.randn(n, generator=g), m=torch.zeros(n), v=torch.zeros(n), a=torch.randn(n, generator=g),
             xa=torch.randn(259, generator=g), xs=torch.randn(259, generator=g))
    out = {k: guarded(t) for k, t in s.items()}
    out["steps"], out["count"] = counter(0), counter(0)
    out["s4"] = torch.full((4,), SENTINEL, dtype=torch.float32, device=dev())
    out["s2"] = torch.full((2,), SENTINEL, dtype=torch.float32, device=dev())
    return out


@pytest.mark.parametrize("n", AC.FUSED_SIZES)
@pytest.mark.parametrize("kind,warmup", [(R.EMA, True), (R.SWA, False)])
def test_fused_step_equals_step_then_update(n, kind, warmup):
    hp = TC.DEFAULT_HP
    A, B = adamw_state(n, n), adamw_state(n, n)
    rl = rule(kind, 0.9 if kind == R.EMA else 0.0, warmup)
    lib = vk.lib()
    for step, flag in enumerate([0.0, 1.0, None]):              # the middle step is skipped by found_inf
        grad = TC.rounded_adamw_grad(n, step).to(dev())
        fi, gs = scalar(flag), scalar(1024.0)
        args = lambda S: (n, S["p"][1].data_ptr(), grad.data_ptr(), S["m"][1].data_ptr(), S["v"][1].data_ptr(), hp["lr"], hp["beta1"],
                          hp["beta2"], hp["eps"], hp["wd"], S["steps"].data_ptr(), 0.5, gs.data_ptr(), P_(fi), S["s4"].data_ptr(), None, 0)
        vk._lib.check(lib.vk_adamw_step_amp_avg(*args(A), A["a"][1].data_ptr(), A["count"].data_ptr(), rl, A["s2"].data_ptr(),
                                                A["xa"][1].data_ptr(), A["xs"][1].data_ptr(), 259, st()), "vk_adamw_step_amp_avg")
        vk._lib.check(lib.vk_adamw_step_amp(*args(B), st()), "vk_adamw_step_amp")
        avg_update([(B["a"][1], B["p"][1]), (B["xa"][1], B["xs"][1])], rl, B["count"], fi, B["s2"])
        for k in ("p", "m", "v", "a", "xa", "xs"):
            assert same_bits(A[k][1], B[k][1]) and torch.equal(A[k][1], B[k][1]), (step, k)
            assert guards_ok(*A[k])
        taken = sum(1 for f in [0.0, 1.0, None][:step + 1] if not f)
        assert A["steps"].item() == B["steps"].item() == taken and A["count"].item() == B["count"].item() == taken, step
    assert not same_bits(A["a"][1], adamw_state(n, n)["a"][1])   # the average did move


def test_fused_step_without_an_extra_range_and_with_a_16_bit_copy():
    n, hp = 4097, TC.DEFAULT_HP
    A, B = adamw_state(n, 1), adamw_state(n, 1)
    lowA = torch.zeros(n, dtype=torch.bfloat16, device=dev())
    lowB = torch.zeros_like(lowA)
    grad = TC.rounded_adamw_grad(n, 5).to(dev())
    rl = rule(R.EMA, 0.999, False)
    args = lambda S, low: (n, S["p"][1].data_ptr(), grad.data_ptr(), S["m"][1].data_ptr(), S["v"][1].data_ptr(), hp["lr"], hp["beta1"],
                           hp["beta2"], hp["eps"], hp["wd"], S["steps"].data_ptr(), 1.0, None, None, S["s4"].data_ptr(), low.data_ptr(),
                           L_.VK_BF16)
    vk._lib.check(vk.lib().vk_adamw_step_amp_avg(*args(A, lowA), A["a"][1].data_ptr(), A["count"].data_ptr(), rl, A["s2"].data_ptr(),
                                                 None, None, 0, st()), "vk_adamw_step_amp_avg")
    vk._lib.check(vk.lib().vk_adamw_step_amp(*args(B, lowB), st()), "vk_adamw_step_amp")
    avg_update([(B["a"][1], B["p"][1])], rl, B["count"], None, B["s2"])
    for k in ("p", "m", "v", "a", "xa"):
        assert same_bits(A[k][1], B[k][1]), k
    assert torch.equal(lowA.view(torch.int16), lowB.view(torch.int16)) and same_bits(A["xa"][1], adamw_state(n, 1)["xa"][1])


# ================================================================================================ whole models
def build(seed=21, cls=None, **kw):
    from oracle import unet_oracle as O
    O.set_seed(seed)
    if cls is None:
        return vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev()).train()
    return cls(encoder_weights=None, **kw).to(dev()).train()


def batch(step=0, n=2, s=64):
    from oracle import unet_oracle as O
    x, y = O.synthetic_batch(n, s, seed=500 + step)
    return x.to(dev()), y.to(dev())


def twin_of(m):
    t = build()
    t.load_state_dict(m.state_dict(), strict=True)
    return t


def configure(m, mode):
    """The optimizer of a whole-model case: the whole-buffer step, or one of the fallbacks (frozen encoder, two param groups)."""
    if mode == "frozen":
        for name, p in m.named_parameters():
            if name.startswith("encoder."):
                p.requires_grad_(False)
    if mode == "groups":
        return vk.adamw_for(m, lr=1e-3, groups=vk.finetune_groups(m, 1e-3, encoder_lr_scale=0.1))
    return vk.adamw_for(m, lr=1e-3)


def same_model(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


@pytest.mark.parametrize("mode", ["whole", "frozen", "groups"])
@pytest.mark.parametrize("kind", ["ema", "swa"])
def test_attached_step_equals_step_then_update(mode, kind):
    """Three steps at fp32, the middle one a forced GradScaler overflow: attached through vk.GradScaler.step, the twin by hand with the
    same flag."""
    make = (lambda m: vk.ModelEMA(m, decay=0.9, warmup=True)) if kind == "ema" else vk.SWA
    m = build()
    t = twin_of(m)
    opt_m, opt_t = configure(m, mode), configure(t, mode)
    avg_m, avg_t = make(m).attach(opt_m), make(t)
    scaler = vk.GradScaler("cuda", init_scale=2.0 ** 10)
    scaler.scale(torch.zeros((), device=dev()))                 # creates the scale tensor (the loss is scaled inside the engine)
    gs = scalar(2.0 ** 10)
    for step in range(3):
        x, y = batch(step)
        for model, opt in ((m, opt_m), (t, opt_t)):
            opt.zero_grad(set_to_none=True)
            model.loss_and_backward(x, y, grad_scale=2.0 ** 10)
            if step == 1:
                model.flat_grads[model._param_ranges[-1][0]] = math.inf      # the overflow, in a tensor every mode trains
        before = m.flat_params.clone()
        scaler.step(opt_m)
        scaler.update(new_scale=2.0 ** 10)
        fi = (~torch.isfinite(t.flat_grads).all()).float().reshape(1)
        opt_t.step(found_inf=fi, grad_scale=gs)
        avg_t.update(found_inf=fi)
        assert (step == 1) == torch.equal(m.flat_params, before)
        assert same_bits(m.flat_params, t.flat_params) and same_bits(m._flat["bufs"], t._flat["bufs"]), step
        assert same_bits(avg_m._params, avg_t._params) and same_bits(avg_m._bufs, avg_t._bufs), step
        assert avg_m.updates == avg_t.updates == opt_m.step_count == (step + 1 if step < 1 else step), step
    assert not same_bits(avg_m._params, m.flat_params) and not same_bits(avg_m._bufs, m._flat["bufs"])
    if mode == "frozen":                                         # frozen tensors' averages stay at their (unchanged) values
        off, numel = m._param_ranges[0]
        assert same_bits(avg_m._params[off:off + numel], m.flat_params[off:off + numel])
    avg_m.detach()
    assert opt_m._average is None and avg_m._optimizer is None
    avg_m.update()                                               # detached: update() is allowed again
    assert avg_m.updates == 3


def test_average_is_within_the_proved_bound_of_torch_lerp():
    decay = 0.9
    m = build()
    opt = vk.adamw_for(m, lr=1e-3)
    ema = vk.ModelEMA(m, decay=decay, warmup=False).attach(opt)
    snap = lambda: {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if v.dtype == torch.float32}
    start, after = snap(), []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        m.loss_and_backward(*batch(step))
        opt.step()
        after.append(snap())
    got = {k: v.cpu() for k, v in ema.state_dict().items()}
    assert len(start) == len(m.state_dict()) - m._flat["nbt"].numel()          # every tensor but num_batches_tracked
    worst = 0.0
    for k, a0 in start.items():
        ps = [s[k].reshape(-1) for s in after]
        _, bound = AC.ema_bound_steps(a0.reshape(-1), ps, decay)
        theirs = a0.reshape(-1).clone()
        for p in ps:
            theirs = torch.lerp(theirs, p, 1.0 - decay)
        diff = (got[k].reshape(-1).double() - theirs.double()).abs()
        assert bool((diff <= bound).all()), (k, diff.max().item(), bound.max().item())
        worst = max(worst, (diff / bound.clamp_min(1e-300)).max().item())
    print(f"largest |ours - torch.lerp| / bound over {len(start)} tensors: {worst:.3f}")
    assert any("running_mean" in k for k in start) and not torch.equal(got["encoder.bn1.running_mean"], start["encoder.bn1.running_mean"])


def perturbed_model_and_average(kind="ema"):
    """A model in eval mode whose average differs from it in parameters and statistics."""
    m = build()
    avg = vk.ModelEMA(m, decay=0.5) if kind == "ema" else vk.SWA(m)
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        m.flat_params.mul_(1.0 + 0.05 * torch.randn(m.flat_params.numel(), generator=g, device=dev()))
        m._flat["bufs"].mul_(1.25).add_(0.01)
    m.mark_weights_dirty()
    avg.update()
    m.flat_params.mul_(0.97)
    m.mark_weights_dirty()
    return m.eval(), avg


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_applied_swaps_the_weights_under_the_engines_caches(dtype):
    m, ema = perturbed_model_and_average()
    x = batch(9, n=1)[0]

    def fwd(model):
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            return model(x).clone()

    before, sd_before = fwd(m), {k: v.detach().clone() for k, v in m.state_dict().items()}
    fresh = build(seed=99)
    fresh.load_state_dict(ema.state_dict(), strict=True)
    want = fwd(fresh.eval())
    assert not torch.equal(want, before)
    nbt = m._flat["nbt"].clone()
    with ema.applied() as inside:
        assert inside is m
        assert torch.equal(fwd(m), want)
        assert torch.equal(m._flat["nbt"], nbt)                  # num_batches_tracked is left alone
        with pytest.raises(vk.VkError, match="applied"):
            ema.update()
        with pytest.raises(vk.VkError, match="re-entrant"):
            with ema.applied():
                pass
        with pytest.raises(vk.VkError, match="applied"):
            ema.copy_to()
    unchanged = lambda: all(same_bits(v, sd_before[k]) if v.dtype == torch.float32 else torch.equal(v, sd_before[k])
                            for k, v in m.state_dict().items())
    assert torch.equal(fwd(m), before) and unchanged()
    with pytest.raises(RuntimeError, match="body"):
        with ema.applied():
            assert torch.equal(fwd(m), want)
            raise RuntimeError("body")
    assert torch.equal(fwd(m), before) and unchanged()
    # attached: update() is refused, and so is a step inside applied()
    m.train()
    opt = vk.adamw_for(m, lr=1e-3)
    ema.attach(opt)
    with pytest.raises(vk.VkError, match="attached"):
        ema.update()
    opt.zero_grad(set_to_none=True)
    m.loss_and_backward(*batch(0))
    with ema.applied():
        with pytest.raises(vk.VkError, match="applied"):
            opt.step()
    with pytest.raises(vk.VkError, match="attached"):
        vk.SWA(m).attach(opt)
    # copy_to makes the average the model's weights for good
    ema.copy_to()
    assert same_bits(m.flat_params, ema._params) and same_bits(m._flat["bufs"], ema._bufs)
    assert torch.equal(fwd(m.eval()), want)


@pytest.mark.parametrize("kind", ["ema", "swa"])
def test_averaging_state_round_trip(kind):
    m, avg = perturbed_model_and_average(kind)
    if kind == "ema":
        avg.warmup = True
    buf = io.BytesIO()
    torch.save(avg.averaging_state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=True)
    assert set(sd) == {"kind", "decay", "warmup", "updates", "params", "bufs"} and sd["updates"] == 1 and sd["kind"] == kind
    other = vk.ModelEMA(m, decay=0.123) if kind == "ema" else vk.SWA(m)
    other.load_averaging_state_dict(sd)
    assert other.updates == 1 and other.decay == avg.decay and other.warmup == avg.warmup
    assert same_bits(other._params, avg._params) and same_bits(other._bufs, avg._bufs)
    avg.update()
    other.update()
    assert same_bits(other._params, avg._params) and same_bits(other._bufs, avg._bufs) and other.updates == avg.updates == 2
    wrong = vk.SWA(m) if kind == "ema" else vk.ModelEMA(m)
    with pytest.raises(vk.VkError, match="kind"):
        wrong.load_averaging_state_dict(sd)
    short = dict(sd, params=sd["params"][:-1])
    with pytest.raises(vk.VkError, match="elements"):
        other.load_averaging_state_dict(short)


def test_device_and_size_mismatches_raise_at_update():
    m = build()
    ema = vk.ModelEMA(m)
    ema._params = ema._params[:-4].clone()
    with pytest.raises(vk.VkError, match="elements"):
        ema.update()
    ema = vk.ModelEMA(m)
    ema.to("cpu")
    with pytest.raises(vk.VkError, match="move it too"):
        ema.update()
    ema.to(dev())
    ema.update()
    assert ema.updates == 1 and ema.device == m.flat_params.device


@pytest.mark.parametrize("which", ["multiclass", "resnet18"])
def test_other_model_classes(which):
    if which == "multiclass":
        make = lambda seed: build(seed, vk.multiclass.Unet, classes=3)
    else:
        make = lambda seed: build(seed, vk.encoders.Unet, encoder_name="resnet18")
    m = make(3)
    ema = vk.ModelEMA(m, decay=0.5)
    with torch.no_grad():
        m.flat_params.mul_(1.5)
    ema.update()
    assert ema.updates == 1
    sd = ema.state_dict()
    assert list(sd) == list(m.state_dict())
    fresh = make(4)
    fresh.load_state_dict(sd, strict=True)
    assert same_bits(fresh.flat_params, ema._params) and same_bits(fresh._flat["bufs"], ema._bufs)
    # the restatement, from the copy the average started as (the same seed builds the same model)
    start = make(3).flat_params
    assert same_bits(ema._params.cpu(), torch.from_numpy(R.avg_elem(start.cpu().numpy(), m.flat_params.cpu().numpy(), np.float32(0.5))))
