"""Param groups and gradient clipping of FusedAdamW, the parts that need no GPU: the list-of-dicts constructor and its limits,
vk.finetune_groups, LR schedulers per group, the state dict with groups, the argument checks of vk_adamw_step_groups /
vk_grad_norm_segments and of clip_grad_norm_, and the exactness conditions of the norm's lattice cases (tests/param_groups_cases.py)."""
import copy
import ctypes as C
import math

import pytest
import torch

import param_groups_cases as PC


def _model(vk, enc="resnet34"):
    cls = vk.Unet if enc == "resnet34" else vk.encoders.Unet
    return cls(encoder_name=enc, encoder_weights=None, in_channels=3, classes=1, activation=None)


def test_list_of_dicts_builds_with_group_defaults(vk):
    """torch's param-group form (smp's examples: Adam([dict(params=model.parameters(), lr=1e-4)])): every group takes what it does not
    set from the constructor."""
    m = _model(vk)
    opt = vk.FusedAdamW([dict(params=m.parameters(), lr=1e-4)], weight_decay=1e-4).attach(m)
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 140
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-4, (0.9, 0.999), 1e-8, 1e-4)
    ps = list(m.parameters())
    opt = vk.FusedAdamW([dict(params=ps[:10], lr=1e-5), dict(params=ps[10:50], betas=(0.8, 0.99), eps=1e-6),
                         dict(params=ps[50:], weight_decay=0.0)], lr=1e-3, weight_decay=1e-2).attach(m)
    got = [(g["lr"], g["betas"], g["eps"], g["weight_decay"]) for g in opt.param_groups]
    assert got == [(1e-5, (0.9, 0.999), 1e-8, 1e-2), (1e-3, (0.8, 0.99), 1e-6, 1e-2), (1e-3, (0.9, 0.999), 1e-8, 0.0)]
    assert [t for t, _ in opt._owned] == list(range(140))
    assert [opt._group_of[t] for t in range(140)] == [0] * 10 + [1] * 40 + [2] * 90
    assert opt.tensor_steps() == [0] * 140
    # through adamw_for, and a subset of the model in two groups
    opt = vk.adamw_for(m, lr=1e-3, weight_decay=1e-4, groups=[dict(params=ps[100:], lr=1e-4), dict(params=ps[:20])])
    assert [t for t, _ in opt._owned] == list(range(20)) + list(range(100, 140))
    assert opt.param_groups[1]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 1e-4
    with pytest.raises(NotImplementedError):
        vk.FusedAdamW([dict(params=ps)], amsgrad=True)
    with pytest.raises(NotImplementedError):
        opt.step(closure=lambda: None)


def test_more_than_eight_groups_are_refused(vk):
    m = _model(vk)
    ps = list(m.parameters())
    eight = [dict(params=[p]) for p in ps[:8]]
    opt = vk.FusedAdamW(eight, lr=1e-3).attach(m)
    assert len(opt.param_groups) == PC.MAX_GROUPS == vk._lib.VK_ADAMW_MAX_GROUPS
    with pytest.raises(vk.VkError, match="VK_ADAMW_MAX_GROUPS = 8"):
        opt.add_param_group(dict(params=[ps[8]]))
    with pytest.raises(vk.VkError, match="VK_ADAMW_MAX_GROUPS = 8"):
        vk.FusedAdamW([dict(params=[p]) for p in ps[:9]], lr=1e-3)
    # add_param_group below the limit: the new tensors are owned, in the new group
    opt = vk.FusedAdamW([dict(params=ps[:5])], lr=1e-3).attach(m)
    opt.add_param_group(dict(params=ps[5:9], lr=1e-5))
    assert [t for t, _ in opt._owned] == list(range(9)) and opt._group_of[8] == 1 and opt._group_of[0] == 0


def test_a_parameter_of_another_model_fails_at_attach(vk):
    m, other = _model(vk), _model(vk)
    ps = list(m.parameters())
    with pytest.raises(vk.VkError):
        vk.FusedAdamW([dict(params=ps[:70]), dict(params=ps[70:] + [next(other.parameters())], lr=1e-5)], lr=1e-3).attach(m)
    opt = vk.FusedAdamW([dict(params=ps[:70])], lr=1e-3).attach(m)
    with pytest.raises(vk.VkError):
        opt.add_param_group(dict(params=[next(other.parameters())]))


@pytest.mark.parametrize("enc", ["resnet34", "resnet18", "resnet50"])
def test_finetune_groups_partition_every_tensor_once(vk, enc):
    m = _model(vk, enc)
    named = list(m.named_parameters())
    one_d = {id(p) for _, p in named if p.dim() == 1}
    enc_ids = {id(p) for n, p in named if n.startswith("encoder.")}
    if enc == "resnet34":
        assert len(named) == 140 and len(one_d) == 93 and len(named) - len(one_d) == 47
    groups = vk.finetune_groups(m, 1e-3, encoder_lr_scale=0.1, weight_decay=1e-4, decay_norm_and_bias=False)
    assert len(groups) == 4
    seen = [id(p) for g in groups for p in g["params"]]
    assert sorted(seen) == sorted(id(p) for _, p in named) and len(set(seen)) == len(seen)
    for g in groups:
        ids = {id(p) for p in g["params"]}
        assert ids <= enc_ids or not (ids & enc_ids)
        assert g["lr"] == (1e-3 * 0.1 if ids <= enc_ids else 1e-3)
        assert ids <= one_d or not (ids & one_d)
        assert g["weight_decay"] == (0.0 if ids <= one_d else 1e-4)
    assert sum(len(g["params"]) for g in groups if g["weight_decay"] == 0.0) == len(one_d)
    # default: everything decays, encoder and the rest
    groups = vk.finetune_groups(m, 1e-3)
    assert [len(g["params"]) for g in groups] == [len(enc_ids), len(named) - len(enc_ids)]
    assert all(g["weight_decay"] == 1e-4 and g["lr"] == 1e-3 for g in groups)
    # empty groups are dropped
    only = vk.finetune_groups(torch.nn.ModuleDict({"decoder": m.decoder}), 1e-3, decay_norm_and_bias=False)
    assert len(only) == 2
    opt = vk.adamw_for(m, lr=1e-3, groups=vk.finetune_groups(m, 1e-3, 0.1, 1e-4, False))
    assert len(opt.param_groups) == 4 and len(opt._owned) == len(named)


def test_schedulers_drive_each_group(vk):
    m = _model(vk)
    opt = vk.adamw_for(m, lr=1e-3, groups=vk.finetune_groups(m, 1e-3, encoder_lr_scale=0.1, decay_norm_and_bias=False))
    base = [g["lr"] for g in opt.param_groups]
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10)
    opt._opt_called = True                  # no device here: silence torch's "scheduler before optimizer.step()" warning
    for k in range(1, 6):
        sch.step()
        for g, b in zip(opt.param_groups, base):
            assert g["lr"] == pytest.approx(b * (1 + math.cos(math.pi * k / 10)) / 2, rel=1e-12)
    opt = vk.adamw_for(m, lr=1e-3, groups=vk.finetune_groups(m, 1e-3))
    sch = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.0 if e < 2 else 1.0, lambda e: 0.5 ** e])
    opt._opt_called = True
    for k in range(1, 4):
        sch.step()
        assert opt.param_groups[0]["lr"] == (0.0 if k < 2 else 1e-3)
        assert opt.param_groups[1]["lr"] == pytest.approx(1e-3 * 0.5 ** k, rel=1e-12)


def test_state_dict_round_trip_with_three_groups(vk):
    m = _model(vk)
    spec = PC.three_groups(vk, m, 1e-3)
    assert sorted(i for ids, _ in spec for i in ids) == list(range(140)) and len(spec[2][0]) == 93
    opt = vk.FusedAdamW(PC.as_param_groups(spec, m.parameters()), lr=1e-3).attach(m)
    opt.param_groups[0]["lr"] = 3e-5        # what a scheduler leaves behind
    n = m.flat_params.numel()
    sd = opt.state_dict()
    assert set(sd["fused"]) == {"step", "exp_avg", "exp_avg_sq"} and len(sd["param_groups"]) == 3
    steps = [0] * 110 + [3] * 30
    sd["fused"] = {"step": 3, "exp_avg": torch.arange(n, dtype=torch.float32), "exp_avg_sq": torch.ones(n), "steps": steps}
    opt2 = vk.FusedAdamW(PC.as_param_groups(spec, m.parameters()), lr=1e-3).attach(m)
    opt2.load_state_dict(copy.deepcopy(sd))
    assert [g["lr"] for g in opt2.param_groups] == [3e-5, 1e-3, 1e-3]
    assert [g["weight_decay"] for g in opt2.param_groups] == [1e-4, 1e-4, 0.0]
    assert opt2.tensor_steps() == steps and opt2.step_count == 3
    sd2 = opt2.state_dict()
    assert sd2["fused"]["steps"] == steps and torch.equal(sd2["fused"]["exp_avg"], sd["fused"]["exp_avg"])
    assert [g["params"] for g in sd2["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    assert [opt2._group_of[t] for t in range(140)] == [opt._group_of[t] for t in range(140)]
    # a state dict of another grouping is refused by torch's own check
    opt1 = vk.adamw_for(m, lr=1e-3)
    with pytest.raises(ValueError):
        opt1.load_state_dict(copy.deepcopy(sd))


def test_c_entry_points_refuse_bad_arguments_before_any_launch(vk):
    L = vk.lib()
    buf = (C.c_double * 64)()               # any non-null address: a refused call touches neither it nor a device
    a = C.addressof(buf)
    hp = (vk._lib.vk_adamw_group * 9)()

    def step(n_groups=1, groups=hp, **null):
        ptrs = {k: a for k in ("segments", "segment_group", "blocks", "param", "grad", "m", "v", "steps", "scratch")}
        ptrs.update({k: None for k in null})
        return L.vk_adamw_step_groups(1, ptrs["segments"], ptrs["segment_group"], 1, ptrs["blocks"], ptrs["param"], ptrs["grad"], ptrs["m"],
                                      ptrs["v"], n_groups, groups, ptrs["steps"], 1.0, None, None, None, ptrs["scratch"], None)

    for n_groups in (0, -1, 9, 100):
        assert step(n_groups) == -1 and b"groups" in L.vk_last_error_string()
    assert step(1, None) == -1
    for k in ("segments", "segment_group", "blocks", "param", "grad", "m", "v", "steps", "scratch"):
        assert step(1, hp, **{k: True}) == -1, k

    def norm(kind=0, max_norm=1.0, **null):
        ptrs = {k: a for k in ("segments", "blocks", "grad", "partials", "out")}
        ptrs.update({k: None for k in null})
        return L.vk_grad_norm_segments(1, ptrs["segments"], 1, ptrs["blocks"], ptrs["grad"], kind, 1.0, max_norm, ptrs["partials"],
                                       ptrs["out"], None)

    for kind in (-1, 2, 7):
        assert norm(kind) == -1 and b"norm kind" in L.vk_last_error_string()
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        assert norm(0, bad) == -1 and b"max_norm" in L.vk_last_error_string()
    for k in ("segments", "blocks", "grad", "partials", "out"):
        assert norm(0, 1.0, **{k: True}) == -1, k
    assert L.vk_grad_norm_segments(0, a, 1, a, a, 0, 1.0, 1.0, a, a, None) == -1
    assert L.vk_grad_norm_segments(1, a, 0, a, a, 0, 1.0, 1.0, a, a, None) == -1


def test_clip_grad_norm_argument_errors(vk):
    m = _model(vk)
    opt = vk.adamw_for(m, lr=1e-3)
    with pytest.raises(NotImplementedError):
        opt.clip_grad_norm_(1.0, norm_type=3)
    with pytest.raises(NotImplementedError):
        opt.clip_grad_norm_(1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError):
        opt.clip_grad_norm_(1.0, error_if_nonfinite=True)
    with pytest.raises(ValueError):
        opt.clip_grad_norm_(-1.0)
    with pytest.raises(ValueError):
        vk.clip_grad_norm_(opt, float("nan"), norm_type=float("inf"))
    for nt in (2, 2.0, float("inf"), math.inf):
        with pytest.raises(vk.VkError, match="no CPU fallback"):          # a CPU model: the arguments are fine, the device is not
            vk.clip_grad_norm_(opt, 1.0, norm_type=nt)
    with pytest.raises(vk.VkError):
        vk.FusedAdamW(m.parameters(), lr=1e-3).clip_grad_norm_(1.0)       # not attached


def test_lattice_sums_are_exact_in_double_in_any_order():
    """|g| <= 2047 and n = 2^20 + 3: the float64 sum of squares equals the integer sum, whatever the order, and is far below 2^53."""
    g = PC.lattice_grad(PC.LARGE, 5)
    assert g.abs().max().item() <= 2047 and bool((g == g.round()).all()) and bool((g != 0).all())
    want = PC.int_sum_squares(g)
    assert want < 2 ** 47 < 2 ** 53 and 2047 ** 2 * 2 ** 25 < 2 ** 47
    sq = g.double() * g.double()
    assert int(sq.sum().item()) == want
    perm = torch.randperm(PC.LARGE, generator=torch.Generator().manual_seed(1))
    assert int(sq[perm].sum().item()) == want
    assert int(sq[perm].cumsum(0)[-1].item()) == want                   # strictly sequential order
    assert PC.norm_ref([g], PC.NORM_L2) == math.sqrt(want) and PC.norm_ref([g], PC.NORM_L2, 0.5) == 0.5 * math.sqrt(want)
    for n, root in zip(PC.THREES_LENGTHS, (3, 6, 48, 192, 3072)):
        assert PC.norm_ref([PC.threes(n, n)], PC.NORM_L2) == root
        assert PC.norm_ref([PC.threes(n, n)], PC.NORM_INF, 0.5) == 1.5


def test_references_of_the_cases():
    assert PC.ulp32(1.0) == 2.0 ** -23 and PC.ulp32(1.5) == 2.0 ** -23 and PC.ulp32(2.0) == 2.0 ** -22 and PC.ulp32(0.0) == 2.0 ** -149
    assert PC.ulp32(3072.0) == 2.0 ** -12
    assert PC.coef_ref(2.0, 1.0) == 1.0 / (2.0 + 1e-6) and PC.coef_ref(0.5, 1.0) == 1.0 and PC.coef_ref(0.0, 1.0) == 1.0
    assert PC.coef_ref(5.0, 0.0) == 0.0 and PC.coef_ref(float("inf"), 1.0) == 0.0 and math.isnan(PC.coef_ref(float("nan"), 1.0))
    nan = torch.tensor([1.0, float("nan"), -3.0])
    assert math.isnan(PC.norm_ref([nan], PC.NORM_INF)) and math.isnan(PC.norm_ref([nan], PC.NORM_L2))
    assert PC.norm_ref([torch.tensor([1.0, -4.0]), torch.tensor([3.0])], PC.NORM_INF) == 4.0
    # the factor: one rounding of a product that is exact in double; identity without a coefficient
    assert PC.fused_factor(0.3) == PC.f32(0.3) and PC.fused_factor(0.3, None, 1.0) == PC.f32(0.3)
    assert PC.fused_factor(0.5, 1024.0, 0.125) == 2.0 ** -14
    prod = PC.f32(0.3) * PC.f32(0.37)
    assert float(torch.tensor(prod, dtype=torch.float64).float()) == PC.fused_factor(0.3, None, 0.37)
    ranges, total = PC.layout()
    assert len(ranges) == 10 and ranges[-1][1] - ranges[-1][0] == PC.LARGE and all(b % 4 for b, _ in ranges) and ranges[-1][1] <= total
    assert all(a[1] < b[0] for a, b in zip(ranges, ranges[1:]))
    assert len(PC.HP_SETS) == 8
    for k in ("lr", "beta1", "beta2", "eps", "wd"):
        assert len({h[k] for h in PC.HP_SETS}) == 8, k                  # the sets differ in every field
