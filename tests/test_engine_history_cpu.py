"""The tables of tests/history_cases.py, without a GPU: every operation is known and well formed, every shape is one the network takes,
every history ends in a probe, and the declared matrix (what a history did x what probes it afterwards) has no empty required cell —
so that an edit of the tables cannot drop coverage without a test saying so."""
import pytest

import history_cases as K


def _ops():
    for h in K.HISTORIES.values():
        for e in h.entries:
            if e[0] not in K.MARKERS:
                yield "history %r" % h.name, e
    for name, ops in K.PROBES.items():
        for e in ops:
            yield "probe %r" % name, e


def test_every_operation_is_known_and_well_formed():
    for where, e in _ops():
        assert e[0] in K.OP_NAMES, (where, e)
        if e[0] in ("eval_fwd", "eval_fwd_grad", "autograd_step", "fused_step"):
            assert e[1] in (K.A, K.B, K.C) and e[2] in K.DTYPES, (where, e)
        if e[0] in ("autograd_step", "fused_step"):
            assert isinstance(e[-1], bool), (where, e)
        if e[0] == "fused_step":
            assert e[3] in K.ROUTES + ("{r}",), (where, e)
        if e[0] == "opt_step":
            assert e[1] in K.OPT_KINDS, (where, e)
        if e[0] == "bn_mode":
            assert e[2] in ("train", "eval"), (where, e)
    for f in K.FAMILIES.values():
        assert f.route in K.ROUTES
    # a probe never changes flags or state by another road than a step or an optimizer: what follows it must see the history's state
    for name, ops in K.PROBES.items():
        assert ops and all(e[0] in ("eval_fwd", "eval_fwd_grad", "autograd_step", "fused_step", "opt_step") for e in ops), name


def test_every_shape_is_a_multiple_of_32():
    seen = set()
    for where, e in _ops():
        if e[0] in ("eval_fwd", "eval_fwd_grad", "autograd_step", "fused_step"):
            N, H, W = e[1]
            assert N >= 1 and H % 32 == 0 and W % 32 == 0 and H >= 64 and W >= 64, (where, e)
            seen.add(e[1])
    assert seen == {K.A, K.B, K.C}
    assert K.B[1] != K.B[2], "B is there for the (height, width) plan key"
    assert K.A[1:] == K.C[1:] and K.A[0] != K.C[0], "A and C differ in the batch size alone"


def test_every_history_ends_in_a_probe_and_names_known_probes():
    for h in K.HISTORIES.values():
        assert h.entries[-1][0] == "probe" and h.entries[-1][1], h.name
        assert h.entries[0][0] not in K.MARKERS, h.name
        for e in h.entries:
            if e[0] in K.MARKERS:
                assert e[1] and all(n in K.PROBES for n in e[1]), (h.name, e)
        # a probe that must differ from a baseline has one, taken since the last probe marker
        have = set()
        for e in h.entries:
            if e[0] == "baseline":
                have |= set(e[1])
            elif e[0] == "probe":
                if e[2]:
                    assert set(e[1]) <= have, (h.name, e)
                have = set()
        assert h.families and all(f in K.FAMILIES for f in h.families), h.name


def test_families():
    full = [f.name for f in K.FAMILIES.values() if f.full]
    assert full == ["resnet34"]
    for h in K.HISTORIES.values():
        if h.name in ("plans interleaved", "weights change"):
            assert set(h.families) == set(K.FAMILIES), h.name
        elif h.name != "loss routes, 3 classes":
            assert h.families == ("resnet34",), h.name
    assert K.HISTORIES["loss routes, 3 classes"].families == ("multiclass3",)
    assert len(K.cases()) == len(set(K.cases())) == sum(len(h.families) for h in K.HISTORIES.values())


def test_key_collisions_are_there_on_purpose():
    """A/bf16 as a training plan and then in eval mode (one plan serves both); B/f16 in eval mode only (a small eval plan: the fused
    decoder tail and the split reduction are on)"""
    e = K.HISTORIES["plans interleaved"].entries
    t = K.transitions_of(e)
    assert t[e.index(K.eval_fwd(K.A, K.BF16))] == {"eval_on_train_plan"}
    assert t[e.index(K.eval_fwd(K.A, K.F32))] == {"eval_on_train_plan"}
    assert t[e.index(K.eval_fwd(K.B, K.F16))] == {"eval_plan"} and t[e.index(K.eval_fwd(K.B, K.F32))] == {"eval_plan"}
    every = [op for h in K.HISTORIES.values() for op in h.entries] + [op for ops in K.PROBES.values() for op in ops]
    assert not any(op[0] in ("autograd_step", "fused_step", "eval_fwd_grad") and op[1] == K.B for op in every)
    assert {op[2] for op in every if op[0] in ("eval_fwd", "fused_step")} == set(K.DTYPES)


def test_weights_change_covers_every_kind_of_write():
    e = K.HISTORIES["weights change"].entries
    writes = [op for op in e if op[0] in ("opt_step", "load_state", "mul_weights")]
    assert [w[:2] for w in writes] == [("opt_step", "fused"), ("opt_step", "stock"), ("opt_step", "groups"), ("load_state", 7), ("mul_weights",)]
    for w in writes:
        i = e.index(w)
        assert e[i - 1][0] == "baseline" and e[i + 1][0] == "probe" and e[i + 1][2], w
        assert set(e[i - 1][1]) == set(e[i + 1][1]) == {K.TRAIN_A16, K.TRAIN_A32, K.EVAL_B16, K.EVAL_B32}, w
        # the eval probes come last before the write and first after it: nothing but the write lies between their two runs
        assert e[i - 1][1][-2:] == K.FOUR_PLANS_EVAL and e[i + 1][1][:2] == K.FOUR_PLANS_EVAL, w


def test_coverage_matrix_has_no_empty_required_cell():
    assert set(K.REQUIRED) == set(K.TRANSITIONS)
    cov = K.coverage()
    for t, need in K.REQUIRED.items():
        assert need and need <= set(K.PROBE_KINDS), t
        assert need <= cov[t], "transition %r is no longer followed by probes of kind %s" % (t, sorted(need - cov[t]))
    assert {k for name in K.PROBES for k in K.probe_kinds(name)} == set(K.PROBE_KINDS)
    used = {n for h in K.HISTORIES.values() for e in h.entries if e[0] in K.MARKERS for n in e[1]}
    assert used == set(K.PROBES), "unused probes: %s" % sorted(set(K.PROBES) - used)


@pytest.mark.parametrize("shape,route,classes", [(K.A, "default", 1), (K.B, "multiclass", 3), (K.C, "multilabel", 3)])
def test_inputs_are_seeded_and_valid(shape, route, classes):
    import torch
    x, y = K.draw_inputs(("h", 3), shape, classes, route)
    x2, y2 = K.draw_inputs(("h", 3), shape, classes, route)
    x3, _ = K.draw_inputs(("h", 4), shape, classes, route)
    assert torch.equal(x, x2) and torch.equal(y, y2) and not torch.equal(x, x3)
    N, H, W = shape
    assert x.shape == (N, 3, H, W) and x.dtype == torch.float32
    if route == "multiclass":
        assert y.dtype == torch.int64 and y.shape == (N, H, W) and 0 <= int(y.min()) and int(y.max()) < classes
    else:
        assert y.shape == (N, classes, H, W) and set(y.unique().tolist()) <= {0.0, 1.0}


def test_first_difference_names_the_element():
    import torch
    a = torch.arange(12.0).reshape(3, 4)
    b = a.clone()
    assert K.first_difference(a, b) is None and K.first_difference(None, None) is None
    b[1, 2] = -1.0
    assert K.first_difference(a, b).startswith("element 6 of 12 (1 differ): veteran 6.0, twin -1.0")
    assert K.first_difference(a, None) is not None and K.first_difference([True], [False]) is not None
    with pytest.raises(AssertionError, match="not finite"):
        K.assert_equal({"x": torch.tensor([float("nan")])}, {"x": torch.tensor([float("nan")])}, "here")
