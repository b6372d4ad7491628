"""Engine state sweep on the MI355X (-m gpu): every call on a model with a past equals the same call on a fresh model with the same
state, bit for bit (tests/history_cases.py holds the histories, the probes and the harness).  Then the negative control — a raw write
of the parameters without mark_weights_dirty() IS seen, as a stale weight pack — and the graphs whose plan has moved on: a backward
through a forward that another forward of the same plan displaced raises VkError before it writes anything; graphs of different
shapes, and a second backward over a retained graph, equal the twin's.

(The file name sorts behind every older GPU file, like test_vk_*_gpu.py before it: the older tests keep their positions in the
collection order.)"""
import importlib

import pytest
import torch

import encoders_ref
import history_cases as K

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")

_WARM = {}


def warm(family):
    if family.name not in _WARM:
        _WARM[family.name] = K.warm_state(vk, family)
    return _WARM[family.name]


def veteran_of(family=K.FAMILIES["resnet34"]):
    m = K.new_model(vk, family, init=False)
    m.load_state_dict(warm(family), strict=True)
    return K.Side(vk, family, m.train(), warm(family))


class OracleCheck:
    """Once per family: the twin's fp32 eval logits against the CPU oracle with the twin's state, at the suite's 1e-3 — equality of
    veteran and twin says nothing if both are wrong the same way."""

    def __init__(self, family):
        self.family, self.err = family, None

    def __call__(self, twin, x, logits):
        if self.err is not None:
            return
        ref = encoders_ref.build(dict(self.family.kwargs)["encoder_name"], self.family.classes)
        ref.load_state_dict({k: v.detach().cpu() for k, v in twin.model.state_dict().items()}, strict=True)
        ref.eval()
        with torch.no_grad():
            lo = ref(x)
        self.err = (lo - logits.cpu()).abs().max().item()
        print("[%s] twin fp32 eval logits against the oracle: max|err| = %.3e (max|logit| %.3f)" % (self.family.name, self.err, lo.abs().max().item()))
        assert self.err < 1e-3, self.err


@pytest.mark.parametrize("family,history", K.cases(), ids=["%s-%s" % (f, h.replace(" ", "_").replace(",", "")) for f, h in K.cases()])
def test_history(family, history, monkeypatch):
    fam = K.FAMILIES[family]
    oracle = OracleCheck(fam) if history == "plans interleaved" else None
    veteran, report = K.run_history(vk, fam, history, warm(fam), monkeypatch, oracle)
    assert report.probes == sum(len(e[1]) for e in K.HISTORIES[history].entries if e[0] == "probe")
    if history == "plans interleaved":
        assert oracle.err is not None
        plans = veteran.model._plans
        # the collisions the tables set up: A/bf16 and A/f32 in eval mode ran on the training plans, B only ever on eval plans
        assert "eval A/bf16" in report.mirrored and "eval A/f32" in report.mirrored
        assert "eval B/f16" not in report.mirrored and "eval B/f32" not in report.mirrored
        for dt in (torch.float16, torch.float32):
            assert (1, (96, 64), dt, False) in plans and (1, (96, 64), dt, True) not in plans
        for dt in (torch.bfloat16, torch.float32):
            assert (2, 64, dt, True) in plans and (2, 64, dt, False) not in plans


# ---------------------------------------------------------------------------------------------- negative control
def test_harness_sees_a_stale_weight_pack():
    """vk_adamw_step on flat_params.data_ptr() at the reference's lr (5e-5), as FusedAdamW launches it, but without
    mark_weights_dirty(): the bf16 plan keeps its packs of the old weights and differs from the twin, which packs the new ones.  After
    mark_weights_dirty() — the contract its docstring states — the veteran equals a twin again."""
    v = veteran_of()
    m = v.model
    step = K.fused_step(K.A, K.BF16)
    v.run(step, ("control", 0))                       # the plan exists, its packs hold the warm weights, the gradients are there
    p, g = m.flat_params, m.flat_grads
    mom, var, old = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    vk._lib.check(vk.lib().vk_adamw_step(p.numel(), p.data_ptr(), g.data_ptr(), mom.data_ptr(), var.data_ptr(), 5e-5, 0.9, 0.999, 1e-8,
                                         1e-4, 1, 1.0, None, None, vk._lib.VK_F32, vk._lib.current_stream()), "vk_adamw_step")
    torch.cuda.synchronize()
    assert not torch.equal(p, old) and (p - old).abs().max().item() <= 1.01 * 5e-5 * (1.0 + 1e-4 * old.abs().max().item())
    t = K.twin(v)
    v.run(step, ("control", 1))
    t.run(step, ("control", 1))
    ov, ot = v.observe(), t.observe()
    K.assert_finite(ov, "stale veteran")
    K.assert_finite(ot, "twin")
    assert not torch.equal(ov["logits"], ot["logits"]), "a pack one optimizer step stale went unseen"
    assert not torch.equal(ov["flat_grads"], ot["flat_grads"])
    m.mark_weights_dirty()
    t = K.twin(v)
    v.run(step, ("control", 2))
    t.run(step, ("control", 2))
    K.assert_equal(v.observe(), t.observe(), "after mark_weights_dirty()")


# ---------------------------------------------------------------------------------------------- a graph whose plan has moved on
def _x(key, shape=K.A):
    x, y = K.draw_inputs(key, shape, 1, "default")
    return x.to(K.device()), y.to(K.device())


def _grad_state(model):
    torch.cuda.synchronize()
    g = model._flat["grads"]
    return (None if g is None else g.clone()), [None if p.grad is None else p.grad.clone() for p in model.parameters()]


def _assert_grad_state_unchanged(model, before):
    flat, grads = _grad_state(model)
    assert (flat is None) == (before[0] is None) and (flat is None or torch.equal(flat, before[0]))
    for a, b in zip(grads, before[1]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def _with_a_past():
    """a veteran that has trained at A and C in bf16 and fp32, and its gradients as the last step left them"""
    v = veteran_of()
    for i, op in enumerate((K.fused_step(K.A, K.BF16), K.fused_step(K.C, K.F32), K.fused_step(K.A, K.F32))):
        v.run(op, ("past", i))
    return v


def test_two_forwards_of_one_shape_then_one_backward():
    """a = m(x1); b = m(x2); (a.sum() + b.sum()).backward(): the plan holds the activations of x2 only.  Autograd runs the node of b
    first (the later forward), which is valid and writes b's gradients; the node of a then raises before it writes anything — so what
    the buffer holds is exactly what a twin gets from b alone, never a sum with a's head pushed through b's activations."""
    v = _with_a_past()
    t = K.twin(v)
    (x1, _), (x2, _) = _x("two-1"), _x("two-2")
    for s in (v, t):
        s.model.zero_grad(set_to_none=True)
    a, b = v.model(x1), v.model(x2)
    with pytest.raises(vk.VkError, match="has since run a forward with a graph") as ei:
        (a.sum() + b.sum()).backward()
    assert "before the next forward of that shape" in str(ei.value) and "1 forward(s) later" in str(ei.value)
    t.model(x1)
    t.model(x2).sum().backward()
    got, want = _grad_state(v.model), _grad_state(t.model)
    assert torch.equal(got[0], want[0]) and torch.isfinite(got[0]).all() and got[0].abs().max().item() > 0
    assert [g is None for g in got[1]] == [g is None for g in want[1]]
    # the model is usable again at once: the next forward / backward pair of that shape equals the twin's
    for s in (v, t):
        s.run(K.autograd_step(K.A, K.F32), ("two", "after"))
    K.assert_equal(v.observe(), t.observe(), "the step after the refused backward")


@pytest.mark.parametrize("between", ["no_grad eval forward", "loss_and_backward"])
def test_backward_after_the_plan_ran_another_forward(between):
    """lg = m(x); then a torch.no_grad() eval forward of that shape (the training plan serves it: it rewrites the folded BatchNorm
    arena and every z) or loss_and_backward; then lg.sum().backward(): VkError, and flat_grads and every .grad keep what they held."""
    v = _with_a_past()
    t = K.twin(v)
    (x, _), (x2, y2) = _x("moved-1"), _x("moved-2")
    if between == "loss_and_backward":          # (the eval forward keeps the past's gradients: there they are what must not change)
        v.model.zero_grad(set_to_none=True)
    lg = v.model(x)
    t.model(x)
    if between == "loss_and_backward":
        v.model.loss_and_backward(x2, y2)
        t.model.loss_and_backward(x2, y2)
        said = "has since run loss_and_backward"
    else:
        with v.eval_mode(), torch.no_grad():
            v.model(x2)
        said = "has since run a forward without a graph"
    before = _grad_state(v.model)
    assert before[0] is not None and any(g is not None for g in before[1])
    with pytest.raises(vk.VkError, match=said) as ei:
        lg.sum().backward()
    assert "before the next forward of that shape" in str(ei.value)
    _assert_grad_state_unchanged(v.model, before)
    if between == "loss_and_backward":          # the displacing call itself did what it does on a model without the dangling graph
        assert torch.equal(before[0], _grad_state(t.model)[0])
        v.logits = v.loss = None                # (of the steps of the past)
        K.assert_equal(v.observe(), t.observe(), "loss_and_backward between a forward and its backward")


@pytest.mark.parametrize("dtype", [K.F32, K.BF16])
def test_graphs_of_different_shapes_share_one_backward(dtype):
    """a = m(xA); b = m(xC); one backward over both: two plans, each with its own activations — supported, and bit-equal to the twin
    evaluating the same expression"""
    v = _with_a_past()
    t = K.twin(v)
    (xa, _), (xc, _) = _x("shapes-A", K.A), _x("shapes-C", K.C)
    obs = []
    for s in (v, t):
        s.model.zero_grad(set_to_none=True)
        with K._autocast(dtype):
            a, b = s.model(xa), s.model(xc)
        (a.sum() + 0.5 * b.square().sum()).backward()
        s.logits, s.loss = a.detach(), b.detach().flatten()[:8]
        obs.append(s.observe())
    K.assert_equal(obs[0], obs[1], "two shapes, one backward (%s)" % dtype)
    assert obs[0]["flat_grads"].abs().max().item() > 0


@pytest.mark.parametrize("dtype", [K.F32, K.BF16, K.F16])
def test_second_backward_over_a_retained_graph(dtype):
    """loss.backward(retain_graph=True); loss.backward().  No kernel of the backward overwrites what a second pass reads: the
    activation gradients (g, gout) are rewritten from dlogits on, the BatchNorm-backward sums are zeroed by stage 0, the one-pass
    kernels never store dz, vk_bn_bwd_coeffs_frozen rewrites (a, 0, 0) with the forward's value — so the second backward must leave
    flat_grads bit-equal to a twin that ran forward, backward, forward with the same x, backward without zeroing."""
    v = _with_a_past()
    t = K.twin(v)
    x, y = _x("retain")
    bce = torch.nn.BCEWithLogitsLoss()
    scale = 1024.0 if dtype == K.F16 else 1.0
    v.model.zero_grad(set_to_none=True)
    with K._autocast(dtype):
        lg = v.model(x)
    loss = (bce(lg, y) + vk.DiceLoss(mode="binary")(lg, y)) * scale
    loss.backward(retain_graph=True)
    once = _grad_state(v.model)[0]
    loss.backward()
    t.model.zero_grad(set_to_none=True)
    for _ in range(2):
        with K._autocast(dtype):
            lt = t.model(x)
        ((bce(lt, y) + vk.DiceLoss(mode="binary")(lt, y)) * scale).backward()
    got, want = _grad_state(v.model)[0], _grad_state(t.model)[0]
    assert torch.isfinite(got).all() and once.abs().max().item() > 0 and not torch.equal(got, once)
    d = K.first_difference(got, want)
    assert d is None, "second backward over a retained graph (%s): flat_grads differ: %s" % (dtype, d)
