"""Backward through frozen BatchNorm statistics on the MI355X: eval-mode and mixed-mode gradients against plain torch.nn autograd (the
oracle), the running buffers of eval-mode layers left alone, launch pruning with frozen statistics and weights, and the unchanged
all-train path.  The oracle's running statistics are populated by three train-mode forwards first (at init, running_mean = 0 and
running_var = 1 barely normalise, and the eval-mode activations could then grow layer after layer); the engine loads the oracle's state
dict, buffers included."""
import contextlib
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
N, S = 2, 64


def dev():
    return torch.device("cuda:0")


def _O():
    from oracle import unet_oracle as O
    return O


def warm_oracle(seed=5):
    O = _O()
    O.set_seed(seed)
    ref = O.build_model().train()
    with torch.no_grad():
        for k in range(3):
            ref(O.synthetic_batch(N, S, seed=700 + k)[0])
    return ref


def engine_from(ref):
    m = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev())
    m.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    return m


def set_modes(m, mode):
    if mode == "eval":
        m.eval()
    elif mode == "mixed":
        m.train()
        m.encoder.eval()
    else:
        m.train()
    return m


def oracle_grads(ref, x, y, dtype, mode, amp=None):
    """Gradients of BCE+Dice of a copy of the oracle in `dtype` (modes as given); returns ({name: grad}, copy)."""
    import copy
    O = _O()
    r = set_modes(copy.deepcopy(ref).to(dtype), mode)
    r.zero_grad(set_to_none=True)
    ctx = torch.autocast("cpu", dtype=amp) if amp is not None else contextlib.nullcontext()
    with ctx:
        lo = r(x.to(dtype))
    loss = O.total_loss(lo.to(dtype), y.to(dtype))
    loss.backward()
    return {n: p.grad.detach().double() for n, p in r.named_parameters() if p.grad is not None}, r


def engine_grads(m, x, y, amp=None):
    O = _O()
    m.zero_grad(set_to_none=True)
    ctx = torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()
    with ctx:
        lg = m(x.to(dev()))
    loss = O.total_loss(lg.float(), y.to(dev()))
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}, lg.detach().float()


def rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def buffers(m):
    return {n: b.detach().cpu().clone() for n, b in m.named_buffers()}


@pytest.mark.parametrize("mode", ["eval", "mixed"])
def test_backward_vs_oracle_fp32(mode):
    """All 140 gradients against the oracle's autograd in the same modes, float64 copy as the arbiter.  Eval mode (no batch-statistics
    amplification): relative L2 to float64 <= max(1e-3, 3 x the fp32 oracle's own).  Mixed mode has train-mode BatchNorm layers in the
    decoder, whose backward amplifies fp32 round-off in any implementation: it takes the bar of the all-train path
    (test_model_gpu.py::test_train_gradients_fp32_n8_against_plain_oracle: <= 1.5 % from float64), with the median <= 1 %.  That bar
    was set after the first run on the MI355X, which measured on these weights: all-train (the unchanged path) max 0.52 % / median
    0.33 %, mixed max 0.81 % / median 0.63 %, eval max 0.068 % (the fp32 oracle: 0.18 %, 0.17 %, 0.010 %).
    Eval-mode buffers stay bit-unchanged; train-mode buffers move as the oracle's."""
    ref = warm_oracle()
    O = _O()
    x, y = O.synthetic_batch(N, S, seed=1234)
    g64, r64 = oracle_grads(ref, x, y, torch.float64, mode)
    g32, r32 = oracle_grads(ref, x, y, torch.float32, mode)
    m = set_modes(engine_from(ref), mode)
    before = buffers(m)
    ge, _ = engine_grads(m, x, y)
    assert sorted(ge) == sorted(g64) and len(ge) == 140
    errs = {n: (rel(ge[n], g64[n]), rel(g32[n], g64[n])) for n in g64}
    print(f"\n[{mode} fp32] worst engine {max(errs.items(), key=lambda kv: kv[1][0])}")
    if mode == "eval":
        bad = [(n, e, r) for n, (e, r) in errs.items() if not e <= max(1e-3, 3 * r)]
    else:
        bad = [(n, e, r) for n, (e, r) in errs.items() if not e <= 1.5e-2]
        assert sorted(e for e, _ in errs.values())[70] <= 1e-2
    assert not bad, (mode, bad)
    after = buffers(m)
    ref_bufs = dict(r32.named_buffers())
    for n, b in after.items():
        frozen = mode == "eval" or n.startswith("encoder.")
        if frozen:
            assert torch.equal(b, before[n]), n                       # running stats and num_batches_tracked untouched
        elif n.endswith("num_batches_tracked"):
            assert b.item() == before[n].item() + 1, n
        else:
            assert torch.allclose(b, ref_bufs[n].float(), rtol=1e-4, atol=1e-5), (n, (b - ref_bufs[n]).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_eval_backward_16bit_vs_yardstick(dtype):
    """16-bit eval-mode backward under autocast against the fp64 oracle; yardstick: the oracle under CPU autocast in the same dtype.
    Bar per tensor: relative L2 <= 1.5 x the yardstick's + 0.02 (floor: the 16-bit storage of every activation and gradient tensor
    of the engine, where CPU autocast keeps the BatchNorm / ReLU / loss chain in fp32)."""
    ref = warm_oracle()
    O = _O()
    x, y = O.synthetic_batch(N, S, seed=1234)
    g64, _ = oracle_grads(ref, x, y, torch.float64, "eval")
    gy, _ = oracle_grads(ref, x, y, torch.float32, "eval", amp=dtype)
    m = set_modes(engine_from(ref), "eval")
    before = buffers(m)
    ge, lg = engine_grads(m, x, y, amp=dtype)
    assert torch.isfinite(lg).all()
    bad = []
    for n in g64:
        e_eng, e_y = rel(ge[n], g64[n]), rel(gy[n], g64[n])
        if not e_eng <= 1.5 * e_y + 0.02:
            bad.append((n, e_eng, e_y))
    assert not bad, bad
    after = buffers(m)
    assert all(torch.equal(after[n], before[n]) for n in before)


def _families(fn):
    L = vk.lib()
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.vk_prof_enable(0)
    return vk._lib.prof_collect()


def _bwd_families(m, x, y):
    O = _O()
    fam = None
    for _ in range(2):                  # the second backward runs with the batched weight-gradient tables built
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lg = m(x)
        loss = O.total_loss(lg.float(), y)
        fam = _families(lambda: loss.backward())
    return fam


def test_frozen_encoder_weights_and_statistics_launch_nothing_of_the_encoder():
    """Encoder frozen in weights (requires_grad_(False)) and statistics (eval()): the backward launches exactly what the weights-only
    freeze launches (the encoder's BatchNorm modes add no reduction and no kernel) and nothing of the stem / encoder families."""
    ref = warm_oracle()
    O = _O()
    x, y = (t.to(dev()) for t in O.synthetic_batch(4, 128, seed=31))
    fams = {}
    for stats_frozen in (False, True):
        m = engine_from(ref).train()
        m.encoder.requires_grad_(False)
        if stats_frozen:
            m.encoder.eval()
        fams[stats_frozen] = _bwd_families(m, x, y)
    bad = [t for t in fams[True] if any(k in t for k in ("maxpool_bwd", "stem", "s2dg", "igemm", "_s2", "coeffs_frozen"))]
    assert not bad, sorted(fams[True])
    assert {k: v["n"] for k, v in fams[True].items()} == {k: v["n"] for k, v in fams[False].items()}


def _step(m, x, y, path):
    O = _O()
    m.zero_grad(set_to_none=True)
    if path == "fused":
        loss = m.loss_and_backward(x, y, dtype=torch.float32)[0]
        lg = m.last_logits
    else:
        lg = m(x)
        loss = O.total_loss(lg, y)
        loss.backward()
    torch.cuda.synchronize()
    return (lg.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()},
            m._flat["bufs"].clone(), m._flat["nbt"].clone())


@pytest.mark.parametrize("path", ["autograd", "fused"])
def test_eval_then_train_holders_equal_fresh_model(path):
    """Holders that went eval() -> train() give the same logits, loss, gradients and buffers, to the bit, as a fresh model, with the same
    launch families (the all-train path is the unchanged schedule)."""
    ref = warm_oracle()
    O = _O()
    x, y = (t.to(dev()) for t in O.synthetic_batch(N, S, seed=77))
    fresh = engine_from(ref).train()
    flipped = engine_from(ref)
    flipped.eval()
    with torch.no_grad():
        flipped(x)
    set_modes(flipped, "mixed")
    flipped.zero_grad(set_to_none=True)
    O.total_loss(flipped(x), y).backward()                 # one grad-mode mixed step, then back to train mode on fresh buffers
    flipped.load_state_dict(fresh.state_dict())
    flipped.train()
    out, fam = {}, {}
    for name, m in (("fresh", fresh), ("flipped", flipped)):
        fam[name] = _families(lambda: out.__setitem__(name, _step(m, x, y, path)))
    a, b = out["fresh"], out["flipped"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][n], b[2][n]) for n in a[2])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert {k: v["n"] for k, v in fam["fresh"].items()} == {k: v["n"] for k, v in fam["flipped"].items()}


def test_no_grad_eval_forward_unchanged_by_grad_mode_eval_forward():
    ref = warm_oracle()
    O = _O()
    x, y = (t.to(dev()) for t in O.synthetic_batch(N, S, seed=78))
    m = engine_from(ref).eval()
    with torch.no_grad():
        a = m(x).clone()
    bufs = m._flat["bufs"].clone()
    lg = m(x)
    assert lg.requires_grad
    O.total_loss(lg, y).backward()
    with torch.no_grad():
        b = m(x).clone()
    assert torch.equal(a, b)
    assert torch.equal(bufs, m._flat["bufs"])


@pytest.mark.parametrize("mode", ["eval", "mixed"])
def test_loss_and_backward_equals_autograd_path(mode):
    """The fused step follows the same per-layer modes.  The two paths take dlogits from two loss implementations (the engine's loss
    kernel, torch's BCE + Dice) whose fp32 roundings differ, so the bar is relative L2 <= 1e-5 per tensor, not bit equality."""
    ref = warm_oracle()
    O = _O()
    x, y = (t.to(dev()) for t in O.synthetic_batch(N, S, seed=79))
    outs = []
    for path in ("autograd", "fused"):
        m = set_modes(engine_from(ref), mode)
        outs.append(_step(m, x, y, path))
    (la, sa, ga, ba, na), (lf, sf, gf, bf, nf) = outs
    assert torch.equal(la, lf)
    assert abs(sa.item() - sf.item()) <= 1e-6 * max(1.0, abs(sa.item()))
    for n in ga:
        assert rel(gf[n].double(), ga[n].double()) <= 1e-5, n
    assert torch.equal(ba, bf) and torch.equal(na, nf)
