"""Fine-tuning with frozen parameters on the MI355X: the pruned backward gives the full backward's gradients for the trainable tensors
and none for the frozen ones, really launches less, and the per-tensor AdamW (vk_adamw_step_amp_segments) matches torch.optim.AdamW,
GradScaler's skipped steps included.  Small shapes (4 x 128 x 128) so that every kernel family of the real step takes part."""
import contextlib
import copy
import ctypes as C
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")


def dev():
    return torch.device("cuda:0")


def build(seed=21):
    from oracle import unet_oracle as O
    O.set_seed(seed)
    return vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev()).train()


def batch(step=0, n=4, s=128):
    from oracle import unet_oracle as O
    x, y = O.synthetic_batch(n, s, seed=300 + step)
    return x.to(dev()), y.to(dev())


def names(m):
    return [n for n, _ in m.named_parameters()]


def _is_bn(name, p):
    return p.dim() == 1 and not name.startswith("segmentation_head.")


PATTERNS = {
    "encoder": lambda m: m.encoder.requires_grad_(False),
    "stem_layer1_layer2": lambda m: [m.get_submodule(s).requires_grad_(False)
                                     for s in ("encoder.conv1", "encoder.bn1", "encoder.layer1", "encoder.layer2")],
    "every_bn": lambda m: [p.requires_grad_(False) for n, p in m.named_parameters() if _is_bn(n, p)],
    "decoder_head": lambda m: (m.decoder.requires_grad_(False), m.segmentation_head.requires_grad_(False)),
    "one_tensor": lambda m: m.get_parameter("encoder.layer3.2.conv1.weight").requires_grad_(False),
}

_BCE = torch.nn.BCEWithLogitsLoss()
_DICE = vk.DiceLoss(mode="binary")


def run_backward(m, path, dtype, step=0):
    """One forward + BCE+Dice + backward; returns (loss, logits) as device tensors."""
    x, y = batch(step)
    if path == "fused":
        out = m.loss_and_backward(x, y, dtype=dtype)
        return out[0].clone(), m.last_logits.clone()
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else contextlib.nullcontext()
    with ctx:
        logits = m(x)
    logits = logits.float()
    loss = _BCE(logits, y) + _DICE(logits, y)
    loss.backward()
    return loss.detach().clone(), logits.detach().clone()


@pytest.mark.parametrize("path", ["autograd", "fused"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_frozen_gradients_match_full_backward(dtype, path):
    full = build()
    loss_f, logits_f = run_backward(full, path, dtype)
    torch.cuda.synchronize()
    grads_f = {n: p.grad.detach().clone() for n, p in full.named_parameters()}
    bufs_f, nbt_f = full._flat["bufs"].clone(), full._flat["nbt"].clone()
    for pat, freeze in PATTERNS.items():
        m = build()
        freeze(m)
        mask = m._trainable_mask()
        assert 0 < sum(mask) < 140, pat
        loss, logits = run_backward(m, path, dtype)
        torch.cuda.synchronize()
        assert torch.equal(loss, loss_f) and torch.equal(logits, logits_f), pat
        assert torch.equal(m._flat["bufs"], bufs_f) and torch.equal(m._flat["nbt"], nbt_f), pat
        flat = m.flat_grads
        for (name, p), (off, numel), t in zip(m.named_parameters(), m._param_ranges, mask):
            if not t:
                assert p.grad is None, (pat, name)
                assert not flat[off:off + numel].any(), (pat, name)        # the flat buffer stays exactly zero over frozen ranges
                continue
            g, gf = p.grad, grads_f[name]
            assert g is not None, (pat, name)
            if dtype == torch.float32:
                assert torch.equal(g, gf), (pat, name, (g - gf).abs().max().item())
            else:
                # the batched weight-gradient partition depends on which layers are in the batch: its fp32 sums may reorder
                bar = 1e-4 * gf.abs().max().item()
                assert (g - gf).abs().max().item() <= bar, (pat, name, (g - gf).abs().max().item(), bar)
        del m


def _families(fn):
    L = vk.lib()
    torch.cuda.synchronize()
    vk._lib.prof_collect()              # drop anything recorded before
    L.vk_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.vk_prof_enable(0)
    return vk._lib.prof_collect()


def test_frozen_encoder_prunes_launches():
    counts = {}
    for frozen in (False, True):
        m = build()
        if frozen:
            m.encoder.requires_grad_(False)
        x, y = batch()
        for _ in range(2):              # the second backward runs with the batched weight-gradient tables built
            m.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = m(x)
            loss = _BCE(logits.float(), y) + _DICE(logits.float(), y)
            fam = _families(lambda: loss.backward())
        counts[frozen] = fam
        if frozen:
            bad = [t for t in fam if any(k in t for k in ("maxpool_bwd", "stem", "s2dg", "igemm", "_s2"))]
            assert not bad, sorted(fam)
            # stages 3-9 (the encoder), called one at a time as the data-parallel reducer does: nothing is launched
            m.zero_grad(set_to_none=True)
            m.loss_and_backward(x, y, dtype=torch.bfloat16)
            plan = m.plan_for(4, 128, torch.bfloat16, True)
            L = vk.lib()

            def stages():
                for s in range(3, 10):
                    vk._lib.check(L.vk_unet_backward(plan.h, None, s, s + 1, vk._lib.current_stream()))
            assert _families(stages) == {}
    n_full = sum(v["n"] for v in counts[False].values())
    n_frozen = sum(v["n"] for v in counts[True].values())
    assert n_frozen < 0.5 * n_full, (n_frozen, n_full, sorted(counts[True]))


def _ref_copies(m):
    return [p.detach().clone().requires_grad_(True) for p in m.parameters()]


def _feed(ref, m, inv_scale=1.0):
    for r, p in zip(ref, m.parameters()):
        r.grad = None if p.grad is None else p.grad.detach().float() * inv_scale


def _resync(ref, m):
    """Each step is compared from the same parameters: the bar is one step's rounding, as in test_adamw_matches_torch."""
    with torch.no_grad():
        for r, p in zip(ref, m.parameters()):
            r.copy_(p)


def _schedule(m, opt, steps, ref=None, ref_opt=None, on_step=None):
    """Steps 0-1 with the encoder frozen, then unfrozen; checks against the torch reference when given."""
    for step in steps:
        m.encoder.requires_grad_(step >= 2)
        opt.zero_grad(set_to_none=True)
        m.loss_and_backward(*batch(step), dtype=torch.bfloat16)
        before = [p.detach().clone() for p in m.parameters()]
        opt.step()
        if ref is not None:
            _feed(ref, m)
            ref_opt.step()
            torch.cuda.synchronize()
            for (name, p), r, b in zip(m.named_parameters(), ref, before):
                assert (p.detach() - r.detach()).abs().max().item() <= 2e-7, (step, name)
                if not p.requires_grad:
                    assert torch.equal(p.detach(), b), (step, name)       # frozen: untouched
            _resync(ref, m)
        if on_step is not None:
            on_step(step)


def test_per_tensor_adamw_matches_torch_through_freeze_and_unfreeze():
    m = build()
    opt = vk.FusedAdamW(m.parameters(), lr=5e-5, weight_decay=1e-4).attach(m)
    ref = _ref_copies(m)
    ref_opt = torch.optim.AdamW(ref, lr=5e-5, weight_decay=1e-4, foreach=False)
    enc = [n.startswith("encoder.") for n in names(m)]

    def counts(step):
        want = [(step + 1) if not e else max(0, step - 1) for e in enc]
        assert opt.tensor_steps() == want, step
    _schedule(m, opt, range(4), ref, ref_opt, counts)
    # a state-dict round trip in the middle of the schedule continues with the same bits
    a, b = build(), build()
    opt_a = vk.FusedAdamW(a.parameters(), lr=5e-5, weight_decay=1e-4).attach(a)
    _schedule(a, opt_a, range(4))
    opt_b = vk.FusedAdamW(b.parameters(), lr=5e-5, weight_decay=1e-4).attach(b)
    _schedule(b, opt_b, range(2))
    sd = copy.deepcopy(opt_b.state_dict())
    assert "steps" in sd["fused"]
    opt_b2 = vk.FusedAdamW(b.parameters(), lr=5e-5, weight_decay=1e-4).attach(b)
    opt_b2.load_state_dict(sd)
    _schedule(b, opt_b2, range(2, 4))
    torch.cuda.synchronize()
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb), n
    assert opt_a.tensor_steps() == opt_b2.tensor_steps()
    # the one-counter format still loads (every tensor at "step") and steps on
    old = copy.deepcopy(opt_a.state_dict())
    del old["fused"]["steps"]
    opt_c = vk.FusedAdamW(a.parameters(), lr=5e-5, weight_decay=1e-4).attach(a)
    opt_c.load_state_dict(old)
    _schedule(a, opt_c, [4])
    assert opt_c.tensor_steps() == [5] * 140


def test_optimizer_over_trainable_subset_only():
    """FusedAdamW(p for p in m.parameters() if p.requires_grad): tensors outside the group never move, even with a gradient."""
    m = build()
    m.encoder.requires_grad_(False)
    opt = vk.FusedAdamW((p for p in m.parameters() if p.requires_grad), lr=5e-5, weight_decay=1e-4).attach(m)
    ref = _ref_copies(m)
    ref_opt = torch.optim.AdamW([r for r, p in zip(ref, m.parameters()) if p.requires_grad], lr=5e-5, weight_decay=1e-4,
                                foreach=False)
    m.encoder.requires_grad_(True)          # unfrozen after the optimizer was built: gradients, but not in the group
    enc0 = [p.detach().clone() for n, p in m.named_parameters() if n.startswith("encoder.")]
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        m.loss_and_backward(*batch(step), dtype=torch.bfloat16)
        opt.step()
        _feed(ref, m)
        ref_opt.step()
        torch.cuda.synchronize()
        for (n, p), r in zip(m.named_parameters(), ref):
            if not n.startswith("encoder."):
                assert (p.detach() - r.detach()).abs().max().item() <= 2e-7, (step, n)
        _resync(ref, m)
    enc1 = [p.detach() for n, p in m.named_parameters() if n.startswith("encoder.")]
    assert all(torch.equal(a, b) for a, b in zip(enc0, enc1))


@pytest.mark.parametrize("scaler_cls", ["vk", "torch"])
def test_amp_frozen_encoder_overflow_skips_without_counting(scaler_cls):
    m = build()
    m.encoder.requires_grad_(False)
    opt = vk.FusedAdamW(m.parameters(), lr=5e-5, weight_decay=1e-4).attach(m)
    scaler = vk.GradScaler("cuda", init_scale=2.0 ** 10) if scaler_cls == "vk" else torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    ref = _ref_copies(m)
    ref_opt = torch.optim.AdamW(ref, lr=5e-5, weight_decay=1e-4, foreach=False)
    enc = [n.startswith("encoder.") for n in names(m)]
    taken = 0
    for step in range(4):
        if step in (1, 2):
            scaler.update(new_scale=2.0 ** 60 if step == 1 else 2.0 ** 10)     # step 1: forced overflow (inf fp16 gradients)
        opt.zero_grad(set_to_none=True)
        x, y = batch(step)
        with torch.autocast("cuda", dtype=torch.float16):
            logits = m(x)
        loss = _BCE(logits.float(), y) + _DICE(logits.float(), y)
        scale = scaler.get_scale()
        scaler.scale(loss).backward()
        finite = all(torch.isfinite(p.grad).all().item() for p in m.parameters() if p.grad is not None)
        before = [p.detach().clone() for p in m.parameters()]
        scaler.step(opt)
        scaler.update()
        if finite:
            taken += 1
            _feed(ref, m, 1.0 / scale)
            ref_opt.step()
        torch.cuda.synchronize()
        assert finite != (step == 1), step
        assert opt.tensor_steps() == [0 if e else taken for e in enc], step
        for (n, p), r, b in zip(m.named_parameters(), ref, before):
            if step == 1 or not p.requires_grad:
                assert torch.equal(p.detach(), b), (step, n)
            assert (p.detach() - r.detach()).abs().max().item() <= 2e-7, (step, n)
        _resync(ref, m)
    assert taken == 3


def test_segmented_adamw_equals_whole_buffer_kernel():
    """vk_adamw_step_amp_segments with one segment per tensor, every tensor in, equal counters == vk_adamw_step_amp, bit for bit —
    GradScaler scale, extra inv_scale and a skipped step included."""
    L = vk.lib()
    m = vk.Unet(encoder_weights=None)
    n = m.flat_params.numel()
    gen = torch.Generator().manual_seed(7)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 100
    m0, v0 = torch.randn(n, generator=gen) * 1e-2, torch.rand(n, generator=gen) * 1e-3
    A = [t.clone().to(dev()) for t in (p0, g0, m0, v0)]
    B = [t.clone().to(dev()) for t in (p0, g0, m0, v0)]
    seg = torch.tensor([[off, off + numel, t] for t, (off, numel) in enumerate(m._param_ranges)], dtype=torch.int64)
    sp = C.cast(seg.data_ptr(), C.POINTER(C.c_int64))
    nb = L.vk_adamw_segment_blocks(len(seg), sp, None, 0)
    blocks = torch.empty((nb, 2), dtype=torch.int32)
    assert L.vk_adamw_segment_blocks(len(seg), sp, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), nb) == nb
    seg_d, blocks_d = seg.to(dev()), blocks.to(dev())
    step_a = torch.full((1,), 4, dtype=torch.int32, device=dev())
    steps_b = torch.full((140,), 4, dtype=torch.int32, device=dev())
    scr_a = torch.zeros(4, device=dev())
    scr_b = torch.zeros(4 + 2 * 140, device=dev())
    gs = torch.full((1,), 1024.0, device=dev())
    st = vk._lib.current_stream()
    inside = torch.zeros(n, dtype=torch.bool)
    for off, numel in m._param_ranges:
        inside[off:off + numel] = True
    inside = inside.to(dev())
    for found in (0.0, 1.0, 0.0):
        fi = torch.full((1,), found, device=dev())
        before_b = [t.clone() for t in B]
        vk._lib.check(L.vk_adamw_step_amp(n, *[t.data_ptr() for t in A], 5e-5, 0.9, 0.999, 1e-8, 1e-4, step_a.data_ptr(), 0.5,
                                          gs.data_ptr(), fi.data_ptr(), scr_a.data_ptr(), 0, 0, st))
        vk._lib.check(L.vk_adamw_step_amp_segments(140, seg_d.data_ptr(), nb, blocks_d.data_ptr(), *[t.data_ptr() for t in B], 5e-5, 0.9,
                                                   0.999, 1e-8, 1e-4, steps_b.data_ptr(), 0.5, gs.data_ptr(), fi.data_ptr(),
                                                   scr_b.data_ptr(), st))
        torch.cuda.synchronize()
        for a, b, b0 in zip(A, B, before_b):
            assert torch.equal(a[inside], b[inside]), found
            assert torch.equal(b[~inside], b0[~inside])              # padding between tensors is no segment's
        assert (steps_b == step_a).all().item()
    assert step_a.item() == 6


def test_everything_frozen():
    m = build()
    m.requires_grad_(False)
    x, y = batch()
    nbt0 = m._flat["nbt"].clone()
    out = m(x)
    assert out.requires_grad is False
    torch.cuda.synchronize()
    assert torch.equal(m._flat["nbt"], nbt0 + 1)          # train mode: the running statistics still update, as in torch
    with pytest.raises(vk.VkError):
        m.loss_and_backward(x, y, dtype=torch.bfloat16)
