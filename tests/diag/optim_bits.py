"""Diagnostic: SHA-256 of every buffer the optimizer entry points write, to compare two builds of the library bit for bit.

    python tests/diag/optim_bits.py > a.txt                       # this checkout
    VK_LIB=/path/to/other/libvkunet.so python tests/diag/optim_bits.py > b.txt      # its Python over another library
    python tests/diag/optim_bits.py --tree /path/to/other/checkout > c.txt          # another checkout's package and library
    diff a.txt b.txt

One process per library.  Entry points (vk_adamw_step, vk_adamw_step_amp, vk_adamw_step_amp_segments, vk_adamw_step_groups,
vk_grad_norm_segments, vk_amp_unscale_check) on the cases of tests/tail_cases.py and tests/param_groups_cases.py, then five-step
FusedAdamW trajectories on a 2 x 64 x 64 model, fp32 and bf16: plain; freeze then unfreeze; three groups with clip_grad_norm_; GradScaler
with a forced overflow.  The trajectories take their gradients from a seeded generator (written over the flat gradient buffer after a
real backward), so that a line depends on the optimizer alone."""
import ctypes as C
import hashlib
import importlib
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve()
TREE = Path(sys.argv[sys.argv.index("--tree") + 1]).resolve() if "--tree" in sys.argv else HERE.parents[2]
sys.path.insert(0, str(TREE))
sys.path.insert(0, str(HERE.parents[1]))
vk = importlib.import_module("vickers-hardness-unet_amd")
import param_groups_cases as PG  # noqa: E402
import tail_cases as TC  # noqa: E402

L_ = vk._lib
DEV = torch.device("cuda:0")


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def show(name, **bufs):
    torch.cuda.synchronize()
    print(name, " ".join(f"{k}={sha(v)}" for k, v in bufs.items() if v is not None), flush=True)


def st():
    return torch.cuda.current_stream().cuda_stream


def P_(t):
    return None if t is None else t.data_ptr()


def tables(segs):
    seg = torch.tensor([list(s) for s in segs], dtype=torch.int64)
    sp = C.cast(seg.data_ptr(), C.POINTER(C.c_int64))
    nb = vk.lib().vk_adamw_segment_blocks(len(segs), sp, None, 0)
    blocks = torch.empty((nb, 2), dtype=torch.int32)
    assert vk.lib().vk_adamw_segment_blocks(len(segs), sp, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), nb) == nb
    return seg.to(DEV), blocks.to(DEV), nb


def hp_tuple(h):
    return (h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"])


def group_array(hps):
    return (L_.vk_adamw_group * len(hps))(*[L_.vk_adamw_group(*hp_tuple(h)) for h in hps])


def entry_step(entry, segs, state, grad, hp, counters, t, found=None, lowp=None):
    """One step of `entry` over state = [p, m, v] (device).  "step" and "amp" take the whole buffer, the other two the segments."""
    L = vk.lib()
    p, m, v = state
    n = p.numel()
    gs = torch.full((1,), 1024.0, device=DEV)
    lp = torch.full((n,), 77.0, device=DEV).to(torch.bfloat16) if lowp else None
    code = L_.VK_BF16 if lowp else 0
    scratch = torch.zeros(4 + 2 * len(segs), device=DEV)
    if entry == "step":
        fl = None if found is None else torch.tensor([1], dtype=torch.int32, device=DEV)
        rc = L.vk_adamw_step(n, p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), *hp_tuple(hp), t, 2.0 ** -11, P_(fl), P_(lp), code, st())
    elif entry == "amp":
        rc = L.vk_adamw_step_amp(n, p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), *hp_tuple(hp), counters.data_ptr(), 0.5,
                                 gs.data_ptr(), P_(found), scratch.data_ptr(), P_(lp), code, st())
    else:
        seg, blocks, nb = tables(segs)
        if entry == "segments":
            rc = L.vk_adamw_step_amp_segments(len(segs), seg.data_ptr(), nb, blocks.data_ptr(), p.data_ptr(), grad.data_ptr(), m.data_ptr(),
                                              v.data_ptr(), *hp_tuple(hp), counters.data_ptr(), 0.5, gs.data_ptr(), P_(found),
                                              scratch.data_ptr(), st())
        else:
            sg = torch.zeros(len(segs), dtype=torch.int32, device=DEV)
            rc = L.vk_adamw_step_groups(len(segs), seg.data_ptr(), sg.data_ptr(), nb, blocks.data_ptr(), p.data_ptr(), grad.data_ptr(),
                                        m.data_ptr(), v.data_ptr(), 1, group_array([hp]), counters.data_ptr(), 0.5, gs.data_ptr(), P_(found),
                                        None, scratch.data_ptr(), st())
    L_.check(rc, entry)
    return scratch, lp


ENTRIES = ("step", "amp", "segments", "groups")


def entry_cases():
    # the exact first step on every size of the sweep
    for n in TC.ADAMW_SIZES:
        p0, gr = TC.exact_adamw_inputs(n, n)
        for e in ENTRIES:
            state = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
            cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
            scr, lp = entry_step(e, [(0, n, 0)], state, (gr * 2048.0).to(DEV), TC.EXACT_HP, cnt, 1, lowp=e in ("step", "amp"))
            show(f"exact n={n} {e}", p=state[0], m=state[1], v=state[2], cnt=cnt, scratch=None if e == "step" else scr, lowp=lp)
    # five rounded steps from step t0, then a skipped one
    n = 10007
    for t0 in (1, 2, 100000):
        for hname, hp in (("default", TC.DEFAULT_HP), ("wd0", dict(TC.DEFAULT_HP, wd=0.0))):
            for e in ENTRIES:
                g = torch.Generator().manual_seed(t0)
                state = [torch.randn(n, generator=g).to(DEV), (torch.randn(n, generator=g) * 0.1).to(DEV), (torch.rand(n, generator=g) * 0.01).to(DEV)]
                cnt = torch.full((1,), t0 - 1, dtype=torch.int32, device=DEV)
                for k in range(5):
                    gr = (TC.rounded_adamw_grad(n, 10 * t0 + k) * 2048.0).to(DEV)
                    scr, lp = entry_step(e, [(0, n, 0)], state, gr, hp, cnt, t0 + k, lowp=e in ("step", "amp"))
                show(f"rounded t0={t0} {hname} {e}", p=state[0], m=state[1], v=state[2], cnt=cnt, scratch=None if e == "step" else scr, lowp=lp)
                nan = torch.full((1,), float("nan"), device=DEV)
                scr, lp = entry_step(e, [(0, n, 0)], state, gr, hp, cnt, t0 + 5, found=nan, lowp=e in ("step", "amp"))
                show(f"skipped t0={t0} {hname} {e}", p=state[0], m=state[1], v=state[2], cnt=cnt, scratch=None if e == "step" else scr, lowp=lp)
    # ragged segments with a counter each; then G groups with grad_scale and a clip coefficient
    ranges, total = PG.layout()
    segs = [(b, e, i) for i, (b, e) in enumerate(ranges)]
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(total, generator=g), torch.randn(total, generator=g) * 0.1, torch.rand(total, generator=g) * 0.01]
    gr = (TC.rounded_adamw_grad(total, 31) * 2048.0).to(DEV)
    for e in ("segments", "groups"):
        state = [t.to(DEV) for t in base]
        cnt = torch.tensor([(7 * i) % 50 for i in range(len(segs))], dtype=torch.int32, device=DEV)
        for _ in range(2):
            scr, _ = entry_step(e, segs, state, gr, TC.DEFAULT_HP, cnt, 0)
        show(f"ragged {e}", p=state[0], m=state[1], v=state[2], cnt=cnt, scratch=scr)
    seg, blocks, nb = tables(segs)
    for G in PG.GROUP_COUNTS:
        for clip in (None, 0.37):
            state = [t.to(DEV) for t in base]
            cnt = torch.tensor([(7 * i) % 50 for i in range(len(segs))], dtype=torch.int32, device=DEV)
            sg = torch.tensor([PG.group_index(i, G) for i in range(len(segs))], dtype=torch.int32, device=DEV)
            gs = torch.full((1,), 1024.0, device=DEV)
            cc = None if clip is None else torch.full((1,), clip, device=DEV)
            scr = torch.zeros(4 + 2 * len(segs), device=DEV)
            for _ in range(2):
                L_.check(vk.lib().vk_adamw_step_groups(len(segs), seg.data_ptr(), sg.data_ptr(), nb, blocks.data_ptr(), state[0].data_ptr(),
                                                       gr.data_ptr(), state[1].data_ptr(), state[2].data_ptr(), G, group_array(PG.HP_SETS[:G]),
                                                       cnt.data_ptr(), 0.5, gs.data_ptr(), None, P_(cc), scr.data_ptr(), st()))
            show(f"groups G={G} clip={clip}", p=state[0], m=state[1], v=state[2], cnt=cnt, scratch=scr)
    # the gradient norm
    for gname, grad in (("lattice", PG.lattice_grad(total, 3)), ("rounded", TC.rounded_adamw_grad(total, 32))):
        gd = grad.to(DEV)
        for kind in (PG.NORM_L2, PG.NORM_INF):
            partials = torch.zeros(nb, dtype=torch.float64, device=DEV)
            out = torch.zeros(2, device=DEV)
            L_.check(vk.lib().vk_grad_norm_segments(len(segs), seg.data_ptr(), nb, blocks.data_ptr(), gd.data_ptr(), kind, 0.5, 1.0,
                                                    partials.data_ptr(), out.data_ptr(), st()))
            show(f"grad_norm {gname} kind={kind}", partials=partials, out=out)
    # GradScaler's unscale and check
    for n in (8, 4 * 257, 2 ** 22 + 4):
        for inv in (None, 2.0 ** -16, 1.0 / 3.0):
            for poison in (None, n - 1):
                gd = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
                if poison is not None:
                    gd[poison] = float("inf")
                found = torch.zeros(1, device=DEV)
                iv = None if inv is None else torch.full((1,), inv, device=DEV)
                L_.check(vk.lib().vk_amp_unscale_check(n, gd.data_ptr(), P_(iv), found.data_ptr(), st()))
                show(f"amp_unscale_check n={n} inv={inv} poison={poison}", g=gd, found=found)


def trajectories():
    from oracle import unet_oracle as O
    x, y = O.synthetic_batch(2, 64, seed=300)
    x, y = x.to(DEV), y.to(DEV)

    def model():
        O.set_seed(21)
        return vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(DEV).train()

    def seeded_grads(m, k, scale=1.0, inf=False):
        g = torch.randn(m.flat_grads.numel(), generator=torch.Generator().manual_seed(900 + k)) * 1e-2 * scale
        if inf:
            g[12345] = float("inf")
        m.flat_grads.copy_(g.to(DEV))

    def state(opt, m):
        return dict(p=m.flat_params, m=opt._m, v=opt._v, step=opt._step_dev, steps=opt._steps_dev, scratch=opt._scratch,
                    seg_scratch=opt._seg_scratch)

    for dname, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for kind in ("plain", "freeze_unfreeze", "three_groups_clip", "gradscaler_overflow"):
            m = model()
            if kind == "three_groups_clip":
                spec = PG.three_groups(vk, m, 5e-5)
                opt = vk.adamw_for(m, lr=5e-5, weight_decay=1e-4, groups=PG.as_param_groups(spec, m.parameters()))
            else:
                opt = vk.adamw_for(m, lr=5e-5, weight_decay=1e-4)
            scaler = vk.GradScaler("cuda", init_scale=1024.0) if kind == "gradscaler_overflow" else None
            for k in range(5):
                if kind == "freeze_unfreeze":
                    m.encoder.requires_grad_(k not in (1, 2))
                opt.zero_grad(set_to_none=True)
                scale = 1.0
                if scaler:
                    scaler.scale(torch.zeros((), device=DEV))       # what the loss goes through: the scale now lives on the device
                    scale = scaler.get_scale()
                m.loss_and_backward(x, y, dtype=dt, grad_scale=scale)
                seeded_grads(m, k, scale=scale, inf=scaler is not None and k == 2)
                if kind == "three_groups_clip":
                    show(f"traj {dname} {kind} step {k} norm", norm=opt.clip_grad_norm_(0.5))
                if scaler:
                    scaler.step(opt)                                # check only (vk_amp_unscale_check), then step() with the device scalars
                    scaler.update()
                else:
                    opt.step()
                show(f"traj {dname} {kind} step {k}", **state(opt, m), scale=scaler._scale if scaler else None)
            print(f"traj {dname} {kind} tensor_steps", sorted(set(opt.tensor_steps())), flush=True)


if __name__ == "__main__":
    print("# library", L_.LIB_PATH.name, "package tree", "other" if "--tree" in sys.argv else "this", flush=True)
    entry_cases()
    trajectories()
