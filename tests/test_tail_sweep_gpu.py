"""The tail of a training step through the C ABI against float64, on the cases of tests/tail_cases.py: the segmentation head
(vk_head_fwd / vk_head_bwd / vk_head_bwd_fused, vk_head_fwd_multi / vk_head_bwd_multi), the fused inference tail vk_dec4_tail_eval,
vk_bce_dice_loss, vk_adamw_step / vk_adamw_step_amp / vk_adamw_step_amp_segments, vk_amp_unscale_check and vk_amp_check_inf.

EXACT tier.  Head and dec4 tail on the integer lattice, AdamW's first step on its power-of-two setting, BCE+Dice at x = 0: the result must
EQUAL float64 (torch.equal) in every element, on every route (matrix cores, VK_HEAD_NO_MFMA), with no workspace (fp32 atomics), the full
one and one of exactly three rows, and on a second run.  dw / dbias start from integers of their own (a store in place of += is seen),
dy / logits / dlogits start sentinel-filled (an unwritten pixel is seen), optimizer buffers carry guard elements either side.
tests/test_tail_cases_cpu.py proves on the references alone that each case meets the conditions under which equality must hold.

ROUNDED tier.  BCE+Dice on seeded logits and AdamW over five steps with default hyper-parameters, against float64 of the same fp32
inputs, under elementwise bounds that are formulas of tests/tail_cases.py (their only measured input is the function error K_FUNC)."""
import ctypes as C
import functools
import importlib
from types import SimpleNamespace

import pytest
import torch

import tail_cases as TC
from conv_lattice import TDT

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
CODE = {"f32": L_.VK_F32, "bf16": L_.VK_BF16, "f16": L_.VK_F16}
REPL = 32                      # VK_STATS_REPLICAS
SENTINEL = 77.0                # exact in every type
HEAD_WS_BYTES = 1024 * 148 * 4  # VK_HEAD_WORKSPACE_BYTES
GUARD = 4                      # guard elements either side of an optimizer buffer (keeps the 16-byte alignment of the payload)


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return vk.lib()


def P_(t):
    return None if t is None else t.data_ptr()


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())


def fvec(t):
    return None if t is None else t.float().to(dev())


def filled(shape, dt, value=SENTINEL):
    return torch.full(shape, value, dtype=dt, device=dev())


def typed(cases):
    return [pytest.param(c, t, id=f"{c.name}-{t}") for c in cases for t in c.types]


def where_bad(got, ref, what, path, tile=16):
    """got, ref: same shape, [N][C][H][W] (or anything else, flat).  Count, first wrong element, its 16 x 16 tile, the path."""
    got, ref = got.double().cpu(), ref.double().cpu()
    bad = got != ref
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    where = f"image {idx[0]} channel {idx[1]} pixel ({idx[2]}, {idx[3]}) tile ({idx[2] // tile}, {idx[3] // tile})" if len(idx) == 4 else f"index {idx}"
    return f"[{path}] {what}: {int(bad.sum())} of {bad.numel()} wrong; first at {where}: got {got[idx].item()!r}, want {ref[idx].item()!r}"


# ================================================================================================ head, exact tier
@functools.lru_cache(maxsize=2)
def head_built(case):
    return TC.head_build(case)


class HeadDev:
    """The operands of one (case, type) on the device, and the expected results in the type they are stored in (exact there: CPU file)."""

    def __init__(self, case, dtn):
        b = head_built(case)
        dt = TDT[dtn]
        self.case, self.dtn, self.dt, self.b = case, dtn, dt, b
        self.z = nhwc(b.z, dt)
        self.scale, self.shift = fvec(b.scale), fvec(b.shift)
        self.src = L_.vk_src(self.z.data_ptr(), 16, 0, P_(self.scale), P_(self.shift), case.relu)
        # filter: binary [3][3][16], multi [C][3][3][16]; bias [C]
        wk = b.w.permute(0, 2, 3, 1).contiguous().float()
        self.w = (wk[0] if case.C == 0 else wk).contiguous().to(dev())
        self.bias = b.bias.float().to(dev())
        self.dl = b.dl.float().contiguous().to(dev())
        d0 = b.dw0.permute(0, 2, 3, 1).contiguous().float()
        self.dw0 = (d0[0] if case.C == 0 else d0).contiguous().to(dev())
        self.db0 = b.db0.float().to(dev())
        dwr = (b.dw0 + b.dw).permute(0, 2, 3, 1).contiguous().float()
        self.dw_ref = (dwr[0] if case.C == 0 else dwr).contiguous().to(dev())
        self.db_ref = (b.db0 + b.db).float().to(dev())
        self.logits_ref = b.logits.float().to(dev())
        self.g_ref = nhwc(b.g, dt)
        self.bz = self.bscale = self.bshift = None
        if case.bnr == "own":
            self.bz, self.bscale, self.bshift = self.z, self.scale, self.shift
        elif case.bnr:
            self.bz = self.z if case.bnr == "own_z" else nhwc(b.bz, dt)
            self.bscale, self.bshift = fvec(b.bscale), fvec(b.bshift)

    def forward(self, errors, path):
        c = self.case
        logits = filled((c.N, c.classes, c.H, c.W), torch.float32)
        if c.C == 0:
            rc = lib().vk_head_fwd(CODE[self.dtn], c.N, c.H, c.W, C.byref(self.src), self.w.data_ptr(), self.bias.data_ptr(), logits.data_ptr(), st())
        else:
            rc = lib().vk_head_fwd_multi(CODE[self.dtn], c.N, c.H, c.W, c.C, C.byref(self.src), self.w.data_ptr(), self.bias.data_ptr(),
                                         logits.data_ptr(), st())
        L_.check(rc, "head forward")
        torch.cuda.synchronize()
        if not torch.equal(logits, self.logits_ref):
            errors.append(where_bad(logits, self.logits_ref, "logits", path))
        return logits

    def backward(self, errors, path, ws_bytes):
        """ws_bytes None: no workspace (binary head only: fp32 atomics)."""
        c = self.case
        dy = filled((c.N, c.H, c.W, 16), self.dt)
        dw, db = self.dw0.clone(), self.db0.clone()
        sums = torch.zeros(REPL * 32, dtype=torch.float64, device=dev())
        ws = None if ws_bytes is None else torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
        bnr = None
        if c.bnr:
            bnr = L_.vk_bnr(self.bz.data_ptr(), self.bscale.data_ptr(), self.bshift.data_ptr(), sums.data_ptr(), None, 0)
        code = CODE[self.dtn]
        if c.C == 0 and not c.bnr:
            rc = lib().vk_head_bwd(code, c.N, c.H, c.W, C.byref(self.src), self.w.data_ptr(), self.dl.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                                   db.data_ptr(), P_(ws), ws_bytes or 0, st())
        elif c.C == 0:
            rc = lib().vk_head_bwd_fused(code, c.N, c.H, c.W, C.byref(self.src), self.w.data_ptr(), self.dl.data_ptr(), dy.data_ptr(),
                                         dw.data_ptr(), db.data_ptr(), C.byref(bnr), P_(ws), ws_bytes or 0, st())
        else:
            rc = lib().vk_head_bwd_multi(code, c.N, c.H, c.W, c.C, C.byref(self.src), self.w.data_ptr(), self.dl.data_ptr(), dy.data_ptr(),
                                         dw.data_ptr(), db.data_ptr(), C.byref(bnr) if bnr else None, P_(ws), ws_bytes or 0, st())
        L_.check(rc, "head backward")
        torch.cuda.synchronize()
        if not torch.equal(dy, self.g_ref):
            errors.append(where_bad(dy.permute(0, 3, 1, 2), self.g_ref.permute(0, 3, 1, 2), "dy", path))
        if not torch.equal(dw, self.dw_ref):
            bad = (dw != self.dw_ref).nonzero()[0].tolist()
            errors.append(f"[{path}] dw: {int((dw != self.dw_ref).sum())} of {dw.numel()} wrong; first at (class,) tap, channel {bad}: got "
                          f"{dw[tuple(bad)].item()!r}, want {self.dw_ref[tuple(bad)].item()!r} (started from {self.dw0[tuple(bad)].item()!r})")
        if not torch.equal(db, self.db_ref):
            errors.append(f"[{path}] dbias: got {db.tolist()}, want {self.db_ref.tolist()} (started from {self.db0.tolist()})")
        if c.bnr:
            got = sums.view(REPL, 2, 16).sum(0).cpu()              # integers (or halves) in fp64, added over the replicas
            for i, nm in enumerate(("sum g", "sum g z")):
                if not torch.equal(got[i], self.b.sums[i]):
                    ch = int((got[i] != self.b.sums[i]).nonzero()[0])
                    errors.append(f"[{path}] BN-backward {nm}: first wrong channel {ch}: got {got[i, ch].item()!r}, want {self.b.sums[i][ch].item()!r}")
        elif bool(sums.any()):
            errors.append(f"[{path}] BN-backward sums written without a vk_bnr")
        return dy, dw, db


def head_ws_sizes(case):
    """name -> workspace bytes: none (binary head: fp32 atomics, still exact on the lattice), full, exactly three rows (the grid shrinks to
    the workspace's capacity and every workgroup walks a third of the tiles)."""
    if case.C == 0:
        return {"ws_none": None, "ws_full": HEAD_WS_BYTES, "ws_3rows": 3 * 148 * 4}
    full = lib().vk_head_multi_workspace_bytes(case.C)           # 1,024 rows, one per workgroup of the largest grid
    assert full % 1024 == 0 and full // 1024 >= 145 * case.C * 4
    return {"ws_full": full, "ws_3rows": 3 * (full // 1024)}


def run_head_case(case, dtn, monkeypatch):
    hd = HeadDev(case, dtn)
    errors, outs = [], {}
    for route in (("mfma", "valu") if case.C == 0 else ("default",)):
        if route == "valu":
            monkeypatch.setenv("VK_HEAD_NO_MFMA", "1")
        else:
            monkeypatch.delenv("VK_HEAD_NO_MFMA", raising=False)
        hd.forward(errors, route)
        for wname, wbytes in head_ws_sizes(case).items():
            for rep in (1, 2):
                outs[f"{route}/{wname}/run{rep}"] = hd.backward(errors, f"{route}/{wname}/run{rep}", wbytes)
    # every path equals the reference, hence the others; said once more so that a failure names the pair
    names = list(outs)
    for nm in names[1:]:
        if not all(torch.equal(a, b_) for a, b_ in zip(outs[names[0]], outs[nm])):
            errors.append(f"path {nm} differs from path {names[0]} bit for bit")
    errors = [e for e in errors if e]
    assert not errors, f"{case.name} {dtn} ({case.tiles} tiles):\n" + "\n".join(errors[:12])


@pytest.mark.parametrize("case,dtn", typed(TC.head_cases()))
def test_head_exact(case, dtn, monkeypatch):
    run_head_case(case, dtn, monkeypatch)


@pytest.mark.parametrize("case,dtn", typed(TC.head_multi_cases()))
def test_head_multi_exact(case, dtn, monkeypatch):
    run_head_case(case, dtn, monkeypatch)


@pytest.mark.parametrize("case,dtn", typed(TC.head_large_cases()))
def test_head_exact_past_the_launch_caps(case, dtn, monkeypatch):
    """More tiles than k_head_dgrad (2,048), k_head_wgrad / k_head_bwd_mfma / k_head_bwd_multi (1,024) launch workgroups: the persistent
    loops take a second trip at the op level, with the double-buffered dlogits staging and the hand-over of the prefetched tile."""
    assert case.tiles > 1024
    run_head_case(case, dtn, monkeypatch)


def test_head_multi_refuses_a_missing_workspace():
    case = TC.head_multi_cases()[1]
    hd = HeadDev(case, "f32")
    dy, dw, db = filled((case.N, case.H, case.W, 16), torch.float32), hd.dw0.clone(), hd.db0.clone()
    for ws, nbytes in ((None, 0), (torch.empty(64, dtype=torch.uint8, device=dev()), 64)):
        rc = lib().vk_head_bwd_multi(CODE["f32"], case.N, case.H, case.W, case.C, C.byref(hd.src), hd.w.data_ptr(), hd.dl.data_ptr(), dy.data_ptr(),
                                     dw.data_ptr(), db.data_ptr(), None, P_(ws), nbytes, st())
        torch.cuda.synchronize()
        assert rc < 0 and bool((dy == SENTINEL).all()) and torch.equal(dw, hd.dw0) and torch.equal(db, hd.db0)


# ================================================================================================ vk_dec4_tail_eval, exact tier
def conv_desc(dtn, N, H, W, K, s0):
    return L_.vk_conv_desc(CODE[dtn], N, H, W, H, W, K, 3, 3, 1, 1, 0, s0, L_.vk_src(None, 0, 0, None, None, 0))


class TailDev:
    def __init__(self, case, dtn):
        b = TC.tail_build(case)
        dt = TDT[dtn]
        self.case, self.dtn, self.dt, self.b = case, dtn, dt, b
        self.x = nhwc(b.x, dt)
        self.s0, self.h0 = fvec(b.s0), fvec(b.h0)
        self.src = L_.vk_src(self.x.data_ptr(), 32, 1, self.s0.data_ptr(), self.h0.data_ptr(), 1)
        self.w1 = b.w1.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())          # [16][3][3][32]
        self.w1_pack = torch.empty_like(self.w1)
        L_.check(lib().vk_halo_pack(CODE[dtn], 16, 32, self.w1.data_ptr(), self.w1_pack.data_ptr(), st()), "vk_halo_pack")
        self.w2 = b.w2.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())          # [16][3][3][16]
        self.s1, self.h1, self.s2, self.h2 = fvec(b.s1), fvec(b.h1), fvec(b.s2), fvec(b.h2)
        self.hw = b.hw[0].permute(1, 2, 0).contiguous().float().to(dev())         # [3][3][16]
        self.hb = b.hb.float().to(dev())

    def fused(self):
        c = self.case
        logits = filled((c.N, 1, c.H, c.W), torch.float32)
        rc = lib().vk_dec4_tail_eval(CODE[self.dtn], c.N, c.H, c.W, C.byref(self.src), self.w1_pack.data_ptr(), self.s1.data_ptr(),
                                     self.h1.data_ptr(), self.w2.data_ptr(), self.s2.data_ptr(), self.h2.data_ptr(), self.hw.data_ptr(),
                                     self.hb.data_ptr(), logits.data_ptr(), st())
        torch.cuda.synchronize()
        return rc, logits

    def separate(self):
        """vk_conv_fwd x 2 + vk_head_fwd: the two 16-channel tensors go through memory in the element type."""
        c = self.case
        z1, z2 = filled((c.N, c.H, c.W, 16), self.dt), filled((c.N, c.H, c.W, 16), self.dt)
        d1 = conv_desc(self.dtn, c.N, c.H, c.W, 16, self.src)
        if lib().vk_conv_uses_halo_pack(C.byref(d1)):
            L_.check(lib().vk_conv_fwd_packed(C.byref(d1), self.w1_pack.data_ptr(), z1.data_ptr(), None, 0, 0, None, st()), "conv1")
        else:
            L_.check(lib().vk_conv_fwd(C.byref(d1), self.w1.data_ptr(), z1.data_ptr(), None, 0, 0, None, st()), "conv1")
        d2 = conv_desc(self.dtn, c.N, c.H, c.W, 16, L_.vk_src(z1.data_ptr(), 16, 0, self.s1.data_ptr(), self.h1.data_ptr(), 1))
        L_.check(lib().vk_conv_fwd(C.byref(d2), self.w2.data_ptr(), z2.data_ptr(), None, 0, 0, None, st()), "conv2")
        src = L_.vk_src(z2.data_ptr(), 16, 0, self.s2.data_ptr(), self.h2.data_ptr(), 1)
        logits = filled((c.N, 1, c.H, c.W), torch.float32)
        L_.check(lib().vk_head_fwd(CODE[self.dtn], c.N, c.H, c.W, C.byref(src), self.hw.data_ptr(), self.hb.data_ptr(), logits.data_ptr(), st()),
                 "vk_head_fwd")
        torch.cuda.synchronize()
        return z1, z2, logits


@pytest.mark.parametrize("case,dtn", typed(TC.tail_cases()))
def test_dec4_tail_eval_exact(case, dtn):
    td = TailDev(case, dtn)
    b = td.b
    errors = []
    z1, z2, sep = td.separate()
    errors.append(where_bad(z1.permute(0, 3, 1, 2), b.z1, "z1 of the separate calls", "separate"))
    errors.append(where_bad(z2.permute(0, 3, 1, 2), b.z2, "z2 of the separate calls", "separate"))
    errors.append(where_bad(sep, b.logits, "logits of the separate calls", "separate"))
    for rep in (1, 2):
        rc, fused = td.fused()
        L_.check(rc, "vk_dec4_tail_eval")
        errors.append(where_bad(fused, b.logits, "logits", f"fused/run{rep}"))
        if not torch.equal(fused, sep):
            errors.append(f"[fused/run{rep}] differs from the three separate calls bit for bit")
    errors = [e for e in errors if e]
    assert not errors, f"{case.name} {dtn}:\n" + "\n".join(errors)


@pytest.mark.parametrize("case,dtn", typed(TC.tail_outside_cases()))
def test_dec4_tail_eval_outside_documented_set(case, dtn):
    """An extent that is no multiple of 16, or fp32: a negative code with the sentinel-filled logits untouched, or VK_OK and exact."""
    td = TailDev(case, dtn)
    rc, logits = td.fused()
    print(f"vk_dec4_tail_eval {case.name} {dtn}: {'ran' if rc == 0 else 'returned %d' % rc}")        # pytest -rP
    assert rc <= 0, lib().vk_last_error_string()
    if rc < 0:
        assert bool((logits == SENTINEL).all())
    else:
        msg = where_bad(logits, td.b.logits, "logits", "fused")
        assert msg is None, msg


# ================================================================================================ BCE + Dice
def offset_copy(t, off):
    """A device copy of t that starts `off` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev())
    v = buf[off:off + t.numel()]
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (off % 4 == 0)
    return v


def run_loss(x, y, wb, wd, gs, align="aligned", want_grad=True):
    """x, y: fp32 CPU tensors.  Returns (sums[8] float64, loss_out[3], dlogits or None), all on the CPU; dlogits is checked for its guards."""
    n = x.numel()
    xd = offset_copy(x, 1 if align == "x_off" else 0)
    yd = offset_copy(y, 1 if align == "y_off" else 0)
    sums = torch.full((8,), SENTINEL, dtype=torch.float64, device=dev())
    out = filled((4,), torch.float32)
    dl_full = filled((n + 2 * GUARD,), torch.float32)
    dl = dl_full[GUARD:GUARD + n]
    L_.check(lib().vk_bce_dice_loss(n, xd.data_ptr(), yd.data_ptr(), sums.data_ptr(), out.data_ptr(), dl.data_ptr() if want_grad else None,
                                    gs, wb, wd, st()), "vk_bce_dice_loss")
    torch.cuda.synchronize()
    assert bool((dl_full[:GUARD] == SENTINEL).all()) and bool((dl_full[GUARD + n:] == SENTINEL).all()), "dlogits written outside [0, count)"
    assert out[3].item() == SENTINEL
    if not want_grad:
        assert bool((dl == SENTINEL).all()), "dlogits = NULL, yet the buffer next to it was written"
    return sums.cpu(), out[:3].cpu(), dl.cpu().clone() if want_grad else None


ZERO_TIER = ([(n, a) for n in (1, 3, 4, 5, 1023, 1025) for a in ("aligned", "x_off", "y_off")] +
             [(2 ** 21 + 5, "aligned"), (TC.LOSS_SCALAR_LARGE, "x_off"), (TC.LOSS_SCALAR_LARGE, "y_off")])


@pytest.mark.parametrize("count,align", ZERO_TIER, ids=[f"{n}-{a}" for n, a in ZERO_TIER])
def test_bce_dice_at_zero_logits_is_exact(count, align):
    """x = 0: p = 1/2 exactly, so sums[1..3] = {T/2, count/2, T} whatever the route (vector body, scalar tail, unaligned scalar route,
    second grid-stride trip): a skipped or doubled element is a difference of 1/2.  The Dice value is the float nearest float64."""
    x = torch.zeros(count)
    y = ((torch.arange(count) * 7) % 10 < 3).float()
    y[-1] = 1.0                                                     # the last element counts
    r = TC.loss_ref(x, y, 1.0, 1.0)
    sums, out, dl = run_loss(x, y, 1.0, 1.0, 2.0, align)
    T = float(y.sum())
    assert sums[1:4].tolist() == [T / 2.0, count / 2.0, T], f"sums[1..3] = {sums[1:4].tolist()}, want {[T / 2.0, count / 2.0, T]}"
    assert out[2].item() == torch.tensor(r.dice, dtype=torch.float64).float().item()
    vec = align == "aligned"
    bd = TC.loss_bounds(r, vec, 1.0, 1.0, False)
    assert abs(sums[0].item() - r.sums[0]) <= bd.s0 and abs(out[1].item() - r.bce) <= bd.bce
    # closed form (1/2 - y) invc + (ky y + k0) / 4 with exact sums: only the roundings of k_loss_bwd remain
    bd.dI = bd.dcard = 0.0
    err = (dl.double() / 2.0 - r.grad).abs()
    gb = TC.loss_grad_bound(r, bd, 1.0)
    i = int((err - gb).argmax())
    assert bool((err <= gb).all()), f"dlogits[{i}]: error {err[i].item():.3e} > bound {gb[i].item():.3e}"


def check_loss_rounded(x, y, wb, wd, gs, align, soft, label):
    r = TC.loss_ref(x, y, wb, wd)
    sums, out, dl = run_loss(x, y, wb, wd, gs, align)
    vec = align == "aligned"
    bd = TC.loss_bounds(r, vec, wb, wd, soft)
    figs = []
    for nm, got, want, bound in (("sum bce", sums[0].item(), r.sums[0], bd.s0), ("sum p y", sums[1].item(), r.sums[1], bd.s1),
                                 ("sum p", sums[2].item(), r.sums[2], bd.s2), ("sum y", sums[3].item(), r.sums[3], bd.s3),
                                 ("loss_out[0]", out[0].item(), r.total, bd.total), ("loss_out[1]", out[1].item(), r.bce, bd.bce),
                                 ("loss_out[2]", out[2].item(), r.dice, bd.dice)):
        figs.append((nm, abs(got - want), bound))
    err = (dl.double() / gs - r.grad).abs()
    gb = TC.loss_grad_bound(r, bd, wd)
    i = int((err / gb).argmax())
    print(f"{label}: " + ", ".join(f"{nm} {e:.2e}/{bnd:.2e}" for nm, e, bnd in figs) + f", dlogits[{i}] {err[i].item():.2e}/{gb[i].item():.2e}")
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(out).all())
    for nm, e, bnd in figs:
        assert e <= bnd, f"{label}: {nm} off by {e:.3e} > bound {bnd:.3e}"
    assert bool((err <= gb).all()), f"{label}: dlogits[{i}] (x {x[i].item()!r}, y {y[i].item()!r}): error {err[i].item():.3e} > bound {gb[i].item():.3e}"
    return r, out


ROUNDED_LOSS = ([(n, k, ("aligned", "x_off", "y_off")[(i + j) % 3]) for i, n in enumerate((1, 3, 4, 5, 1023, 1025)) for j, k in enumerate(("hard", "soft"))] +
                [(2 ** 21 + 5, "hard", "aligned"), (TC.LOSS_SCALAR_LARGE, "soft", "x_off")])


@pytest.mark.parametrize("count,kind,align", ROUNDED_LOSS, ids=[f"{n}-{k}-{a}" for n, k, a in ROUNDED_LOSS])
def test_bce_dice_rounded(count, kind, align):
    x, y = TC.loss_inputs(count, kind, count)
    if kind == "hard":
        y[0] = 1.0
    check_loss_rounded(x, y, 1.0, 1.0, 2.0, align, kind == "soft", f"{count} {kind} {align}")


@pytest.mark.parametrize("gs", [1.0, 2.0, 65536.0])
@pytest.mark.parametrize("wb,wd", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0)])
def test_bce_dice_weights_and_grad_scale(wb, wd, gs):
    x, y = TC.loss_inputs(4099, "hard", 77)
    check_loss_rounded(x, y, wb, wd, gs, "aligned", False, f"w ({wb}, {wd}) scale {gs}")


def test_bce_dice_edges():
    n = 4099
    x, y = TC.loss_inputs(n, "hard", 5)
    # an empty target: Dice 0 and its gradient 0 (what remains is the BCE gradient)
    r, out = check_loss_rounded(x, torch.zeros(n), 1.0, 1.0, 1.0, "aligned", False, "empty target")
    assert out[2].item() == 0.0
    _, out0, dl = run_loss(x, torch.zeros(n), 0.0, 1.0, 1.0)
    assert out0[0].item() == 0.0 and out0[2].item() == 0.0 and bool((dl == 0).all())
    # all ones
    check_loss_rounded(x, torch.ones(n), 1.0, 1.0, 2.0, "aligned", False, "all-ones target")
    # every logit at -100 with an empty target: card <= eps takes the clamp; nothing is NaN
    r, out = check_loss_rounded(torch.full((n,), -100.0), torch.zeros(n), 1.0, 1.0, 2.0, "aligned", False, "card <= eps clamp")
    assert r.clamped and out[2].item() == 0.0
    # large |x|, both signs, against both targets
    for big in (20.0, 88.0, 100.0):
        xb = torch.tensor([big, -big, big, -big, 0.5, -0.25, big, -big] * 33)
        yb = torch.tensor([1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0] * 33)
        check_loss_rounded(xb, yb, 1.0, 1.0, 65536.0, "aligned", False, f"|x| = {big}")
    # dlogits = NULL: the values are the same and a sentinel buffer stays untouched (run_loss asserts it)
    s1, o1, _ = run_loss(x, y, 1.0, 1.0, 2.0)
    s2, o2, none = run_loss(x, y, 1.0, 1.0, 2.0, want_grad=False)
    assert none is None and torch.equal(o1, o2) and torch.equal(s1[:4], s2[:4])


# ================================================================================================ AdamW
def guarded(t):
    """(whole buffer, payload view) on the device: the payload sits between GUARD sentinel elements either side."""
    full = torch.full((t.numel() + 2 * GUARD,), SENTINEL, dtype=t.dtype, device=dev())
    v = full[GUARD:GUARD + t.numel()]
    v.copy_(t)
    return full, v


def guards_ok(full):
    return bool((full[:GUARD] == SENTINEL).all()) and bool((full[-GUARD:] == SENTINEL).all())


def seg_tables(segs):
    """segs: [(begin, end, tensor_index)].  Device tables of vk_adamw_step_amp_segments."""
    seg = torch.tensor([list(s) for s in segs], dtype=torch.int64)
    sp = C.cast(seg.data_ptr(), C.POINTER(C.c_int64))
    nb = lib().vk_adamw_segment_blocks(len(segs), sp, None, 0)
    assert nb >= len(segs)
    blocks = torch.empty((nb, 2), dtype=torch.int32)
    assert lib().vk_adamw_segment_blocks(len(segs), sp, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), nb) == nb
    return seg.to(dev()), blocks.to(dev()), nb


class Adam:
    """One flat optimizer state on the device with guard elements, stepped through one of the three entry points.
    entry "step": vk_adamw_step (step and factor from the host); "amp": vk_adamw_step_amp; "segments": vk_adamw_step_amp_segments over
    one segment [0, n).  The device-protocol entries get grad_scale = 1024 and inv_scale = 0.5 (factor 2^-11), the host one inv_scale."""

    def __init__(self, entry, p, m, v, hp, t_done, lowp=None):
        self.entry, self.hp, self.n, self.lowp = entry, hp, p.numel(), lowp
        self.P, self.p = guarded(p)
        self.M, self.m = guarded(m)
        self.V, self.v = guarded(v)
        self.t = t_done
        self.counter = torch.full((3,), 0, dtype=torch.int32, device=dev())
        self.counter[1] = t_done                                          # counters either side of the one in use must not move
        self.scratch = torch.zeros(8, device=dev())
        self.gs = torch.full((1,), 1024.0, device=dev())
        self.LP = self.lp = None
        if lowp is not None:
            self.LP, self.lp = guarded(torch.full((self.n,), SENTINEL).to(TDT[lowp]))
        if entry == "segments":
            self.seg, self.blocks, self.nb = seg_tables([(0, self.n, 1)])

    @property
    def factor(self):
        return 0.5 if self.entry == "step" else 2.0 ** -11

    def step(self, grad, found=None):
        """grad: fp32 CPU tensor.  found: None, or a device tensor (int32 for "step", fp32 otherwise)."""
        self.G, g = guarded(grad)
        h = self.hp
        hyper = (h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"])
        lowp_code = CODE[self.lowp] if self.lowp else 0
        if self.entry == "step":
            rc = lib().vk_adamw_step(self.n, self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), *hyper, self.t + 1, 0.5,
                                     P_(found), P_(self.lp), lowp_code, st())
        elif self.entry == "amp":
            rc = lib().vk_adamw_step_amp(self.n, self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), *hyper,
                                         self.counter[1:].data_ptr(), 0.5, self.gs.data_ptr(), P_(found), self.scratch.data_ptr(), P_(self.lp),
                                         lowp_code, st())
        else:
            rc = lib().vk_adamw_step_amp_segments(1, self.seg.data_ptr(), self.nb, self.blocks.data_ptr(), self.p.data_ptr(), g.data_ptr(),
                                                  self.m.data_ptr(), self.v.data_ptr(), *hyper, self.counter.data_ptr(), 0.5, self.gs.data_ptr(),
                                                  P_(found), self.scratch.data_ptr(), st())
        L_.check(rc, self.entry)
        torch.cuda.synchronize()
        for nm, full in (("param", self.P), ("exp_avg", self.M), ("exp_avg_sq", self.V), ("grad", self.G), ("lowp", self.LP)):
            assert full is None or guards_ok(full), f"{self.entry}: {nm} written outside [0, n)"

    def counters(self):
        return self.counter.tolist()


def first_bad(got, want):
    bad = (got.double().cpu() != want.double().cpu()).nonzero()
    i = int(bad[0]) if len(bad) else -1
    return f"{len(bad)} of {got.numel()} wrong; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


@pytest.mark.parametrize("n", TC.ADAMW_SIZES)
@pytest.mark.parametrize("entry", ["step", "amp", "segments"])
def test_adamw_first_step_is_exact(entry, n):
    """EXACT_HP from zero moments: p, m and v equal float64 bit for bit; the 16-bit copy equals the rounded p; VK_F32 as the copy's type
    leaves a sentinel buffer untouched.  Second case: zero gradients with eps = 2^-20: pure decay, m = v = 0."""
    for zero_grad in (False, True):
        hp = dict(TC.EXACT_HP, eps=2.0 ** -20) if zero_grad else TC.EXACT_HP
        p0, gr = TC.exact_adamw_inputs(n, n, zero_grad)
        pe, me, ve = TC.exact_adamw_expected(p0, gr)
        g_in = gr * (2.0 if entry == "step" else 2048.0)                  # times the power of two the factor takes away again
        for lowp in ((None,) if entry == "segments" else (None, "bf16", "f16", "f32")):
            a = Adam(entry, p0, torch.zeros(n), torch.zeros(n), hp, 0, lowp)
            a.step(g_in)
            what = f"{entry} n {n} zero_grad {zero_grad} lowp {lowp}"
            assert torch.equal(a.p.cpu().double(), pe), f"{what}: p: " + first_bad(a.p, pe)
            assert torch.equal(a.m.cpu().double(), me), f"{what}: exp_avg: " + first_bad(a.m, me)
            assert torch.equal(a.v.cpu().double(), ve), f"{what}: exp_avg_sq: " + first_bad(a.v, ve)
            if lowp in ("bf16", "f16"):
                want = pe.float().to(TDT[lowp])
                assert torch.equal(a.lp.cpu(), want), f"{what}: copy: " + first_bad(a.lp.float(), want.float())
            elif lowp == "f32":
                assert bool((a.lp == SENTINEL).all()), f"{what}: a VK_F32 copy was written"
            assert a.counters() == ([0, 0, 0] if entry == "step" else [0, 1, 0]), a.counters()      # the counters either side stay


def test_adamw_segments_counter_layout():
    """The segment of test_adamw_first_step_is_exact names tensor_index 1: only that counter advances."""
    n = 257
    p0, gr = TC.exact_adamw_inputs(n, 1)
    a = Adam("segments", p0, torch.zeros(n), torch.zeros(n), TC.EXACT_HP, 0)
    a.counter.copy_(torch.tensor([5, 0, 9], dtype=torch.int32))
    a.step(gr * 2048.0)
    assert a.counters() == [5, 1, 9]


def check_adam_step(a, p0, m0, v0, gr, t, label, figs):
    pr, mr, vr = TC.adamw_ref(p0, gr, m0, v0, a.hp, t, a.factor)
    bp, bm, bv = TC.adamw_bounds(p0, gr, m0, v0, a.hp, t, a.factor)
    for nm, got, want, bound in (("p", a.p, pr, bp), ("exp_avg", a.m, mr, bm), ("exp_avg_sq", a.v, vr, bv)):
        err = (got.cpu().double() - want).abs()
        i = int((err - bound).argmax())
        figs[nm] = max(figs.get(nm, 0.0), float((err / bound).max()))
        assert bool(torch.isfinite(got).all()), f"{label}: {nm} not finite"
        assert bool((err <= bound).all()), (f"{label} step {t}: {nm}[{i}] (g {gr[i].item()!r}, p {p0[i].item()!r}, m {m0[i].item()!r}, v {v0[i].item()!r}): "
                                            f"got {got[i].item()!r}, want {want[i].item()!r}: error {err[i].item():.3e} > bound {bound[i].item():.3e}")


@pytest.mark.parametrize("hpname", ["default", "wd0"])
@pytest.mark.parametrize("t0", [1, 2, 10, 100000])
@pytest.mark.parametrize("entry", ["step", "amp", "segments"])
def test_adamw_five_steps_rounded(entry, t0, hpname):
    """Five steps from step number t0 (the `step` argument, or a preset device counter), each compared with float64 of torch's formula
    applied to the kernel's own previous state: p, exp_avg and exp_avg_sq, elementwise, under TC.adamw_bounds."""
    n = 10007
    hp = TC.DEFAULT_HP if hpname == "default" else dict(TC.DEFAULT_HP, wd=0.0)
    g = torch.Generator().manual_seed(t0)
    p0 = torch.randn(n, generator=g)
    m0 = torch.zeros(n) if t0 == 1 else torch.randn(n, generator=g) * 0.1
    v0 = torch.zeros(n) if t0 == 1 else torch.rand(n, generator=g) * 0.01
    a = Adam(entry, p0, m0, v0, hp, t0 - 1, "bf16" if entry == "amp" else None)
    figs = {}
    for k in range(5):
        t = t0 + k
        gr = TC.rounded_adamw_grad(n, 10 * t0 + k)
        g_in = gr * (2.0 if entry == "step" else 2048.0)                  # exact scalings (1e18 x 2048 stays finite)
        before = [x.cpu().clone() for x in (a.p, a.m, a.v)]
        a.t = t - 1
        a.step(g_in)
        check_adam_step(a, *before, g_in, t, f"{entry} {hpname}", figs)
        if entry == "amp":
            assert torch.equal(a.lp.cpu(), a.p.cpu().to(torch.bfloat16))
        if entry != "step":
            assert a.counters()[1] == t
    print(f"{entry} t0 {t0} {hpname}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in figs.items()))


@pytest.mark.parametrize("entry", ["step", "amp", "segments"])
def test_adamw_skip_rule(entry):
    """found_inf holding 1, -1 or NaN (any value != 0) skips the step: p, m, v and the 16-bit copy unwritten, every counter unchanged."""
    n = 4099
    g = torch.Generator().manual_seed(3)
    p0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    gr = torch.randn(n, generator=g)
    if entry == "step":
        flags = [torch.tensor([v], dtype=torch.int32, device=dev()) for v in (1, -1, 0x7FC00000)]
    else:
        flags = [torch.tensor([v], dtype=torch.float32, device=dev()) for v in (1.0, -1.0, float("nan"))]
    for fl in flags:
        a = Adam(entry, p0, m0, v0, TC.DEFAULT_HP, 6, None if entry == "segments" else "f16")
        a.counter.copy_(torch.tensor([3, 6, 4], dtype=torch.int32))
        keep = fl.clone()
        a.step(gr, fl)
        assert torch.equal(a.p.cpu(), p0) and torch.equal(a.m.cpu(), m0) and torch.equal(a.v.cpu(), v0), f"{entry}: a skipped step wrote its state"
        assert a.lp is None or bool((a.lp == SENTINEL).all())
        assert a.counters() == [3, 6, 4]
        assert torch.equal(fl.view(torch.int32), keep.view(torch.int32))       # the flag is the caller's to clear
    # and a zero flag takes the step
    zero = torch.zeros(1, dtype=torch.int32 if entry == "step" else torch.float32, device=dev())
    a = Adam(entry, p0, m0, v0, TC.DEFAULT_HP, 6)
    a.step(gr, zero)
    assert not torch.equal(a.p.cpu(), p0) and (entry == "step" or a.counters()[1] == 7)


def run_segments(segs, total, counters, hp, seed, found=None):
    """One call of vk_adamw_step_amp_segments over ragged segments of a sentinel-filled buffer.  Returns what is needed to judge it."""
    g = torch.Generator().manual_seed(seed)
    p0, m0, v0 = torch.randn(total, generator=g), torch.randn(total, generator=g) * 0.1, torch.rand(total, generator=g) * 0.01
    gr = TC.rounded_adamw_grad(total, seed)
    inside = torch.zeros(total, dtype=torch.bool)
    for b_, e_, _ in segs:
        inside[b_:e_] = True
    for t in (p0, m0, v0):
        t[~inside] = SENTINEL                                             # the gaps between segments hold sentinels
    P, p = guarded(p0)
    M, m = guarded(m0)
    V, v = guarded(v0)
    G, gd = guarded(gr * 2048.0)
    seg, blocks, nb = seg_tables(segs)
    cnt = torch.tensor(counters, dtype=torch.int32, device=dev())
    scratch = torch.zeros(4 + 2 * len(segs), device=dev())
    gs = torch.full((1,), 1024.0, device=dev())
    L_.check(lib().vk_adamw_step_amp_segments(len(segs), seg.data_ptr(), nb, blocks.data_ptr(), p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(),
                                              hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], cnt.data_ptr(), 0.5, gs.data_ptr(), P_(found),
                                              scratch.data_ptr(), st()), "vk_adamw_step_amp_segments")
    torch.cuda.synchronize()
    assert guards_ok(P) and guards_ok(M) and guards_ok(V) and guards_ok(G)
    return SimpleNamespace(p0=p0, m0=m0, v0=v0, g=gr * 2048.0, p=p.cpu(), m=m.cpu(), v=v.cpu(), inside=inside, counters=cnt.tolist())


def check_segments(segs, total, counters, r, hp, label):
    want_cnt = list(counters)
    for b_, e_, ti in segs:
        want_cnt[ti] += 1
        t = want_cnt[ti]
        sl = slice(b_, e_)
        pr, mr, vr = TC.adamw_ref(r.p0[sl], r.g[sl], r.m0[sl], r.v0[sl], hp, t, 2.0 ** -11)
        bp, bm, bv = TC.adamw_bounds(r.p0[sl], r.g[sl], r.m0[sl], r.v0[sl], hp, t, 2.0 ** -11)
        for nm, got, want, bound in (("p", r.p[sl], pr, bp), ("exp_avg", r.m[sl], mr, bm), ("exp_avg_sq", r.v[sl], vr, bv)):
            err = (got.double() - want).abs()
            i = int((err - bound).argmax())
            assert bool((err <= bound).all()), (f"{label}: segment [{b_}, {e_}) tensor {ti} step {t}: {nm}[{b_ + i}] (chunk {i // 4096}, {e_ - b_ - i} before the end): "
                                                f"error {err[i].item():.3e} > bound {bound[i].item():.3e}")
        assert not torch.equal(r.p[sl], r.p0[sl])
    out = ~r.inside
    assert bool((r.p[out] == SENTINEL).all()) and bool((r.m[out] == SENTINEL).all()) and bool((r.v[out] == SENTINEL).all()), f"{label}: a gap was written"
    assert r.counters == want_cnt, f"{label}: counters {r.counters}, want {want_cnt}"


def test_adamw_segments_ragged_lengths_gaps_and_counters():
    """Segments of 1 .. 12,289 elements at begins that are no multiples of 4, sentinel gaps between them, tensor_index in a shuffled order
    with a different preset counter each: every segment gets its own bias correction and only its own counter advances."""
    ranges, total = TC.ragged_segments(TC.SEGMENT_LENGTHS)
    order = [7, 2, 9, 0, 5, 11, 3, 8, 1]                                  # tensor_index per segment; 4, 6, 10 belong to no segment
    counters = [0, 1, 9, 99, 1234, 4, 77, 2, 99999, 0, 55, 3]
    segs = [(b_, e_, ti) for (b_, e_), ti in zip(ranges, order)]
    r = run_segments(segs, total, counters, TC.DEFAULT_HP, 21)
    check_segments(segs, total, counters, r, TC.DEFAULT_HP, "ragged")
    # skipped: nothing moves
    nanflag = torch.full((1,), float("nan"), device=dev())
    r = run_segments(segs, total, counters, TC.DEFAULT_HP, 21, nanflag)
    assert torch.equal(r.p, r.p0) and torch.equal(r.m, r.m0) and torch.equal(r.v, r.v0) and r.counters == counters


def test_adamw_300_single_chunk_segments():
    """More segments than the 256 threads of k_adamw_prepare: its loop takes a second trip."""
    lengths = [1 + (i * 37) % 61 for i in range(300)]
    ranges, total = TC.ragged_segments(lengths)
    perm = [(i * 7) % 300 for i in range(300)]                            # 7 is coprime to 300: a permutation
    counters = [(i * 13) % 50 for i in range(300)]
    segs = [(b_, e_, ti) for (b_, e_), ti in zip(ranges, perm)]
    r = run_segments(segs, total, counters, TC.DEFAULT_HP, 22)
    check_segments(segs, total, counters, r, TC.DEFAULT_HP, "300 segments")


def test_adamw_segments_equal_the_whole_buffer_kernel_at_2e20():
    """n = 2^20 + 3 (past the 1,048,576-thread cap of the whole-buffer kernel, whose loop takes a second trip) cut into ragged adjacent
    segments with equal counters: the four entry points (vk_adamw_step, vk_adamw_step_amp, vk_adamw_step_amp_segments, vk_adamw_step_groups
    with one group and no coefficient) agree bit for bit on p, exp_avg and exp_avg_sq over two steps from the same state at the same step
    number with the same factor 2^-11, and the bf16 copies of the two whole-buffer entries agree.  Every entry runs one element
    function; this is the test that ties the grid-stride loop of the whole-buffer kernel to the block-table loop of the per-tensor one."""
    n = 2 ** 20 + 3
    g = torch.Generator().manual_seed(23)
    p0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-3
    gr = torch.randn(n, generator=g) * 100.0
    cuts = [0, 1, 3, 258, 4354, 8450, 12547, 300000, 300001, 777777, n - 4097, n - 1, n]
    segs = [(cuts[i], cuts[i + 1], i) for i in range(len(cuts) - 1)]
    seg, blocks, nb = seg_tables(segs)
    hyper = (5e-5, 0.9, 0.999, 1e-8, 1e-4)
    names = ("step", "amp", "segments", "groups")
    S = {e: [guarded(t) for t in (p0, gr, m0, v0)] for e in names}
    ptrs = {e: [v.data_ptr() for _, v in S[e]] for e in names}
    LP = {e: guarded(torch.full((n,), SENTINEL).to(torch.bfloat16)) for e in ("step", "amp")}
    step_amp = torch.full((1,), 4, dtype=torch.int32, device=dev())
    steps = {e: torch.full((len(segs),), 4, dtype=torch.int32, device=dev()) for e in ("segments", "groups")}
    scr_amp = torch.zeros(4, device=dev())
    scr = {e: torch.zeros(4 + 2 * len(segs), device=dev()) for e in ("segments", "groups")}
    gs = torch.full((1,), 1024.0, device=dev())
    seg_group = torch.zeros(len(segs), dtype=torch.int32, device=dev())
    groups = (L_.vk_adamw_group * 1)(L_.vk_adamw_group(*hyper))
    for k in range(2):
        L_.check(lib().vk_adamw_step(n, *ptrs["step"], *hyper, 5 + k, 2.0 ** -11, None, LP["step"][1].data_ptr(), L_.VK_BF16, st()))
        L_.check(lib().vk_adamw_step_amp(n, *ptrs["amp"], *hyper, step_amp.data_ptr(), 0.5, gs.data_ptr(), None, scr_amp.data_ptr(),
                                         LP["amp"][1].data_ptr(), L_.VK_BF16, st()))
        L_.check(lib().vk_adamw_step_amp_segments(len(segs), seg.data_ptr(), nb, blocks.data_ptr(), *ptrs["segments"], *hyper,
                                                  steps["segments"].data_ptr(), 0.5, gs.data_ptr(), None, scr["segments"].data_ptr(), st()))
        L_.check(lib().vk_adamw_step_groups(len(segs), seg.data_ptr(), seg_group.data_ptr(), nb, blocks.data_ptr(), *ptrs["groups"], 1, groups,
                                            steps["groups"].data_ptr(), 0.5, gs.data_ptr(), None, None, scr["groups"].data_ptr(), st()))
        torch.cuda.synchronize()
        for e in names:
            for nm, (fa, va), (fb, vb) in zip(("p", "grad", "exp_avg", "exp_avg_sq"), S["amp"], S[e]):
                assert guards_ok(fb), f"{e}: {nm} written outside [0, n)"
                assert torch.equal(va, vb), f"step {k}: {e} against amp: {nm}: " + first_bad(vb, va)
        assert guards_ok(LP["step"][0]) and guards_ok(LP["amp"][0])
        assert torch.equal(LP["step"][1], LP["amp"][1]), f"step {k}: bf16 copy: " + first_bad(LP["step"][1].float(), LP["amp"][1].float())
        assert torch.equal(LP["amp"][1], S["amp"][0][1].to(torch.bfloat16))
    assert step_amp.item() == 6 and steps["segments"].tolist() == [6] * len(segs) and steps["groups"].tolist() == [6] * len(segs)
    assert not torch.equal(S["amp"][0][1].cpu(), p0)


# ================================================================================================ GradScaler kernels
def poison_places(n, second_trip):
    """Element 0, each lane of the first and of a later 16-byte vector, the last element, and one reached only on the second grid trip."""
    return sorted({0, 1, 2, 3, 4 * 77 + 0, 4 * 77 + 1, 4 * 77 + 2, 4 * 77 + 3, n - 1, second_trip} & set(range(n)))


@pytest.mark.parametrize("n", [8, 4 * 257, 2 ** 22 + 4])
def test_amp_unscale_check_finds_every_poisoned_place(n):
    """n = 2^22 + 4: n / 4 is past the 1,048,576 threads of the launch, so the last vector is reached on a second trip."""
    g = torch.Generator().manual_seed(n)
    base = torch.randint(-1000, 1001, (n,), generator=g).float()
    Gf, gd = guarded(base)
    found = torch.zeros(1, device=dev())
    one = torch.ones(1, device=dev())
    for inv in (None, one):
        L_.check(lib().vk_amp_unscale_check(n, gd.data_ptr(), P_(inv), found.data_ptr(), st()))
        torch.cuda.synchronize()
        assert found.item() == 0.0 and torch.equal(gd.cpu(), base) and guards_ok(Gf)
    for place in poison_places(n, 4 * 2 ** 20 + 2):
        for bad in (float("inf"), float("-inf"), float("nan")):
            gd[place] = bad
            found.zero_()
            L_.check(lib().vk_amp_unscale_check(n, gd.data_ptr(), None, found.data_ptr(), st()))
            torch.cuda.synchronize()
            assert found.item() == 1.0, f"{bad} at element {place} (vector {place // 4}, lane {place % 4}) of {n} not found"
            gd[place] = base[place]
    # a clean call never clears the flag
    L_.check(lib().vk_amp_unscale_check(n, gd.data_ptr(), None, found.data_ptr(), st()))
    torch.cuda.synchronize()
    assert found.item() == 1.0 and torch.equal(gd.cpu(), base) and guards_ok(Gf)
    # inv = 2^-16 on the exact grid equals float64
    inv = torch.full((1,), 2.0 ** -16, device=dev())
    found.zero_()
    L_.check(lib().vk_amp_unscale_check(n, gd.data_ptr(), inv.data_ptr(), found.data_ptr(), st()))
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu().double(), base.double() * 2.0 ** -16), first_bad(gd, base.double() * 2.0 ** -16)
    assert found.item() == 0.0 and guards_ok(Gf)
    assert lib().vk_amp_unscale_check(n - 1, gd.data_ptr(), None, found.data_ptr(), st()) < 0
    assert lib().vk_amp_unscale_check(n - 4, gd[1:].data_ptr(), None, found.data_ptr(), st()) < 0       # not 16-byte aligned


def test_amp_unscale_check_factor_one_keeps_every_bit_and_subnormals_follow_ieee():
    bits = torch.tensor([0x7FC01234, -0x7FEDCBAA, -0x80000000, 0x00000001, 0x007FFFFF, 0x3F800000, 0x7F800000, 0x00000000],
                        dtype=torch.int32).repeat(16)                      # NaN payloads (both signs), -0, subnormals, 1, inf, 0
    Gf, gd = guarded(bits.view(torch.float32))
    found = torch.zeros(1, device=dev())
    one = torch.ones(1, device=dev())
    L_.check(lib().vk_amp_unscale_check(bits.numel(), gd.data_ptr(), one.data_ptr(), found.data_ptr(), st()))
    torch.cuda.synchronize()
    assert torch.equal(gd.view(torch.int32).cpu(), bits) and found.item() == 1.0 and guards_ok(Gf)
    # subnormal results: odd multiples of 2^-125 times 2^-16 need rounding to the subnormal grid (ties to even), IEEE 754
    # k x 2^-140 (normal numbers) times 2^-16 = (k / 128) x 2^-149: odd k never fits the subnormal grid, k = 128 m + 64 is a tie
    k = 2.0 ** 15 + torch.arange(0, 128, dtype=torch.float64) * 2.0 + 1.0
    ties = 128.0 * torch.arange(300, 364, dtype=torch.float64) + 64.0
    src = (torch.cat([k, -k, ties, -ties]) * 2.0 ** -140).float()
    assert src.numel() % 4 == 0 and bool((src.abs() >= 2.0 ** -126).all())
    want = (src.double() * 2.0 ** -16).float()                             # one rounding of the exact product
    assert bool((want != 0).all()) and bool((want.double() != src.double() * 2.0 ** -16).all())        # every result is an inexact subnormal
    Gf, gd = guarded(src)
    inv = torch.full((1,), 2.0 ** -16, device=dev())
    found.zero_()
    L_.check(lib().vk_amp_unscale_check(src.numel(), gd.data_ptr(), inv.data_ptr(), found.data_ptr(), st()))
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu().view(torch.int32), want.view(torch.int32)), "subnormal products: " + first_bad(gd, want)
    assert found.item() == 0.0


@pytest.mark.parametrize("n", [1, 5, 1027, 2 ** 20 + 3])
def test_amp_check_inf_finds_every_poisoned_place(n):
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g)
    Gf, gd = guarded(base)
    found = torch.zeros(3, dtype=torch.int32, device=dev())
    L_.check(lib().vk_amp_check_inf(n, gd.data_ptr(), found[1:].data_ptr(), st()))
    torch.cuda.synchronize()
    assert found.tolist() == [0, 0, 0]
    for place in poison_places(n, 2 ** 20 + 1):
        for bad in (float("inf"), float("-inf"), float("nan")):
            gd[place] = bad
            found.zero_()
            L_.check(lib().vk_amp_check_inf(n, gd.data_ptr(), found[1:].data_ptr(), st()))
            torch.cuda.synchronize()
            assert found.tolist() == [0, 1, 0], f"{bad} at element {place} of {n}: found {found.tolist()}"
            gd[place] = base[place]
    L_.check(lib().vk_amp_check_inf(n, gd.data_ptr(), found[1:].data_ptr(), st()))       # clean: the flag is not cleared
    torch.cuda.synchronize()
    assert found.tolist() == [0, 1, 0] and torch.equal(gd.cpu(), base) and guards_ok(Gf)
