"""The convolution kernels (csrc/conv_halo.hip, conv_igemm.hip, conv_wgrad.hip, wgrad_halo.hip, conv1x1.hip) through the C ABI against
float64, on the integer lattice of tests/conv_lattice.py.

EXACT tier.  Operands are small integers, ternary weights, prologue scales from {0.5, 1, 2} and integer shifts that differ from channel to
channel; every kernel accumulates in fp32, so every partial sum is exact whatever its order and the comparison with float64 is EQUALITY of
every element, in f32, bf16 and f16, on every path a case can take (tile shapes, persistent / pipelined / staggered forms, streaming
kernels and their strip heights, the tap-by-tap kernel, split-K counts, slab and atomics epilogues): the paths of one case therefore also
agree with each other bit for bit, and a second run gives the same bits.  BatchNorm statistics and BN-backward sums are compared as
integers in fp64.  Paths are selected with monkeypatch.setenv only; a test runs all paths of its (case, type) and reports every path that
differs, with the first wrong pixel, its channel, 16-byte vector and 8 x 16 tile.  tests/test_conv_lattice_cpu.py proves, on the reference
alone, that each case meets the conditions under which equality must hold.

Shapes: H != W in both orientations on every entry point, extents around the 8 x 16 tile and the 128-pixel tile (H from 1, 2, 3, 7, 8, 9,
17, W from 1, 2, 15, 16, 17, 31, 33, 130), N in 1, 2, 3, 5 so that images end inside a tile, maps smaller than a tile and than the halo,
channel counts that are multiples of the chunk but not of the tile, and counts outside the documented set: there a call either returns
VK_OK with the exact result or a negative code with its sentinel-filled outputs untouched.

ROUNDED tier (thin shape list).  Seeded normal inputs rounded to the type, random per-channel coefficients, and an elementwise bound that is
derived, not tuned (see bound()): store 2 u_T |ref| + the subnormal spacing, plus (fp32 additions in the chain) x 2^-23 x conv(|V|, |w|)."""
import ctypes as C
import functools
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import conv_lattice as CL

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
DT = CL.TDT
CODE = {"f32": L_.VK_F32, "bf16": L_.VK_BF16, "f16": L_.VK_F16}
U = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}      # unit round-off of the stored type
SUB = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133, "f16": 2.0 ** -24}  # spacing of the type's subnormals
VE = {"f32": 4, "bf16": 8, "f16": 8}                               # elements of a 16-byte vector
REPL = 32                                                          # VK_STATS_REPLICAS
SENTINEL = 77.0                                                    # exact in every type; no lattice result is checked against it by accident
WS_BYTES = 64 << 20                                                # VK_WGRAD_WORKSPACE_BYTES
SPLITK_BYTES = 32 << 20                                            # VK_SPLITK_WORKSPACE_BYTES
ENV_KEYS = ["VK_COL_ALT", "VK_COL_PIPE", "VK_COL_PERSIST", "VK_COL_PERSIST_GRID", "VK_STREAM_RS", "VK_NO_STREAM", "VK_COL_NO_KYFAST",
            "VK_NO_S2_TILE", "VK_NO_HALO", "VK_SPLITK", "VK_NO_SPLITK", "VK_IGEMM_NO_PARITY", "VK_NO_WGRAD_HALO",
            "VK_WH_MINBLOCKS", "VK_WH_MAXCOMBO", "VK_WGRAD_ATOMICS", "VK_WH_NO_TS", "VK_WH_BLOCKS", "VK_WS_KW", "VK_NO_WSTREAM",
            "VK_WH_NO_SLAB", "VK_NO_STEM_TILE", "VK_STEM_WGRAD_TAPS"]


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return vk.lib()


def set_env(mp, env):
    for k in ENV_KEYS:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


@functools.lru_cache(maxsize=4)
def built(case):
    return CL.build(case)


def nhwc(t, dt):
    """NCHW float64 (CPU) -> NHWC of the element type on the device."""
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())


def krsc(w, dt):
    """[out][red][R][S] float64 (CPU) -> [out][R][S][red] of the element type on the device."""
    return w.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())


def fvec(t):
    return None if t is None else t.float().to(dev())


def P_(t):
    return None if t is None else t.data_ptr()


def filled(shape, dt, value=SENTINEL):
    return torch.full(shape, value, dtype=dt, device=dev())


def src_of(case, b, dt, keep):
    out = []
    for s, x, sc, sh in zip(case.srcs, b.x, b.scale, b.shift):
        xd, scd, shd = nhwc(x, dt), fvec(sc), fvec(sh)
        keep += [xd, scd, shd]
        out.append(L_.vk_src(xd.data_ptr(), s.C, s.up, P_(scd), P_(shd), 1 if s.pro else 0))
    if len(out) == 1:
        out.append(L_.vk_src(None, 0, 0, None, None, 0))
    return out


def desc_of(case, dtn, s0, s1, transposed=0):
    Ho, Wo = case.out_hw
    if transposed:      # the source is dz on the forward's output grid, the result has the forward's input grid
        return L_.vk_conv_desc(CODE[dtn], case.N, Ho, Wo, case.H, case.W, case.K, case.R, case.R, case.stride, case.pad, 1, s0, s1)
    return L_.vk_conv_desc(CODE[dtn], case.N, case.H, case.W, Ho, Wo, case.K, case.R, case.R, case.stride, case.pad, 0, s0, s1)


def weights_for(d, w_plain, keep):
    """(pointer, packed) under the CURRENT environment: the halo pack where vk_conv_uses_halo_pack says so, plain weights otherwise."""
    if not lib().vk_conv_uses_halo_pack(C.byref(d)):
        return w_plain, 0
    red = d.src0.C + (d.src1.C if d.src1.ptr else 0)
    pk = torch.empty_like(w_plain)
    keep.append(pk)
    L_.check(lib().vk_halo_pack(d.dtype, d.K, red, w_plain.data_ptr(), pk.data_ptr(), st()), "vk_halo_pack")
    return pk, 1


def where_bad(got, ref, dtn):
    """got, ref: NCHW float64 on the CPU.  Count, first wrong pixel, channel, 16-byte vector, 8 x 16 tile."""
    bad = got != ref
    if not bool(bad.any()):
        return None
    n, c, h, w = (int(v) for v in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements wrong; first at image {n} pixel ({h}, {w}) channel {c} (vector {c // VE[dtn]}, "
            f"tile ({h // 8}, {w // 16})): got {got[n, c, h, w].item()!r}, want {ref[n, c, h, w].item()!r}")


def diff(errors, path, what, got_nhwc, ref_nchw, dtn):
    msg = where_bad(got_nhwc.double().cpu().permute(0, 3, 1, 2), ref_nchw, dtn)
    if msg:
        errors.append(f"[{path}] {what}: {msg}")


def diff_sums(errors, path, what, sums_dev, ref2):
    """Partial sums spread over the replicas, as integers in fp64."""
    got = sums_dev.view(REPL, 2, -1).sum(0).cpu()
    for i, name in enumerate(("sum", "sum of products")):
        bad = got[i] != ref2[i]
        if bool(bad.any()):
            c = int(bad.nonzero()[0])
            errors.append(f"[{path}] {what} {name}: {int(bad.sum())} of {bad.numel()} channels wrong; first channel {c}: got {got[i, c].item()!r}, "
                          f"want {ref2[i, c].item()!r}")


def documented(case):
    """The channel counts and extents the operator-level entry points document (include/vk_unet.h, and the argument checks of
    vk_conv_fwd / vk_conv_wgrad): every source a multiple of 32 channels, or a single source of 16; K a multiple of 16; even maps under an
    upsampled source or a 2 x 2 pooled output."""
    cs = [s.C for s in case.srcs]
    chan = all(c % 32 == 0 for c in cs) or cs == [16]
    even = case.H % 2 == 0 and case.W % 2 == 0
    return chan and case.K % 16 == 0 and case.K >= 16 and (even or not (any(s.up for s in case.srcs) or case.pool2))


def settled(rc, case, outputs, errors, path, may_refuse=False):
    """True when the call ran.  A refusal must be negative, must not concern a documented shape, and must leave every (tensor, untouched
    copy) of `outputs` as it was."""
    torch.cuda.synchronize()
    print(f"{case.kind} {case.name}: [{path}] {'ran' if rc == 0 else 'returned %d' % rc}")      # pytest -rP: which paths of a case executed
    if rc == 0:
        return True
    if rc > 0:
        pytest.fail(f"[{path}] {case.name}: hipError {rc}: {lib().vk_last_error_string().decode(errors='replace')}")
    if documented(case) and not may_refuse:
        errors.append(f"[{path}] documented shape refused with {rc}: {lib().vk_last_error_string().decode(errors='replace')}")
    for t, t0 in outputs:
        if not torch.equal(t, t0):
            errors.append(f"[{path}] refused with {rc} but wrote an output")
    return False


def agree(errors, outs, what):
    """All paths that ran produced the same bits."""
    names = list(outs)
    for nm in names[1:]:
        if not torch.equal(outs[names[0]], outs[nm]):
            errors.append(f"{what}: path {nm} differs from path {names[0]} bit for bit")


def ids(cases):
    return [c.name for c in cases]


def typed(cases):
    return [pytest.param(c, t, id=f"{c.name}-{t}") for c in cases for t in c.types]


# ------------------------------------------------------------------------------------------------ forward
def fwd_paths(case, dtn):
    """name -> environment.  Every path goes through vk_conv_fwd_packed where vk_conv_uses_halo_pack says the descriptor runs on the tile
    kernels under that environment and through vk_conv_fwd with plain weights otherwise (the streaming and C = 16 kernels take plain
    weights); `igemm` is always the tap-by-tap implicit-GEMM kernel."""
    one = {"VK_COL_PERSIST": "0"}
    paths = {"igemm": {"VK_NO_HALO": "1"}, "default": {}, "tile": one}
    if case.stride == 2:
        paths["no_s2_tile"] = {"VK_NO_S2_TILE": "1"}
        return paths
    if case.R != 3:
        return paths
    if case.K >= 128:
        for alt in "2378":
            paths[f"tile_alt{alt}"] = dict(one, VK_COL_ALT=alt)
        for alt in "27":
            paths[f"tile_alt{alt}_plain"] = dict(one, VK_COL_ALT=alt, VK_COL_PIPE="0")
            paths[f"tile_alt{alt}_stag"] = dict(one, VK_COL_ALT=alt, VK_COL_PIPE="2")
        paths["no_kyfast"] = dict(one, VK_COL_NO_KYFAST="1")
    else:
        paths["tile_persist"] = {"VK_COL_PERSIST": "2", "VK_COL_PERSIST_GRID": "3"}
    if dtn != "f32" and case.C in (16, 32):
        for rs in ("8", "24", "64"):
            paths[f"stream_rs{rs}"] = {"VK_STREAM_RS": rs}
        paths["no_stream"] = dict(one, VK_NO_STREAM="1")
    return paths


def run_fwd(case, dtn, mp, paths=None, with_stats=True):
    b = built(case)
    dt = DT[dtn]
    keep, errors, outs = [], [], {}
    s0, s1 = src_of(case, b, dt, keep)
    d = desc_of(case, dtn, s0, s1)
    wd = krsc(b.w, dt)
    Ho, Wo = case.out_hw
    for path, env in (paths or fwd_paths(case, dtn)).items():
        set_env(mp, env)
        wp, packed = weights_for(d, wd, keep)
        y = filled((case.N, Ho, Wo, case.K), dt)
        y0 = y.clone()
        stats = torch.zeros(REPL * 2 * case.K, dtype=torch.float64, device=dev()) if with_stats else None
        fn = lib().vk_conv_fwd_packed if packed else lib().vk_conv_fwd
        rc = fn(C.byref(d), wp.data_ptr(), y.data_ptr(), None, 0, 0, P_(stats), st())
        if not settled(rc, case, [(y, y0)] + ([(stats, torch.zeros_like(stats))] if with_stats else []), errors, path):
            continue
        diff(errors, path, "y", y, b.y, dtn)
        if with_stats:
            diff_sums(errors, path, "stats", stats, b.stats)
        outs[path] = y
    agree(errors, outs, "y")
    assert not errors, f"vk_conv_fwd {case.name} {dtn}:\n" + "\n".join(errors)
    return outs


@pytest.mark.parametrize("case,dtn", typed(CL.fwd_cases()))
def test_conv_fwd_exact(case, dtn, monkeypatch):
    """vk_conv_fwd / vk_conv_fwd_packed with `stats`, with and without the BN+ReLU prologue, up + concat, stride 2 (3x3 and 1x1): equality
    with float64 on every path of fwd_paths()."""
    outs = run_fwd(case, dtn, monkeypatch)
    assert outs, "no path ran"


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.large_cases() if c.kind == "fwd"]))
def test_conv_fwd_exact_large(case, dtn, monkeypatch):
    """Full-network layer shapes (3x3 stride 1, up + concat, stride 2): grid-stride and persistent loops take more than one trip (tile
    counts in conv_lattice.large_cases).  The default route, the one-tile form and the tap-by-tap kernel."""
    run_fwd(case, dtn, monkeypatch, paths={"default": {}, "tile": {"VK_COL_PERSIST": "0"}, "igemm": {"VK_NO_HALO": "1"}})


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.outside_cases() if c.kind == "fwd"]))
def test_conv_fwd_outside_documented_set(case, dtn, monkeypatch):
    """C = 8, 24, 40, K = 8, 24, 40 and an upsampled source under an odd map: refused with the output untouched, or exact."""
    if case.name == "out_up_odd":
        b = built(case)
        dt = DT[dtn]
        x = nhwc(b.x[0][:, :, :case.H // 2 + 1, :case.W // 2 + 1], dt)
        d = desc_of(case, dtn, L_.vk_src(x.data_ptr(), 32, 1, None, None, 0), L_.vk_src(None, 0, 0, None, None, 0))
        wd = krsc(b.w, dt)
        for env in ({}, {"VK_NO_HALO": "1"}):
            set_env(monkeypatch, env)
            y = filled((case.N, case.H, case.W, case.K), dt)
            rc = lib().vk_conv_fwd(C.byref(d), wd.data_ptr(), y.data_ptr(), None, 0, 0, None, st())
            torch.cuda.synchronize()
            assert rc < 0 and bool((y == SENTINEL).all()), rc
        return
    run_fwd(case, dtn, monkeypatch)


@pytest.mark.parametrize("case,dtn", typed(CL.splitk_cases()))
def test_conv_fwd_splitk_exact(case, dtn, monkeypatch):
    """vk_conv_fwd_splitk: VK_SPLITK auto / 2 / 5 / 32 / disabled / no workspace.  With exact sums all give the same bits, twice."""
    b = built(case)
    dt = DT[dtn]
    keep, errors, outs = [], [], {}
    s0, s1 = src_of(case, b, dt, keep)
    d = desc_of(case, dtn, s0, s1)
    set_env(monkeypatch, {})
    wp, packed = weights_for(d, krsc(b.w, dt), keep)
    assert packed
    ws = torch.empty(SPLITK_BYTES, dtype=torch.uint8, device=dev())
    for path, env, wsp in [("auto", {}, ws), ("ks2", {"VK_SPLITK": "2"}, ws), ("ks5", {"VK_SPLITK": "5"}, ws), ("ks32", {"VK_SPLITK": "32"}, ws),
                           ("off", {"VK_NO_SPLITK": "1"}, ws), ("no_ws", {}, None), ("small_ws", {"VK_SPLITK": "32"}, ws[:3 * case.N * case.H * case.W * case.K * 4])]:
        set_env(monkeypatch, env)
        for rep in range(2):
            y = filled((case.N, case.H, case.W, case.K), dt)
            rc = lib().vk_conv_fwd_splitk(C.byref(d), wp.data_ptr(), y.data_ptr(), P_(wsp), wsp.numel() if wsp is not None else 0, st())
            torch.cuda.synchronize()
            assert rc == 0, (path, rc)
            diff(errors, f"{path}#{rep}", "y", y, b.y, dtn)
            outs[f"{path}#{rep}"] = y
    agree(errors, outs, "y")
    assert not errors, f"vk_conv_fwd_splitk {case.name} {dtn}:\n" + "\n".join(errors)


# ------------------------------------------------------------------------------------------------ data gradient
def dgrad_paths(case, dtn):
    one = {"VK_COL_PERSIST": "0"}
    paths = {"igemm": {"VK_NO_HALO": "1"}, "default": {}, "tile": one}
    if case.stride == 2:
        paths["igemm_no_parity"] = {"VK_NO_HALO": "1", "VK_IGEMM_NO_PARITY": "1"}
        paths["no_s2_tile"] = {"VK_NO_S2_TILE": "1"}
        paths["no_s2_tile_no_parity"] = {"VK_NO_S2_TILE": "1", "VK_IGEMM_NO_PARITY": "1"}
        return paths
    if case.R != 3:
        return paths
    if case.K >= 128:
        for alt in "2378":
            paths[f"tile_alt{alt}"] = dict(one, VK_COL_ALT=alt)
    else:
        paths["tile_persist"] = {"VK_COL_PERSIST": "2", "VK_COL_PERSIST_GRID": "3"}
    return paths


def run_dgrad(case, dtn, mp, paths=None):
    """vk_conv_fwd[_packed] with transposed = 1: plain store into a sentinel-filled buffer, `accumulate` onto integers already there and
    onto the result itself (2 x the gradient), channel split."""
    b = built(case)
    dt = DT[dtn]
    keep, errors, outs = [], [], {}
    dzd = nhwc(b.dz, dt)
    d = desc_of(case, dtn, L_.vk_src(dzd.data_ptr(), case.srcs[0].C, 0, None, None, 0), L_.vk_src(None, 0, 0, None, None, 0), 1)
    wd = krsc(b.w, dt)
    k0 = case.split or case.K
    plain_ref = b.dx[:, :k0]
    for path, env in (paths or dgrad_paths(case, dtn)).items():
        set_env(mp, env)
        wp, packed = weights_for(d, wd, keep)
        fn = lib().vk_conv_fwd_packed if packed else lib().vk_conv_fwd
        y = filled((case.N, case.H, case.W, k0), dt)
        y1 = filled((case.N, case.H, case.W, case.K - k0), dt) if case.split else None
        touched = [(y, y.clone())] + ([(y1, y1.clone())] if case.split else [])
        rc = fn(C.byref(d), wp.data_ptr(), y.data_ptr(), P_(y1), case.split, 0, None, st())
        if not settled(rc, case, touched, errors, path):
            continue
        diff(errors, path, "dx", y, plain_ref, dtn)
        if case.split:
            diff(errors, path, "dx (skip part)", y1, b.y1, dtn)
        outs[path] = y
        if case.accumulate:
            rc = fn(C.byref(d), wp.data_ptr(), y.data_ptr(), None, 0, 1, None, st())
            torch.cuda.synchronize()
            assert rc == 0, (path, rc)
            diff(errors, path, "dx accumulated onto itself", y, 2 * b.dx, dtn)
            yo = nhwc(b.old, dt)
            rc = fn(C.byref(d), wp.data_ptr(), yo.data_ptr(), None, 0, 1, None, st())
            torch.cuda.synchronize()
            assert rc == 0, (path, rc)
            diff(errors, path, "dx accumulated onto integers", yo, b.y, dtn)
    agree(errors, outs, "dx")
    assert not errors, f"data gradient {case.name} {dtn}:\n" + "\n".join(errors)
    return outs


@pytest.mark.parametrize("case,dtn", typed(CL.dgrad_cases()))
def test_conv_dgrad_exact(case, dtn, monkeypatch):
    """Stride 1; stride 2 with the 3x3 and 1x1 parity kernels, the tile data-gradient kernel and VK_IGEMM_NO_PARITY / VK_NO_S2_TILE;
    accumulate; split at several k1."""
    assert run_dgrad(case, dtn, monkeypatch) or not documented(case), "no path ran"


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.large_cases() if c.kind == "dgrad" and not c.bnr]))
def test_conv_dgrad_exact_large(case, dtn, monkeypatch):
    run_dgrad(case, dtn, monkeypatch, paths={"default": {}, "tile": {"VK_COL_PERSIST": "0"}, "igemm": {"VK_NO_HALO": "1"}})


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.outside_cases() if c.kind == "dgrad"]))
def test_conv_dgrad_outside_documented_set(case, dtn, monkeypatch):
    run_dgrad(case, dtn, monkeypatch)


def fused_paths(case, dtn):
    paths = {"one_tile": {"VK_COL_PERSIST": "0"}, "persistent": {"VK_COL_PERSIST": "2", "VK_COL_PERSIST_GRID": "3"}, "default": {}}
    if dtn != "f32" and case.srcs[0].C in (16, 32):
        paths["stream_rs8"] = {"VK_STREAM_RS": "8"}
        paths["stream_rs24"] = {"VK_STREAM_RS": "24"}
        paths["no_stream"] = {"VK_COL_PERSIST": "0", "VK_NO_STREAM": "1"}
    return paths


def run_fused(case, dtn, mp, paths=None, force_pool2=None):
    """vk_conv_dgrad_fused (and vk_conv_dgrad_pool2 where there is no bnr) on one case, every path."""
    b = built(case)
    dt = DT[dtn]
    keep, errors, outs = [], [], {}
    pool2 = case.pool2 if force_pool2 is None else force_pool2
    dzd = nhwc(b.dz, dt)
    d = desc_of(case, dtn, L_.vk_src(dzd.data_ptr(), case.srcs[0].C, 0, None, None, 0), L_.vk_src(None, 0, 0, None, None, 0), 1)
    wd = krsc(b.w, dt)
    k0 = case.split or case.K
    Hy, Wy = (case.H // 2, case.W // 2) if pool2 else (case.H, case.W)
    zd = nhwc(b.z, dt) if case.bnr else None
    md = nhwc(b.mask, dt) if case.bnr == "mask" else None
    scd, shd = fvec(b.bn_scale), fvec(b.bn_shift)
    # a 16-channel reduction in a 16-bit type runs the C = 16 kernels, which have no external-mask epilogue (the network has no such layer)
    may_refuse = (case.bnr == "mask" and case.srcs[0].C == 16 and dtn != "f32") or force_pool2 is not None
    entries = ["fused"] + (["pool2"] if pool2 and not case.bnr else [])
    for path, env in (paths or fused_paths(case, dtn)).items():
        set_env(mp, env)
        wp, _ = weights_for(d, wd, keep)
        for entry in entries:
            y = nhwc(b.old, dt) if case.accumulate else filled((case.N, Hy, Wy, k0), dt)
            # vk_bnr.accumulate adds into both parts: y1 starts from integers of its own, so a kernel that stores there instead is seen
            y1 = (nhwc(b.old1, dt) if case.accumulate else filled((case.N, case.H, case.W, case.K - k0), dt)) if case.split else None
            sums = torch.zeros(REPL * 2 * k0, dtype=torch.float64, device=dev()) if case.bnr else None
            touched = [(y, y.clone())] + ([(y1, y1.clone())] if case.split else []) + ([(sums, torch.zeros_like(sums))] if case.bnr else [])
            if entry == "pool2":
                rc = lib().vk_conv_dgrad_pool2(C.byref(d), wp.data_ptr(), y.data_ptr(), P_(y1), case.split, 0, st())
            else:
                bnr = L_.vk_bnr(zd.data_ptr(), P_(scd), P_(shd), sums.data_ptr(), P_(md), case.accumulate) if case.bnr else None
                rc = lib().vk_conv_dgrad_fused(C.byref(d), wp.data_ptr(), y.data_ptr(), P_(y1), case.split, pool2, C.byref(bnr) if bnr else None, st())
            name = f"{path}/{entry}"
            if not settled(rc, case, touched, errors, name, may_refuse):
                continue
            assert force_pool2 is None, "an odd map was pooled"
            diff(errors, name, "y", y, b.y, dtn)
            if case.split:
                diff(errors, name, "y1", y1, b.y1, dtn)
            if case.bnr:
                diff_sums(errors, name, "bnr sums", sums, b.sums)
            outs[name] = y
            if entry == "pool2":        # its own `accumulate`: both parts are added to integers already there
                g = torch.Generator().manual_seed(11)
                old, old1 = CL.ints(tuple(b.y.shape), -2, 2, g), (CL.ints(tuple(b.y1.shape), -2, 2, g) if case.split else None)
                assert CL.exact_in(b.y + old, dtn) and (old1 is None or CL.exact_in(b.y1 + old1, dtn))       # on the reference alone
                ya, y1a = nhwc(old, dt), (nhwc(old1, dt) if case.split else None)
                rc = lib().vk_conv_dgrad_pool2(C.byref(d), wp.data_ptr(), ya.data_ptr(), P_(y1a), case.split, 1, st())
                torch.cuda.synchronize()
                assert rc == 0, (name, rc)
                diff(errors, name, "y accumulated", ya, b.y + old, dtn)
                if case.split:
                    diff(errors, name, "y1 accumulated", y1a, b.y1 + old1, dtn)
    agree(errors, outs, "y")
    assert not errors, f"vk_conv_dgrad_fused {case.name} {dtn}:\n" + "\n".join(errors)
    return outs


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.fused_cases() if c.name != "pool_odd_9x17"]))
def test_conv_dgrad_fused_exact(case, dtn, monkeypatch):
    """Every combination the header allows of pool2 / bnr (scale + shift, or an external mask) / bnr.accumulate / split, in the one-tile
    and persistent forms and on the streaming kernels: stored gradient, skip part and the two BN-backward sums, all equal to float64."""
    outs = run_fused(case, dtn, monkeypatch)
    assert outs or (case.bnr == "mask" and case.srcs[0].C == 16 and dtn != "f32"), "no path ran"


@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_conv_dgrad_pool2_refuses_odd_map(dtn, monkeypatch):
    case = [c for c in CL.fused_cases() if c.name == "pool_odd_9x17"][0]
    run_fused(case, dtn, monkeypatch, paths={"default": {}}, force_pool2=1)


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.large_cases() if c.kind == "dgrad" and c.bnr]))
def test_conv_dgrad_fused_exact_large(case, dtn, monkeypatch):
    run_fused(case, dtn, monkeypatch, paths={"default": {}, "one_tile": {"VK_COL_PERSIST": "0", "VK_NO_STREAM": "1"}})


# ------------------------------------------------------------------------------------------------ weight gradient
DW0 = 5.0      # dw is accumulated into: it starts from a constant, not from zero


def wgrad_paths(case, dtn):
    halo = {"VK_WH_MINBLOCKS": "1", "VK_WH_MAXCOMBO": "1000"}
    paths = {"tap": ({"VK_NO_WGRAD_HALO": "1"}, False), "tap_slab": ({"VK_NO_WGRAD_HALO": "1"}, True),
             "tap_slab_atomics": ({"VK_NO_WGRAD_HALO": "1", "VK_WGRAD_ATOMICS": "1"}, True),
             "default": ({}, True), "default_atomics": ({}, False), "halo": (halo, False), "halo_slab": (halo, True),
             "halo_no_ts": (dict(halo, VK_WH_NO_TS="1"), True), "halo_blocks3": (dict(halo, VK_WH_BLOCKS="3"), True),
             "halo_blocks40": (dict(halo, VK_WH_BLOCKS="40"), True)}
    if case.stride == 2:
        paths["no_s2_tile"] = (dict(halo, VK_NO_S2_TILE="1"), True)
    if dtn != "f32" and case.C == 32 and len(case.srcs) == 1 and case.K in (16, 32):
        paths["no_wstream"] = (dict(halo, VK_NO_WSTREAM="1"), True)
        paths["ws_kw16"] = (dict(halo, VK_WS_KW="16"), True)
        paths["ws_kw32"] = (dict(halo, VK_WS_KW="32"), True)
    return paths


def run_wgrad(case, dtn, mp, paths=None):
    b = built(case)
    dt = DT[dtn]
    keep, errors, outs = [], [], {}
    s0, s1 = src_of(case, b, dt, keep)
    d = desc_of(case, dtn, s0, s1)
    dzd = nhwc(b.dz, dt)
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev())
    ref = (b.dw + DW0).permute(0, 2, 3, 1).contiguous()
    assert float(ref.abs().max()) < CL.TWO24
    for path, (env, slab) in (paths or wgrad_paths(case, dtn)).items():
        set_env(mp, env)
        dw = torch.full((case.K, case.R, case.R, case.C), DW0, dtype=torch.float32, device=dev())
        rc = lib().vk_conv_wgrad(C.byref(d), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr() if slab else None, WS_BYTES if slab else 0, st())
        if not settled(rc, case, [(dw, torch.full_like(dw, DW0))], errors, path):
            continue
        got = dw.double().cpu()
        bad = got != ref
        if bool(bad.any()):
            k, r, s, c = (int(v) for v in bad.nonzero()[0])
            errors.append(f"[{path}] dw: {int(bad.sum())} of {bad.numel()} wrong; first at k {k} tap ({r}, {s}) channel {c} (vector {c // 4}): got "
                          f"{got[k, r, s, c].item() - DW0!r}, want {ref[k, r, s, c].item() - DW0!r}")
        outs[path] = dw
    agree(errors, outs, "dw")
    assert not errors, f"vk_conv_wgrad {case.name} {dtn}:\n" + "\n".join(errors)
    return outs


@pytest.mark.parametrize("case,dtn", typed(CL.wgrad_cases()))
def test_conv_wgrad_exact(case, dtn, monkeypatch):
    """vk_conv_wgrad (fp32 output: equality needs only the 2^24 bound): tap / halo / stream kernels, slab and atomics epilogues
    (VK_WGRAD_ATOMICS, NULL workspace), VK_WH_NO_TS, VK_WH_BLOCKS, VK_WS_KW 16 / 32, up + concat sources, stride 2, 1x1."""
    assert run_wgrad(case, dtn, monkeypatch), "no path ran"


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.large_cases() if c.kind == "wgrad"]))
def test_conv_wgrad_exact_large(case, dtn, monkeypatch):
    run_wgrad(case, dtn, monkeypatch, paths={"default": ({}, True), "default_atomics": ({}, False), "tap_slab": ({"VK_NO_WGRAD_HALO": "1"}, True)})


@pytest.mark.parametrize("case,dtn", typed([c for c in CL.outside_cases() if c.kind == "wgrad"]))
def test_conv_wgrad_outside_documented_set(case, dtn, monkeypatch):
    run_wgrad(case, dtn, monkeypatch)


@pytest.mark.parametrize("workgroups", [0, 1, 3, 7, 16, 256], ids=lambda w: f"wg{w}")
@pytest.mark.parametrize("dtn", ["bf16", "f16"])
def test_conv_wgrad_batch_exact(dtn, workgroups, monkeypatch):
    """vk_conv_wgrad_batch: ragged, non-square layers in one launch, bit-equal to float64 and so to vk_conv_wgrad layer by layer."""
    set_env(monkeypatch, {})
    dt = DT[dtn]
    layers = CL.batch_layers()
    keep, descs, dzs, refs = [], [], [], []
    for case in layers:
        b = CL.build(case)
        s0, s1 = src_of(case, b, dt, keep)
        d = desc_of(case, dtn, s0, s1)
        assert lib().vk_conv_wgrad_batch_supports(C.byref(d)) == 1, case.name
        descs.append(d)
        dzs.append(nhwc(b.dz, dt))
        refs.append((b.dw + DW0).permute(0, 2, 3, 1).contiguous())
    n = len(layers)
    darr = (L_.vk_conv_desc * n)(*descs)
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev())
    tables = torch.empty(128 << 10, dtype=torch.uint8, device=dev())
    errors = []
    for rep in range(2):
        dws = [torch.full((c.K, 3, 3, c.C), DW0, dtype=torch.float32, device=dev()) for c in layers]
        dzp = (C.c_void_p * n)(*[t.data_ptr() for t in dzs])
        dwp = (C.c_void_p * n)(*[t.data_ptr() for t in dws])
        L_.check(lib().vk_conv_wgrad_batch(darr, dzp, dwp, n, workgroups, tables.data_ptr(), tables.numel(), ws.data_ptr(), WS_BYTES, st()), "batch")
        torch.cuda.synchronize()
        for li, c in enumerate(layers):
            bad = dws[li].double().cpu() != refs[li]
            if bool(bad.any()):
                k, r, s, ch = (int(v) for v in bad.nonzero()[0])
                errors.append(f"run {rep} layer {c.name}: {int(bad.sum())} of {bad.numel()} wrong; first at k {k} tap ({r}, {s}) channel {ch}")
    for li, c in enumerate(layers):
        single = torch.full_like(dws[li], DW0)
        L_.check(lib().vk_conv_wgrad(C.byref(descs[li]), dzs[li].data_ptr(), single.data_ptr(), ws.data_ptr(), WS_BYTES, st()), "single")
        torch.cuda.synchronize()
        if not torch.equal(single, dws[li]):
            errors.append(f"layer {c.name}: batch differs from vk_conv_wgrad")
    assert not errors, "\n".join(errors)


# ------------------------------------------------------------------------------------------------ pointwise convolutions
@pytest.mark.parametrize("case,dtn", typed(CL.conv1x1_cases() + CL.large_conv1x1_cases()))
def test_conv1x1_exact(case, dtn, monkeypatch):
    """vk_conv1x1_fwd (both `transposed` values, strides 1 and 2, accumulate, stats) and vk_conv1x1_wgrad (with and without workspace)."""
    set_env(monkeypatch, {})
    b = built(case)
    dt = DT[dtn]
    keep, errors = [], []
    null = L_.vk_src(None, 0, 0, None, None, 0)
    Ho, Wo = case.out_hw
    if case.kind == "fwd":
        s0, _ = src_of(case, b, dt, keep)
        d = desc_of(case, dtn, s0, null)
        wd = b.w[:, :, 0, 0].contiguous().to(dt).to(dev())
        y = filled((case.N, Ho, Wo, case.K), dt)
        stats = torch.zeros(REPL * 2 * case.K, dtype=torch.float64, device=dev())
        L_.check(lib().vk_conv1x1_fwd(C.byref(d), wd.data_ptr(), y.data_ptr(), 0, stats.data_ptr(), st()), "vk_conv1x1_fwd")
        torch.cuda.synchronize()
        diff(errors, "store", "y", y, b.y, dtn)
        diff_sums(errors, "store", "stats", stats, b.stats)
        old = CL.ints(tuple(b.y.shape), -2, 2, torch.Generator().manual_seed(7))
        assert CL.exact_in(b.y + old, dtn)                       # on the reference alone
        y2 = nhwc(old, dt)
        L_.check(lib().vk_conv1x1_fwd(C.byref(d), wd.data_ptr(), y2.data_ptr(), 1, None, st()), "vk_conv1x1_fwd")
        torch.cuda.synchronize()
        diff(errors, "accumulate", "y", y2, b.y + old, dtn)
    elif case.kind == "dgrad":
        dzd = nhwc(b.dz, dt)
        d = desc_of(case, dtn, L_.vk_src(dzd.data_ptr(), case.srcs[0].C, 0, None, None, 0), null, 1)
        wd = b.w[:, :, 0, 0].contiguous().to(dt).to(dev())      # [out][red]
        y = nhwc(b.old, dt) if case.accumulate else filled((case.N, case.H, case.W, case.K), dt)
        L_.check(lib().vk_conv1x1_fwd(C.byref(d), wd.data_ptr(), y.data_ptr(), case.accumulate, None, st()), "vk_conv1x1_fwd(transposed)")
        torch.cuda.synchronize()
        diff(errors, "accumulate" if case.accumulate else "store", "dx", y, b.y, dtn)   # at stride 2 the pixels no tap reaches: zero / untouched
    else:
        s0, _ = src_of(case, b, dt, keep)
        d = desc_of(case, dtn, s0, null)
        dzd = nhwc(b.dz, dt)
        ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev())
        ref = (b.dw[:, :, 0, 0] + DW0)
        outs = {}
        for path, wsp in (("slab", ws), ("slab#2", ws), ("no_ws", None)):
            dw = torch.full((case.K, case.C), DW0, dtype=torch.float32, device=dev())
            L_.check(lib().vk_conv1x1_wgrad(C.byref(d), dzd.data_ptr(), dw.data_ptr(), P_(wsp), WS_BYTES if wsp is not None else 0, st()), "vk_conv1x1_wgrad")
            torch.cuda.synchronize()
            bad = dw.double().cpu() != ref
            if bool(bad.any()):
                k, c = (int(v) for v in bad.nonzero()[0])
                errors.append(f"[{path}] dw: {int(bad.sum())} of {bad.numel()} wrong; first at k {k} channel {c}")
            outs[path] = dw
        agree(errors, outs, "dw")
    assert not errors, f"conv1x1 {case.kind} {case.name} {dtn}:\n" + "\n".join(errors)


# ------------------------------------------------------------------------------------------------ stem
STEM_MAPS = [(2, 40, 104), (1, 66, 34), (3, 2, 2), (1, 8, 32), (2, 16, 64), (1, 34, 130)]


def stem_operands(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = CL.ints((N, 3, H, W), -2, 2, g)
    w = CL.ternary((64, 3, 7, 7), 1.0, g)
    dz = CL.ints((N, 64, H // 2, W // 2), -2, 2, g)
    return x, w, dz


def stem_x4(x, dt):
    N, _, H, W = x.shape
    x4 = torch.zeros((N, H, W, 4), dtype=dt, device=dev())
    x4[..., :3] = x.permute(0, 2, 3, 1).to(dt).to(dev())
    return x4


STEM_LARGE = (2, 512, 512)      # the network's input: 131072 output pixels, 512 stem tiles of 16 x 16


@pytest.mark.parametrize("shape", STEM_MAPS, ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_stem_fwd_exact(dtn, shape, monkeypatch):
    stem_fwd(dtn, shape, monkeypatch)


def test_stem_fwd_exact_large(monkeypatch):
    stem_fwd("bf16", STEM_LARGE, monkeypatch)


def stem_fwd(dtn, shape, monkeypatch):
    """vk_stem_fwd, staged-window kernel and tap kernel, with statistics: 147 ternary taps on integers in [-2, 2] (|y| <= 294 in
    principle; asserted on the reference)."""
    N, H, W = shape
    dt = DT[dtn]
    x, w, _ = stem_operands(N, H, W, 700 + H)
    ref = F.conv2d(x, w, stride=2, padding=3)
    assert CL.exact_in(ref, dtn) and CL.TILE_PIX * 2 * float(ref.abs().max()) ** 2 < CL.TWO24      # 16 x 16 stem tiles: 256 pixels
    x4 = stem_x4(x, dt)
    wp = torch.zeros(64, 7, 8, 4, dtype=torch.float64)
    wp[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    wpd = wp.reshape(64, 7, 32).to(dt).to(dev())
    errors, outs = [], {}
    for path, env in (("tile", {}), ("tap", {"VK_NO_STEM_TILE": "1"})):
        set_env(monkeypatch, env)
        y = filled((N, H // 2, W // 2, 64), dt)
        stats = torch.zeros(REPL * 128, dtype=torch.float64, device=dev())
        L_.check(lib().vk_stem_fwd(CODE[dtn], N, H, W, x4.data_ptr(), wpd.data_ptr(), y.data_ptr(), stats.data_ptr(), st()), "vk_stem_fwd")
        torch.cuda.synchronize()
        diff(errors, path, "y", y, ref, dtn)
        diff_sums(errors, path, "stats", stats, torch.stack([ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))]))
        outs[path] = y
    agree(errors, outs, "y")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("shape", STEM_MAPS, ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_stem_wgrad_exact(dtn, shape, monkeypatch):
    stem_wgrad(dtn, shape, monkeypatch)


def test_stem_wgrad_exact_large(monkeypatch):
    stem_wgrad("f16", STEM_LARGE, monkeypatch)


def stem_wgrad(dtn, shape, monkeypatch):
    """vk_stem_wgrad (atomics, slab, tap kernel) and vk_stem_wgrad_bn with dyadic coef_abc: dz = a g + b z + c is an integer or a half
    below 8, exact in every type, so the folded form equals float64 too."""
    N, H, W = shape
    dt = DT[dtn]
    x, _, dz = stem_operands(N, H, W, 720 + H)
    g = torch.Generator().manual_seed(730 + H)
    z = CL.ints(tuple(dz.shape), -2, 2, g)
    a, bb, cc = CL.lat_scale(64, 0), CL.lat_int(64, 1, 3), CL.lat_int(64, 2, 5) * 0.5
    dz_bn = a.view(1, -1, 1, 1) * dz + bb.view(1, -1, 1, 1) * z + cc.view(1, -1, 1, 1)
    assert CL.exact_in(dz_bn, dtn)

    def reference(dzv):
        wv = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, wv, stride=2, padding=3).backward(dzv)
        wa = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.abs(), wa, stride=2, padding=3).backward(dzv.abs())
        assert float(wa.grad.max()) + DW0 < CL.TWO24
        return (wv.grad + DW0).permute(0, 2, 3, 1).contiguous()

    x4, dzd, zd = stem_x4(x, dt), nhwc(dz, dt), nhwc(z, dt)
    coef = torch.cat([a, bb, cc]).float().to(dev())
    ws = torch.empty(16 << 20, dtype=torch.uint8, device=dev())
    errors = []
    ref, ref_bn = reference(dz), reference(dz_bn)
    for path, env, wsp in (("atomics", {}, None), ("slab", {}, ws), ("taps", {"VK_STEM_WGRAD_TAPS": "1"}, ws)):
        set_env(monkeypatch, env)
        dw = torch.full((64, 7, 7, 3), DW0, dtype=torch.float32, device=dev())
        L_.check(lib().vk_stem_wgrad(CODE[dtn], N, H, W, x4.data_ptr(), dzd.data_ptr(), dw.data_ptr(), P_(wsp), wsp.numel() if wsp is not None else 0, st()),
                 "vk_stem_wgrad")
        torch.cuda.synchronize()
        bad = dw.double().cpu() != ref
        if bool(bad.any()):
            errors.append(f"[{path}] vk_stem_wgrad: {int(bad.sum())} of {bad.numel()} wrong; first at (k, r, s, c) = {tuple(int(v) for v in bad.nonzero()[0])}")
    set_env(monkeypatch, {})
    for path, wsp in (("bn_atomics", None), ("bn_slab", ws)):
        dw = torch.full((64, 7, 7, 3), DW0, dtype=torch.float32, device=dev())
        rc = lib().vk_stem_wgrad_bn(CODE[dtn], N, H, W, x4.data_ptr(), dzd.data_ptr(), zd.data_ptr(), coef.data_ptr(), dw.data_ptr(), P_(wsp),
                                    wsp.numel() if wsp is not None else 0, st())
        torch.cuda.synchronize()
        if dtn == "f32":
            assert rc == -3 and bool((dw == DW0).all())          # VK_ERR_UNSUPPORTED (include/vk_unet.h), nothing written
            continue
        L_.check(rc, "vk_stem_wgrad_bn")
        bad = dw.double().cpu() != ref_bn
        if bool(bad.any()):
            errors.append(f"[{path}] vk_stem_wgrad_bn: {int(bad.sum())} of {bad.numel()} wrong; first at (k, r, s, c) = {tuple(int(v) for v in bad.nonzero()[0])}")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("shape", [(2, 8, 32), (1, 40, 96), (3, 16, 64), (1, 72, 32)], ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("fold", [0, 1], ids=["plain", "bn"])
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_stem_dgrad_exact(dtn, fold, shape):
    """vk_stem_dgrad: dx fp32 NCHW written from dz (or from a g + b z + c with dyadic coefficients) and the fp32 ternary stem weight."""
    N, H, W = shape
    dt = DT[dtn]
    x, w, dz = stem_operands(N, H, W, 740 + H)
    g = torch.Generator().manual_seed(750 + H)
    z = CL.ints(tuple(dz.shape), -2, 2, g)
    a, bb, cc = CL.lat_scale(64, 0), CL.lat_int(64, 1, 3), CL.lat_int(64, 2, 5) * 0.5
    dzv = a.view(1, -1, 1, 1) * dz + bb.view(1, -1, 1, 1) * z + cc.view(1, -1, 1, 1) if fold else dz
    assert CL.exact_in(dzv, dtn)
    xin = torch.zeros(N, 3, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, w, stride=2, padding=3).backward(dzv)
    ref = xin.grad
    assert float(ref.abs().max()) < CL.TWO24
    dzd, zd = nhwc(dz, dt), nhwc(z, dt)
    coef = torch.cat([a, bb, cc]).float().to(dev())
    wd = w.permute(0, 2, 3, 1).contiguous().float().to(dev())
    dx = torch.full((N, 3, H, W), SENTINEL, dtype=torch.float32, device=dev())
    L_.check(lib().vk_stem_dgrad(CODE[dtn], N, H, W, dzd.data_ptr(), zd.data_ptr() if fold else None, coef.data_ptr() if fold else None, wd.data_ptr(),
                                 dx.data_ptr(), st()), "vk_stem_dgrad")
    torch.cuda.synchronize()
    bad = dx.double().cpu() != ref
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} wrong; first at (n, c, h, w) = {tuple(int(v) for v in bad.nonzero()[0])}"


# ------------------------------------------------------------------------------------------------ rounded tier
ROUNDED = [  # kind, N, H, W, sources (C, up, prologue), K, stride
    ("fwd", 2, 9, 33, ((64, 0, True),), 64, 1), ("fwd", 1, 18, 14, ((128, 1, True), (64, 0, False)), 128, 1), ("fwd", 3, 7, 17, ((32, 0, True),), 32, 1),
    ("fwd", 1, 16, 34, ((64, 0, False),), 128, 2), ("fwd", 1, 5, 9, ((512, 0, True),), 512, 1),
    ("dgrad", 2, 9, 33, ((64, 0, False),), 64, 1), ("dgrad", 1, 16, 34, ((128, 0, False),), 64, 2), ("dgrad", 1, 17, 15, ((192, 0, False),), 128, 1),
    ("wgrad", 2, 9, 33, ((64, 0, True),), 64, 1), ("wgrad", 1, 18, 14, ((64, 1, True), (64, 0, False)), 64, 1), ("wgrad", 3, 8, 18, ((32, 0, True),), 32, 1),
    ("wgrad", 1, 16, 34, ((64, 0, False),), 128, 2),
]


def bound(dtn, ref, absdot, chain, prodot, fp32_out=False):
    """Elementwise and derived.  Store: one rounding to the output type, or the other neighbour of an fp32 value that is itself a rounding
    away: 2 u |ref|, absolute (the subnormal spacing) below the normal range.  Accumulation: `chain` fp32 additions, each with a
    relative error of at most 2^-23 (2^-24 if the matrix core rounds to nearest; 2^-23 allows for one that truncates) on a partial sum
    bounded by conv(|V|, |w|).  Prologue: `prodot` = conv(dV, |w|), where dV is how far the operand a kernel may form (see prologue())
    lies from the reference's; it is zero for almost every operand and is not a per-operand allowance."""
    u = U["f32"] if fp32_out else U[dtn]
    sub = SUB["f32"] if fp32_out else SUB[dtn]
    return 2 * u * ref.abs() + sub + chain * 2.0 ** -23 * absdot + prodot


def prologue(x, sc, sh, dt):
    """V = relu(x * scale + shift) rounded to the type, as the reference forms it (float64, one rounding to the type), and dV >= 0, the
    distance from it to the two values a kernel can arrive at in fp32: through one fused multiply-add (the float64 value rounded to fp32,
    then to the type: a double rounding) or through a rounded product and a rounded sum.  Where all three agree, dV is zero."""
    a = x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)      # a 24-bit by 24-bit product and the sum: exact enough
    v = torch.relu(a).to(dt).double()
    fused = torch.relu(a.float()).to(dt).double()
    unfused = torch.relu(x.float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).to(dt).double()
    return v, torch.maximum((fused - v).abs(), (unfused - v).abs())


@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("spec", ROUNDED, ids=[f"{s[0]}_n{s[1]}_{s[2]}x{s[3]}_c{sum(c[0] for c in s[4])}k{s[5]}s{s[6]}" for s in ROUNDED])
def test_conv_rounded(spec, dtn, monkeypatch):
    """Chain lengths (fp32 additions per output element).  fwd / dgrad: one product per tap and reduction channel, 9 C (the MFMA's internal
    adds included), + up to 32 split-K partials, + 1 for accumulate: 9 C + 33.  wgrad: one product per output pixel, N Ho Wo, + the
    split / slab partials (at most one per 128-pixel tile) + 1 for the += into dw: N Ho Wo (1 + 1/128) + 2.  Each path prints its largest
    err / bound before it asserts (pytest -rP shows them)."""
    kind, N, H, W, srcs, K, stride = spec
    dt = DT[dtn]
    g = torch.Generator().manual_seed(900 + H * W + K)
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1)
    keep, vs, dvs, dsrc = [], [], [], []
    Ct = sum(c for c, _, _ in srcs)
    for Cc, up, pro in srcs:
        x = torch.randn(N, Cc, H >> up, W >> up, generator=g).to(dt)
        sc = (0.5 + torch.rand(Cc, generator=g)) if pro else None
        sh = (0.3 * torch.randn(Cc, generator=g)) if pro else None
        v, dv = x.double(), torch.zeros(x.shape, dtype=torch.float64)
        if pro:
            v, dv = prologue(x, sc, sh, dt)
        if up:
            v, dv = F.interpolate(v, scale_factor=2, mode="nearest"), F.interpolate(dv, scale_factor=2, mode="nearest")
        vs.append(v)
        dvs.append(dv)
        xd, scd, shd = x.permute(0, 2, 3, 1).contiguous().to(dev()), fvec(sc), fvec(sh)
        keep += [xd, scd, shd]
        dsrc.append(L_.vk_src(xd.data_ptr(), Cc, up, P_(scd), P_(shd), 1 if pro else 0))
    if len(dsrc) == 1:
        dsrc.append(L_.vk_src(None, 0, 0, None, None, 0))
    V, dV = torch.cat(vs, 1), torch.cat(dvs, 1)
    absV = V.abs() + dV                                           # >= |V| of either form
    if kind == "fwd":
        w = (torch.randn(K, Ct, 3, 3, generator=g) * (2.0 / (9 * Ct)) ** 0.5).to(dt)
        ref = F.conv2d(V, w.double(), stride=stride, padding=1)
        absdot = F.conv2d(absV, w.double().abs(), stride=stride, padding=1)
        bnd = bound(dtn, ref, absdot, 9 * Ct + 33, F.conv2d(dV, w.double().abs(), stride=stride, padding=1))
        d = L_.vk_conv_desc(CODE[dtn], N, H, W, Ho, Wo, K, 3, 3, stride, 1, 0, dsrc[0], dsrc[1])
        wd = w.permute(0, 2, 3, 1).contiguous().to(dev())
        for path, env in (("default", {}), ("igemm", {"VK_NO_HALO": "1"}), ("tile", {"VK_COL_PERSIST": "0"})):
            set_env(monkeypatch, env)
            wp, packed = weights_for(d, wd, keep)
            y = filled((N, Ho, Wo, K), dt)
            fn = lib().vk_conv_fwd_packed if packed else lib().vk_conv_fwd
            L_.check(fn(C.byref(d), wp.data_ptr(), y.data_ptr(), None, 0, 0, None, st()), path)
            torch.cuda.synchronize()
            ratio = ((y.double().cpu().permute(0, 3, 1, 2) - ref).abs() / bnd).max().item()
            print(f"rounded tier: fwd/{path}/{dtn}: worst err / bound = {ratio:.3g}")
            assert ratio <= 1.0, f"[{path}] worst err / bound = {ratio:.3g}"
    elif kind == "dgrad":
        Kred = Ct                                                 # srcs describe dz; K = channels of dx; H, W = the map of dx
        dzv = torch.randn(N, Kred, Ho, Wo, generator=g).to(dt)
        wf = (torch.randn(Kred, K, 3, 3, generator=g) * (2.0 / (9 * Kred)) ** 0.5).to(dt)
        xin = torch.zeros(N, K, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, wf.double(), stride=stride, padding=1).backward(dzv.double())
        xa = torch.zeros(N, K, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xa, wf.double().abs(), stride=stride, padding=1).backward(dzv.double().abs())
        ref, absdot = xin.grad, xa.grad
        bnd = bound(dtn, ref, absdot, 9 * Kred + 33, 0.0)
        dzd = dzv.permute(0, 2, 3, 1).contiguous().to(dev())
        d = L_.vk_conv_desc(CODE[dtn], N, Ho, Wo, H, W, K, 3, 3, stride, 1, 1, L_.vk_src(dzd.data_ptr(), Kred, 0, None, None, 0), dsrc[1])
        wd = wf.permute(1, 2, 3, 0).contiguous().to(dev())
        for path, env in (("default", {}), ("igemm", {"VK_NO_HALO": "1"})):
            set_env(monkeypatch, env)
            wp, packed = weights_for(d, wd, keep)
            y = filled((N, H, W, K), dt)
            fn = lib().vk_conv_fwd_packed if packed else lib().vk_conv_fwd
            L_.check(fn(C.byref(d), wp.data_ptr(), y.data_ptr(), None, 0, 0, None, st()), path)
            torch.cuda.synchronize()
            ratio = ((y.double().cpu().permute(0, 3, 1, 2) - ref).abs() / bnd).max().item()
            print(f"rounded tier: dgrad/{path}/{dtn}: worst err / bound = {ratio:.3g}")
            assert ratio <= 1.0, f"[{path}] worst err / bound = {ratio:.3g}"
    else:
        dzv = torch.randn(N, K, Ho, Wo, generator=g).to(dt)
        wv = torch.zeros(K, Ct, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(V, wv, stride=stride, padding=1).backward(dzv.double())
        wa = torch.zeros(K, Ct, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(absV, wa, stride=stride, padding=1).backward(dzv.double().abs())
        wd_ = torch.zeros(K, Ct, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(dV, wd_, stride=stride, padding=1).backward(dzv.double().abs())
        ref, absdot, prodot = wv.grad.permute(0, 2, 3, 1), wa.grad.permute(0, 2, 3, 1), wd_.grad.permute(0, 2, 3, 1)
        px = N * Ho * Wo
        bnd = bound(dtn, ref, absdot, px + math.ceil(px / 128) + 2, prodot, fp32_out=True)
        d = L_.vk_conv_desc(CODE[dtn], N, H, W, Ho, Wo, K, 3, 3, stride, 1, 0, dsrc[0], dsrc[1])
        dzd = dzv.permute(0, 2, 3, 1).contiguous().to(dev())
        ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev())
        for path, env, slab in (("default", {}, True), ("tap", {"VK_NO_WGRAD_HALO": "1"}, True),
                                ("halo", {"VK_WH_MINBLOCKS": "1", "VK_WH_MAXCOMBO": "1000"}, True), ("halo_atomics", {"VK_WH_MINBLOCKS": "1", "VK_WH_MAXCOMBO": "1000"}, False)):
            set_env(monkeypatch, env)
            dw = torch.zeros((K, 3, 3, Ct), dtype=torch.float32, device=dev())
            L_.check(lib().vk_conv_wgrad(C.byref(d), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr() if slab else None, WS_BYTES if slab else 0, st()), path)
            torch.cuda.synchronize()
            ratio = ((dw.double().cpu() - ref).abs() / bnd).max().item()
            print(f"rounded tier: wgrad/{path}/{dtn}: worst err / bound = {ratio:.3g}")
            assert ratio <= 1.0, f"[{path}] worst err / bound = {ratio:.3g}"
