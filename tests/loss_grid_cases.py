"""Built cases for the sweep of the loss kernels at the workgroup counts real batches take (csrc/seg_loss.hip, csrc/kp_loss.hip and the
two loss entry points of csrc/multiclass.hip, plus the two launch caps of vk_lovasz_loss).  No GPU is needed to import this module.

Every kernel here divides a plane (or an image) among nbx workgroups, each workgroup writes one row of float64 partials, and one
finalize workgroup adds the rows.  The host picks nbx from the shape alone; the three rules are restated below from the constants of the
sources, and the case list is built from them: a case is listed under the route (nbx, sweeps of a thread, ragged last sweep, rows, trips
of the finalize row loop) that the rules give it, and tests/test_loss_grid_cpu.py proves that it takes that route.

Families: seg_sig (vk_seg_loss, binary for C = 1 and multilabel otherwise), seg_mc (vk_seg_loss, multiclass), kp (vk_kp_loss),
ml (vk_multilabel_loss), mc (vk_multiclass_loss)."""
from __future__ import annotations

import functools

import numpy as np
import torch

import keypoints_loss_cases as KC
import seglosses_cases as K

IGN = K.IGN

# ------------------------------------------------------------------------------------------------ the rules of the sources
BLOCK, VEC = 256, 4                      # threads of a workgroup; pixels of a thread on the 16-byte route (1 on the scalar route)
NBX_CAP = 64                             # no plane or image gets more workgroups
SEG_WG_PIXELS = 2048                     # seg_loss.hip: one workgroup per 2048 pixels ...
SEG_BUDGET_SIGMOID = 2048                # ... but no more than 2048 workgroups over the N C planes of the sigmoid modes
SEG_BUDGET_MULTICLASS = 1024             # ... and 1024 over the N images of the multiclass mode
SEG_FINALIZE_LANES = 64                  # k_sl_finalize: 64 lanes stride the rows of a column
SEG_COEF_DOUBLES = 64
KP_WG_PIXELS, KP_BUDGET = 2048, 2048     # kp_loss.hip
KP_FINALIZE_LANES = 64
KP_COEF_DOUBLES = 16
MULTI_WG_PIXELS = 4096                   # multiclass.hip: HW // 4096 workgroups, one pixel per thread on every route
MULTI_FINALIZE_THREADS = 256             # k_ml_finalize, k_mc_finalize: 256 threads stride the rows
MULTI_COEF_DOUBLES = 64


def _clamp(v: int) -> int:
    return max(1, min(NBX_CAP, v))


def seg_nbx(multiclass: bool, N: int, C: int, HW: int) -> int:
    units = N if multiclass else N * C
    want = max((SEG_BUDGET_MULTICLASS if multiclass else SEG_BUDGET_SIGMOID) // units, 1)
    return min(want, _clamp(HW // SEG_WG_PIXELS))


def kp_nbx(N: int, C: int, HW: int) -> int:
    return min(max(KP_BUDGET // (N * C), 1), _clamp(HW // KP_WG_PIXELS))


def multi_nbx(HW: int) -> int:
    return _clamp(HW // MULTI_WG_PIXELS)


def seg_workspace_bytes(N: int, C: int, HW: int) -> int:
    """the larger of the two modes' tables (the function does not know the mode), after the coefficients"""
    sig = 6 * C * N * seg_nbx(False, N, C, HW)
    mc = (3 * C + 4) * N * seg_nbx(True, N, C, HW)
    return 8 * (SEG_COEF_DOUBLES + max(sig, mc))


def kp_workspace_bytes(N: int, C: int, HW: int) -> int:
    return 8 * KP_COEF_DOUBLES + C * N * kp_nbx(N, C, HW) * (8 + 8)              # a double and a 64-bit count per row


def multi_workspace_bytes(N: int, C: int, HW: int) -> int:
    nbx = multi_nbx(HW)
    return 8 * (MULTI_COEF_DOUBLES + max(N * C * nbx * 4, N * nbx * (3 * C + 2)))


def route(family: str, N: int, C: int, HW: int) -> dict:
    """What the rules give a shape: nbx; V pixels per thread; sweeps, the trips of the pixel loop of thread 0 of workgroup 0 (no thread
    makes more); ragged: the last sweep is not full; idle_last: workgroups without a pixel on the last sweep; rows: the rows one finalize
    loop strides; trips: the trips of that loop's busiest lane.  ml has a second loop over all N C nbx rows (the BCE sum): trips_all."""
    if family in ("seg_sig", "seg_mc"):
        nbx, V, lanes = seg_nbx(family == "seg_mc", N, C, HW), (VEC if HW % 4 == 0 else 1), SEG_FINALIZE_LANES
    elif family == "kp":
        nbx, V, lanes = kp_nbx(N, C, HW), (VEC if HW % 4 == 0 else 1), KP_FINALIZE_LANES
    elif family in ("ml", "mc"):
        nbx, V, lanes = multi_nbx(HW), 1, MULTI_FINALIZE_THREADS
    else:
        raise KeyError(family)
    stride = nbx * BLOCK * V
    sweeps = -(-HW // stride)
    last = (sweeps - 1) * stride
    idle = sum(1 for bx in range(nbx) if last + bx * BLOCK * V >= HW)
    rows = N * nbx
    r = dict(nbx=nbx, V=V, stride=stride, sweeps=sweeps, ragged=HW % stride != 0, idle_last=idle, rows=rows, trips=-(-rows // lanes))
    if family == "ml":
        r["rows_all"] = N * C * nbx
        r["trips_all"] = -(-r["rows_all"] // lanes)
    return r


def share(family: str, N: int, C: int, HW: int, bx: int) -> np.ndarray:
    """the pixels of workgroup bx: {(bx 256 + t) V + k nbx 256 V}, t < 256, below HW"""
    r = route(family, N, C, HW)
    V, stride = r["V"], r["stride"]
    base = (bx * BLOCK + np.arange(BLOCK)[:, None]) * V + np.arange(V)[None, :]
    idx = (base.reshape(1, -1) + stride * np.arange(r["sweeps"])[:, None]).reshape(-1)
    return np.sort(idx[idx < HW])


# ------------------------------------------------------------------------------------------------ the case list
# vk_kp_loss runs two of keypoints_loss_cases.CONFIGS: the heat-only one and the 16-plane mixed one (N of a case replaces the config's)
KP_HEAT = next(c for c in KC.CONFIGS if c[0] == "n1c1_heat")
KP_MIXED = next(c for c in KC.CONFIGS if c[0] == "n3c16_a8b8")
KP_THR = 0.9
WEIGHTS = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0)]          # the three pairs of tests/test_multiclass_gpu.py


def _smallest_hw(wg_pixels: int, nbx: int, vector: bool, extra: int = 0) -> int:
    """the smallest HW >= nbx wg_pixels + extra on the asked route with a ragged last sweep"""
    hw = nbx * wg_pixels + extra
    while (hw % 4 == 0) != vector or hw % (nbx * BLOCK * (VEC if vector else 1)) == 0:
        hw += 1
    return hw


def _three(wg_pixels: int, V_of_vector: int):
    """four HW with three workgroups: (16-byte, scalar) x (only workgroup 0 has pixels on the last sweep, every workgroup but a part of
    the last has).  On the 16-byte route of the 2048-pixel rule the last workgroup can never have one: 2 strides + 2 shares is 8192."""
    out = []
    for vector in (True, False):
        V = V_of_vector if vector else 1
        stride = 3 * BLOCK * V
        lo = 3 * wg_pixels
        full = -(-lo // stride) * stride                 # the first multiple of the stride at or above the class's lower end
        first = full + (4 if vector else 3)             # a few pixels into the next sweep: workgroup 0 alone
        wide = full + 2 * BLOCK * V + (8 if vector else 5)   # into the last workgroup's share
        if wide >= 4 * wg_pixels:                        # (the 16-byte route of seg / kp) stay in the class: the middle workgroup's share
            wide = full + BLOCK * V + 8
        for hw in (first, wide):
            assert lo <= hw < 4 * wg_pixels and (hw % 4 == 0) == vector
            out.append(hw)
    return out


def _cases():
    c = []

    def add(family, cls, N, C, HW, config=None):
        c.append(dict(family=family, cls=cls, N=N, C=C, HW=HW, config=config,
                      id="%s-%s-n%dc%d-hw%d" % (family, cls, N, C, HW)))

    two_s = [_smallest_hw(SEG_WG_PIXELS, 2, True, 4), _smallest_hw(SEG_WG_PIXELS, 2, False, 3)]         # 4100, 4099
    two_m = [_smallest_hw(MULTI_WG_PIXELS, 2, True, 4), _smallest_hw(MULTI_WG_PIXELS, 2, False, 3)]     # 8196, 8195
    three_s, three_m = _three(SEG_WG_PIXELS, VEC), _three(MULTI_WG_PIXELS, 1)
    cap_s = [_smallest_hw(SEG_WG_PIXELS, NBX_CAP, True, 4), _smallest_hw(SEG_WG_PIXELS, NBX_CAP, False, 3)]   # 131076, 131075
    cap_m = [_smallest_hw(MULTI_WG_PIXELS, NBX_CAP, True, 4), _smallest_hw(MULTI_WG_PIXELS, NBX_CAP, False, 3)]
    # ---- vk_seg_loss, sigmoid modes: C in {1, 4, 16}
    for C in (1, 4, 16):
        for hw in two_s:
            add("seg_sig", "two", 2, C, hw)
    for C, hw in zip((4, 1, 16, 4), three_s):
        add("seg_sig", "three", 2, C, hw)
    add("seg_sig", "cap", 2, 4, cap_s[0])                 # 128 rows: 2 trips
    add("seg_sig", "cap", 3, 1, cap_s[1])                 # 192 rows: 3 trips
    add("seg_sig", "cap", 5, 1, cap_s[0])                 # 320 rows: 5 trips
    add("seg_sig", "odd", 3, 16, _smallest_hw(SEG_WG_PIXELS, 42, True, 4))        # nbx = 42 from the budget 2048 // 48: 126 rows
    add("seg_sig", "odd", 3, 16, _smallest_hw(SEG_WG_PIXELS, 42, False, 3))       # the same on the scalar route
    add("seg_sig", "want2", 64, 16, three_s[2])           # N C = 1024: want 2 while HW // 2048 = 3
    add("seg_sig", "want2", 64, 16, three_s[0])           # the same on the 16-byte route
    add("seg_sig", "nbx1", 129, 16, two_s[0])             # N C = 2064 > 2048: one workgroup although HW >= 4096
    # ---- vk_seg_loss, multiclass: C in {2, 5, 16}, the three CM instantiations
    for C in (2, 5, 16):
        for hw in two_s:
            add("seg_mc", "two", 2, C, hw)
    for C, hw in zip((5, 2, 16, 5), three_s):
        add("seg_mc", "three", 2, C, hw)
    add("seg_mc", "cap", 2, 16, cap_s[0])                 # CM = 16, 128 rows
    add("seg_mc", "cap", 3, 5, cap_s[1])                  # CM = 8, 192 rows
    add("seg_mc", "cap", 5, 2, cap_s[0])                  # CM = 4, 320 rows
    add("seg_mc", "odd", 5, 5, _smallest_hw(SEG_WG_PIXELS, 21, True, 4))          # nbx = 21: 105 rows, 105 mod 64 = 41
    add("seg_mc", "odd", 3, 2, _smallest_hw(SEG_WG_PIXELS, 43, False, 3))         # nbx = 43: 129 rows, one row into the third trip
    add("seg_mc", "want2", 512, 2, three_s[2])            # N = 512: want 2
    add("seg_mc", "want2", 512, 2, three_s[0])            # the same on the 16-byte route
    add("seg_mc", "nbx1", 1025, 2, two_s[0])              # N > 1024: one workgroup
    # ---- vk_kp_loss
    for cfg, N in ((KP_HEAT, 1), (KP_MIXED, 3)):
        for hw in two_s:
            add("kp", "two", N, cfg[2], hw, cfg)
    for (cfg, N), hw in zip(((KP_HEAT, 1), (KP_MIXED, 3), (KP_MIXED, 3), (KP_HEAT, 1)), three_s):
        add("kp", "three", N, cfg[2], hw, cfg)
    add("kp", "cap", 2, 1, cap_s[0], KP_HEAT)
    add("kp", "cap", 3, 1, cap_s[1], KP_HEAT)
    add("kp", "cap", 5, 1, cap_s[0], KP_HEAT)
    add("kp", "odd", 3, 16, _smallest_hw(KP_WG_PIXELS, 42, True, 4), KP_MIXED)
    add("kp", "odd", 3, 16, _smallest_hw(KP_WG_PIXELS, 42, False, 3), KP_MIXED)
    add("kp", "want2", 64, 16, three_s[2], KP_MIXED)
    add("kp", "want2", 64, 16, three_s[0], KP_MIXED)
    add("kp", "nbx1", 129, 16, two_s[0], KP_MIXED)
    # ---- multiclass.hip (one pixel per thread whatever HW % 4 is; both kinds of HW all the same)
    for C in (1, 4):
        for hw in two_m:
            add("ml", "two", 2, C, hw)
    add("ml", "two", 2, 16, two_m[1])
    for C, hw in zip((4, 1, 4, 4), three_m):
        add("ml", "three", 2, C, hw)
    for C in (2, 5):
        for hw in two_m:
            add("mc", "two", 2, C, hw)
    add("mc", "two", 2, 16, two_m[0])
    for C, hw in zip((3, 5, 3, 2), three_m):
        add("mc", "three", 2, C, hw)
    for fam in ("ml", "mc"):
        add(fam, "cap", 5, 2, _smallest_hw(MULTI_WG_PIXELS, 52, False, 3))    # the smallest N nbx > 256: 5 x 52 = 260 rows, 2 trips
        add(fam, "cap", 5, 2, cap_m[0])                                       # nbx = 64: 320 rows
        add(fam, "cap", 9, 2, cap_m[1])                                       # 576 rows: 3 trips
    add("mc", "cap", 13, 2, cap_m[0])                                         # 832 rows: 4 trips (ml makes 5 over its 1152 at N = 9)
    return c


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
MANY_SHARES = 100                        # shares from which the sensitivity test checks a fixed sample of them


def cases(family: str, *classes: str):
    return [c for c in CASES if c["family"] == family and (not classes or c["cls"] in classes)]


def ident(case) -> str:
    return case["id"]


def seg_mode(case) -> str:
    return "multiclass" if case["family"] == "seg_mc" else ("binary" if case["C"] == 1 else "multilabel")


# the single terms of vk_seg_loss run on the two- and three-workgroup shapes only, four shapes per mode: both classes on both routes,
# with C (and so CM) going round with the term
SINGLE_NAMES = [n for n in K.case_names() if n != "sum5"]


def single_term_cases(family: str):
    out = []
    for i, name in enumerate(SINGLE_NAMES):
        for cls in ("two", "three"):
            for vector in (True, False):
                pool = [c for c in cases(family, cls) if (c["HW"] % 4 == 0) == vector]
                out.append((pool[i % len(pool)], name))
    return out


# ------------------------------------------------------------------------------------------------ inputs
def _seed(case) -> int:
    return 7919 * case["N"] + 104729 * case["C"] + case["HW"] + 13 * ["seg_sig", "seg_mc", "kp", "ml", "mc"].index(case["family"])


def _ladder(lo: float, hi: float, n: int) -> np.ndarray:
    return np.linspace(lo, hi, n) if n > 1 else np.full(1, 0.5 * (lo + hi))


def _plane_offsets(rng, N: int, C: int) -> np.ndarray:
    """one offset per plane, all different: a ladder over [-1.5, 1.5] along the classes (the first and the last class differ most: the
    two whose shares the sensitivity test exchanges) plus a shuffled ladder over [-0.4, 0.4] along the images"""
    return _ladder(-1.5, 1.5, C).reshape(1, C, 1) + rng.permutation(_ladder(-0.4, 0.4, N)).reshape(N, 1, 1)


def _plane_rates(rng, N: int, C: int, lo: float, hi: float) -> np.ndarray:
    """one foreground rate per plane: a ladder over [lo, hi] along the classes, times a shuffled 0.8 .. 1.2 along the images"""
    return _ladder(lo, hi, C).reshape(1, C, 1) * rng.permutation(_ladder(0.8, 1.2, N)).reshape(N, 1, 1)


def _ramp(HW: int) -> np.ndarray:
    return (np.arange(HW, dtype=np.float64) / HW - 0.5).reshape(1, 1, HW)


def _sigmoid_inputs(case, ignore: bool):
    """logits 2 randn + plane offset + a ramp of 2 along the pixel index; foreground rate per plane in [0.1, 0.48], times 0.5 .. 1.5
    along the pixel index; class 1 absent from the batch when C > 1; 10 % of the entries ignored"""
    N, C, HW = case["N"], case["C"], case["HW"]
    rng = np.random.default_rng(_seed(case))
    u = _ramp(HW)
    x = (2.0 * rng.standard_normal((N, C, HW), dtype=np.float32) + (_plane_offsets(rng, N, C) + 2.0 * u).astype(np.float32))
    rate = _plane_rates(rng, N, C, 0.12, 0.4) * (1.0 + u)
    y = (rng.random((N, C, HW), dtype=np.float32) < rate.astype(np.float32)).astype(np.float32)
    if C > 1:
        y[:, 1] = 0.0
    if ignore:
        y[rng.random((N, C, HW), dtype=np.float32) < 0.1] = float(IGN)
    return x, y


def _multiclass_inputs(case, ignore: bool):
    """logits 2 randn - plane offset (class 0 is favoured, the last class least) + a ramp along the pixel index whose slope differs per
    class; labels floor(Ce v^e) with v uniform
    and the exponent e per image in [1.4, 2.6] times 0.6 .. 1.4 along the pixel index (class 0 is the most frequent, the last class the
    rarest, and the low classes gain along an image); class 1 absent
    when C > 2; the logit of the labelled class raised by 3 (class 0) down to 0 (the last class), so that the classes' scores differ as
    much as their sizes; 10 % of the pixels ignored"""
    N, C, HW = case["N"], case["C"], case["HW"]
    rng = np.random.default_rng(_seed(case))
    u = _ramp(HW)
    slope = np.linspace(-2.0, 2.0, C).reshape(1, C, 1)
    x = 2.0 * rng.standard_normal((N, C, HW), dtype=np.float32) + (slope * u - _plane_offsets(rng, N, C)).astype(np.float32)
    Ce = C - 1 if C > 2 else C
    e = rng.permutation(_ladder(1.4, 2.6, N)).reshape(N, 1) * (1.0 + 0.8 * u.reshape(1, HW))
    t = np.minimum(np.floor(Ce * rng.random((N, HW)) ** e), Ce - 1).astype(np.int64)
    if C > 2:
        t += t >= 1
    boost = np.linspace(3.0, 0.0, C, dtype=np.float32)    # the labelled class's logit is raised: by 3 for class 0, not at all for the last
    x += boost.reshape(1, C, 1) * (t[:, None, :] == np.arange(C).reshape(1, C, 1))
    if ignore:
        t[rng.random((N, HW), dtype=np.float32) < 0.1] = IGN
    return x, t


def _kp_inputs(case):
    """logits as the sigmoid modes'; targets v^2 with v uniform (a twentieth of them at or above the threshold 0.9) and exact ones at
    the plane's foreground rate"""
    N, C, HW = case["N"], case["C"], case["HW"]
    rng = np.random.default_rng(_seed(case))
    u = _ramp(HW)
    x = (2.0 * rng.standard_normal((N, C, HW), dtype=np.float32) + (_plane_offsets(rng, N, C) + 2.0 * u).astype(np.float32))
    y = rng.random((N, C, HW), dtype=np.float32) ** 2
    rate = _plane_rates(rng, N, C, 0.05, 0.2) * (1.0 + u)
    y[rng.random((N, C, HW), dtype=np.float32) < rate.astype(np.float32)] = 1.0
    return x, y


@functools.lru_cache(maxsize=2)
def _inputs_cached(case_id: str, ignore: bool):
    case = BY_ID[case_id]
    fam = case["family"]
    if fam in ("seg_sig", "ml"):
        return _sigmoid_inputs(case, ignore and fam == "seg_sig")
    if fam in ("seg_mc", "mc"):
        return _multiclass_inputs(case, ignore and fam == "seg_mc")
    return _kp_inputs(case)


def inputs(case, ignore: bool = True):
    """(logits float32 [N][C][HW], target) as numpy arrays that the caller leaves unchanged: float32 [N][C][HW] for seg_sig, ml and
    kp, int64 [N][HW] for seg_mc and mc.  ignore: vk_seg_loss only (the other entry points have no ignore_index)."""
    return _inputs_cached(case["id"], bool(ignore))


def kp_ref_cfg(case) -> dict:
    return KC.ref_cfg(case["config"], KP_THR)


def sample_shares(case):
    """(n, c, bx) whose share the sensitivity test zeroes: every share of every plane of a small case; of a large one the first, the
    last, one in the middle and one per image (of at most five images, evenly spread).  With one workgroup per plane (the nbx1 class)
    a share is a whole plane and the images differ by their offset alone: the first, the last and the middle one."""
    fam, N, C = case["family"], case["N"], case["C"]
    nbx = route(fam, N, C, case["HW"])["nbx"]
    planes = 1 if fam in ("seg_mc", "mc") else C            # a multiclass workgroup owns all classes of its pixels
    if N * planes * nbx <= MANY_SHARES:
        return [(n, c, bx) for n in range(N) for c in range(planes) for bx in range(nbx)]
    picks = [(0, 0, 0), (N - 1, planes - 1, nbx - 1), (N // 2, planes // 2, nbx // 2)]
    if nbx == 1:
        return sorted(set(picks))
    for j, n in enumerate(sorted(set(np.linspace(0, N - 1, min(N, 5)).round().astype(int).tolist()))):
        picks.append((n, (3 * j + 1) % planes, (17 * j + 5) % nbx))
    return sorted(set(picks))


# ------------------------------------------------------------------------------------------------ the two Lovasz launch caps
LV_BAD_CAP, LV_BWD_CAP = 1024, 8192      # workgroups of 256 threads: k_lv_bad, k_lv_softmax_bwd (csrc/lovasz.hip)
# (name, N, C, HW, first pixel of the second trip of the kernel the case is about).  d0 of each case (tests/lovasz_cases.softmax_d0,
# measured on the CPU) is recorded in LOVASZ_D0; tests/test_loss_grid_cpu.py measures it again
LOVASZ = [("bad_cap", 2, 2, 131076, LV_BAD_CAP * BLOCK), ("bwd_cap", 2, 2, 1048580, LV_BWD_CAP * BLOCK)]
LOVASZ_D0 = {"bad_cap": 1.819e-07, "bwd_cap": 9.032e-08}


def lovasz_inputs(name: str):
    """(logits float32 [N][C][1][HW], labels int64 [N][1][HW]) as torch tensors: both classes present, 10 % ignored"""
    _, N, C, HW, _ = next(c for c in LOVASZ if c[0] == name)
    x, t = _multiclass_inputs(dict(family="seg_mc", N=N, C=C, HW=HW), True)
    return torch.from_numpy(x).reshape(N, C, 1, HW), torch.from_numpy(t).reshape(N, 1, HW)
