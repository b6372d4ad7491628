"""Built cases of tests/test_sweep_cpu.py and tests/test_vk_sweep_gpu.py: threshold grids, prediction values placed on, beside and
between the thresholds, targets with bad and ignored values, and histograms for the curves pass.  Everything is seeded by the case's name; the CPU file
checks the numpy restatement on the same cases the GPU file runs through the kernels.

Shapes are the smallest at which the histogram kernel takes another path: plane lengths around the vector width (4 elements) and
the workgroup (256 threads), lengths that are no multiple of either, several workgroups per plane
(4097, 12289, 96 x 160, 512 x 512), base pointers one element off a 16-byte boundary (the vector path must switch off)."""
import zlib
from collections import namedtuple

import numpy as np

F32 = np.float32
IGNORE = 255

PLANES = (1, 3, 4, 5, 255, 256, 257, 1023, 4097, 12289, 96 * 160)
KS = (1, 2, 3, 63, 64, 65, 99, 1024)
GRIDS = ("uniform", "nonuniform", "ulp", "wide", "negative")


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def grid(kind, K, rng=None):
    """K float32 thresholds, strictly ascending."""
    if kind == "uniform":
        thr = (np.arange(1, K + 1) / (K + 1)).astype(F32)
    elif kind == "default":
        assert K == 99
        thr = (np.arange(1, 100) / 100).astype(F32)
    elif kind == "nonuniform":
        thr = np.cumsum(rng.random(K) ** 3 + 1e-4)
        thr = (thr / (thr[-1] * 1.02)).astype(F32)
    elif kind == "ulp":                      # neighbours one ulp apart, around 0.5
        thr = np.empty(K, F32)
        v = F32(0.5)
        for _ in range(K // 2):
            v = np.nextafter(v, F32(-1))
        for i in range(K):
            thr[i] = v
            v = np.nextafter(v, F32(2))
    elif kind == "wide":                     # beyond [0, 1] on both sides: scores, not probabilities
        thr = np.linspace(-3.0, 4.0, K).astype(F32) if K > 1 else np.array([1.5], F32)
    elif kind == "negative":
        thr = np.linspace(-9.0, -1.0, K).astype(F32) if K > 1 else np.array([-2.0], F32)
    else:
        raise ValueError(kind)
    assert thr.dtype == F32 and thr.size == K and np.isfinite(thr).all() and (np.diff(thr) > 0).all(), (kind, K)
    return thr


def values(kind, shape, thr, rng):
    """fp32 prediction values (probabilities or scores: no transcendental between them and the bins)."""
    n = int(np.prod(shape))
    lo, hi = float(thr[0]), float(thr[-1])
    span = max(hi - lo, 1e-3)
    if kind == "uniform":
        v = (lo - 0.1 * span + rng.random(n) * 1.2 * span).astype(F32)
    elif kind == "at_thr":                   # on a threshold and one ulp either side: the strict `>`
        t = thr[rng.integers(0, thr.size, n)]
        side = rng.integers(0, 3, n)
        v = np.where(side == 0, t, np.where(side == 1, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf)))).astype(F32)
    elif kind == "special":
        v = (lo + rng.random(n) * span).astype(F32)
        pick = rng.integers(0, 8, n)
        v[pick == 0] = np.nan
        v[pick == 1] = np.inf
        v[pick == 2] = -np.inf
    elif kind == "mix":
        parts = [values(k, (m,), thr, rng) for k, m in zip(("uniform", "at_thr", "special"), (n - 2 * (n // 3), n // 3, n // 3))]
        v = rng.permutation(np.concatenate(parts))
    elif kind == "saturated":                # everything in the two end bins
        ends = np.array([thr[0], F32(lo - 1.0), np.nextafter(thr[-1], F32(np.inf)), F32(hi + 1.0)], F32)
        v = ends[rng.integers(0, 4, n)]
    elif kind == "one_bin":                  # everything in ONE bin b, a middle one where the grid has one: thr[b - 1] < v <= thr[b]
        b = max(1, thr.size // 2)
        v = np.full(n, np.nextafter(thr[b - 1], F32(np.inf)), F32)
    else:
        raise ValueError(kind)
    return v.reshape(shape).astype(F32)


def targets(kind, shape, rng, dtype):
    n = int(np.prod(shape))
    t = (rng.random(n) < 0.3).astype(np.int64)
    if kind == "zeros":
        t[:] = 0
    elif kind == "ones":
        t[:] = 1
    t = t.astype(dtype)
    if kind == "bad":                        # values that are neither 0 nor 1
        pick = rng.integers(0, 6, n)
        t[pick == 0] = 2
        t[pick == 1] = 0.5 if dtype == F32 else 7
        if dtype == F32:
            t[pick == 2] = np.nan
    elif kind == "ignore":
        t[rng.integers(0, 4, n) == 0] = IGNORE
        t[rng.integers(0, 16, n) == 0] = 3   # and a few bad ones beside them
    elif kind == "all_ignored":
        t[:] = IGNORE
    return t.reshape(shape)


HCase = namedtuple("HCase", "name n c plane K grid values target tdtype ignore offset")


def _h(name, n=2, c=1, plane=4097, K=99, g="uniform", v="mix", t="random", dt="f32", ignore=None, offset=0):
    return HCase(name, n, c, plane, K, g, v, t, dt, ignore, offset)


def hist_cases():
    cases = []
    for dt in ("f32", "u8"):
        for L in PLANES:
            cases.append(_h("plane%d_%s" % (L, dt), plane=L, dt=dt))
        cases.append(_h("two_512x512_%s" % dt, plane=512 * 512, dt=dt, v="uniform"))
        for L in (257, 4096):                # one element off the 16-byte boundary
            cases.append(_h("offset1_plane%d_%s" % (L, dt), plane=L, dt=dt, offset=1))
        cases.append(_h("offset4_plane4096_%s" % dt, plane=4096, dt=dt, offset=4))
        for t in ("zeros", "ones", "bad"):
            cases.append(_h("target_%s_%s" % (t, dt), plane=96 * 160, t=t, dt=dt))
        cases.append(_h("target_ignore_%s" % dt, plane=96 * 160, t="ignore", dt=dt, ignore=IGNORE))
        cases.append(_h("target_all_ignored_%s" % dt, plane=1023, t="all_ignored", dt=dt, ignore=IGNORE))
    for K in KS:
        for g in GRIDS:
            cases.append(_h("K%d_%s" % (K, g), n=1, c=3, K=K, g=g))
    for K in (1, 3, 99, 1024):
        cases.append(_h("K%d_saturated" % K, n=1, c=2, K=K, v="saturated"))
        cases.append(_h("K%d_one_bin" % K, n=1, c=2, K=K, v="one_bin", dt="u8"))
    for n in (1, 2, 5):
        for c in (1, 3, 16):
            cases.append(_h("N%d_C%d" % (n, c), n=n, c=c, plane=1023, dt="u8" if (n + c) % 2 else "f32"))
    return cases


HIST_CASES = hist_cases()
HIST_IDS = [c.name for c in HIST_CASES]


def build_hist_case(case):
    """-> (thr, pred fp32 [N, C, L], target [N, C, L])"""
    rng = rng_of(case.name)
    thr = grid(case.grid, case.K, rng)
    shape = (case.n, case.c, case.plane)
    pred = values(case.values, shape, thr, rng)
    tgt = targets(case.target, shape, rng, F32 if case.tdtype == "f32" else np.uint8)
    return thr, pred, tgt


# ------------------------------------------------------------------------------------------------ curves pass
CCase = namedtuple("CCase", "name n c K kind groups")
BIG = 2 ** 31 - 1


def _groups(kind, n):
    if kind is None:
        return None, 0
    if kind == "132":                        # sizes (1, 3, 2), interleaved
        assert n == 6
        return np.array([1, 0, 1, 2, 1, 2], np.int32), 3
    if kind == "one":                        # every image in one group
        return np.zeros(n, np.int32), 1
    if kind == "three":                      # three interleaved groups of unequal size
        return (np.arange(n) * 7 % 5 % 3).astype(np.int32), 3
    raise ValueError(kind)


CURVE_CASES = [
    CCase("N1_C1_K99", 1, 1, 99, "random", None),
    CCase("N1_C3_K1", 1, 3, 1, "random", None),
    CCase("N64_C1_K99", 64, 1, 99, "random", None),
    CCase("N65_C3_K99", 65, 3, 99, "random", None),
    CCase("N70_C16_K99", 70, 16, 99, "random", None),
    CCase("N70_C1_K1024", 70, 1, 1024, "random", None),
    CCase("N5_C3_K1024", 5, 3, 1024, "sparse", None),
    CCase("N65_C16_K1", 65, 16, 1, "random", None),
    CCase("N3_C3_K99_big", 3, 3, 99, "big", None),
    CCase("N4_C3_K99_empty", 4, 3, 99, "empty", None),
    CCase("N5_C3_K99_onesided", 5, 3, 99, "onesided", None),
    CCase("N6_C1_K99_groups132", 6, 1, 99, "random", "132"),
    CCase("N6_C3_K1024_groups132", 6, 3, 1024, "sparse", "132"),
    CCase("N70_C1_K99_onegroup", 70, 1, 99, "random", "one"),
    CCase("N70_C3_K99_threegroups", 70, 3, 99, "random", "three"),
    CCase("N200_C1_K99_threegroups", 200, 1, 99, "random", "three"),
]
CURVE_IDS = [c.name for c in CURVE_CASES]


def build_curve_case(case):
    """-> (hist int32 [N, C, 2, K + 1], groups or None, G)"""
    rng = rng_of(case.name)
    shape = (case.n, case.c, 2, case.K + 1)
    if case.kind == "random":                # saturated ends, a thin middle: the shape of a real map
        h = rng.integers(0, 40, shape)
        h[..., 0] += rng.integers(0, 200000, shape[:-1])
        h[..., -1] += rng.integers(0, 9000, shape[:-1])
    elif case.kind == "sparse":
        h = rng.integers(0, 3, shape) * (rng.random(shape) < 0.1)
    elif case.kind == "big":                 # bins near 2^31 - 1: the sums leave int32 and fp32's exact integers
        h = BIG - rng.integers(0, 5, shape)
        h[0, 0] = BIG
    elif case.kind == "empty":               # planes with no valid element at all, beside ordinary ones
        h = rng.integers(0, 50, shape)
        h[0] = 0
        h[2, 1] = 0
    elif case.kind == "onesided":            # classes with no positives (class 0) or no negatives (class 1) anywhere
        h = rng.integers(0, 50, shape)
        h[:, 0, 1] = 0
        h[:, 1, 0] = 0
    else:
        raise ValueError(case.kind)
    groups, G = _groups(case.groups, case.n)
    return h.astype(np.int32), groups, G


# ------------------------------------------------------------------------------------------------ logits
def logits_case(n, c, h, w, seed):
    """Logits with exact zeros, +-0.2007 (where the sigmoid crosses 0.45 / 0.55), saturated and huge values among N(0, 16) draws."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c, h, w)) * 4).astype(F32)
    flat = x.reshape(-1)
    pick = rng.integers(0, 12, flat.size)
    for code, val in enumerate((0.0, 0.2007, -0.2007, 30.0, -30.0, 100.0, -100.0)):
        flat[pick == code] = val
    t = (rng.random((n, c, h, w)) < 0.3).astype(F32)
    return x, t
