"""Cases and bounds of the tiling tests (tests/test_tiling_cpu.py, tests/test_tiling_gpu.py); the arithmetic is in tiling_ref.py.

Every shape is the smallest at which a path of csrc/tiling.hip can go wrong: images below one tile (padding), exactly one tile, a last
tile pulled back so that three tiles cover a pixel per axis, the largest overlap (T/2), overlap 0 (a ramp of one step: a clamped last
tile still overlaps), a ramp that is no power of two, tiles below / at / above k_tile_pre's 32-pixel patch and k_tile_blend's 16-pixel
block, and the limit of 64 origins."""
from dataclasses import dataclass

import numpy as np

from tail_cases import K_FUNC, P_FLOOR, U32
import tiling_ref as R


@dataclass(frozen=True)
class Case:
    name: str
    h: int
    w: int
    T: int
    overlap: int

    @property
    def lattice(self):
        """The ramp is a power of two, so integer logits blend without a rounding (see lattice_logits)."""
        r = self.overlap if self.overlap > 0 else 1
        return r & (r - 1) == 0 and r <= 8

    @property
    def ntiles(self):
        return len(R.axis_origins(self.h, self.T, self.overlap)) * len(R.axis_origins(self.w, self.T, self.overlap))


CASES = [
    Case("1x1", 1, 1, 8, 2),
    Case("7x9-padded", 7, 9, 16, 4),
    Case("16x16-one-tile", 16, 16, 16, 4),
    Case("33x47-ov4-triple", 33, 47, 16, 4),
    Case("33x47-ov8-max", 33, 47, 16, 8),
    Case("40x23-ov0", 40, 23, 16, 0),
    Case("50x45-T32-ov6", 50, 45, 32, 6),
    Case("259x11-64-origins", 259, 11, 8, 4),
    Case("45x41-T40-ov8", 45, 41, 40, 8),          # two 32-pixel patches per tile side in k_tile_pre, the second one partial
]
CASE_IDS = [c.name for c in CASES]
TTAS = ["none", "hflip", "flips", "d4"]
CLASSES = [1, 3, 16]
THRESH = 0.5


def image(case, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (case.h, case.w, 3), dtype=np.uint8)


def random_logits(case, tta, C, seed=0):
    n = case.ntiles * len(R.TTA_VIEWS[tta])
    return (np.random.default_rng(seed).standard_normal((n, C, case.T, case.T)) * 3.0).astype(np.float32)


def lattice_logits(case, tta, C, seed=0):
    """Integers |l| <= 1024.  With a ramp R = 2^k <= 8, at most 8 views and at most 9 covering tiles every intermediate of the
    logit-mode blend is a multiple of 1/(8 R^2) = 2^-9 below 9 * 1024 < 2^14: 23 bits, exact in fp32.  The one rounding left is the
    division acc / wsum of two exact operands, which double rounds innocuously through fp64 (53 >= 2 * 24 + 2).  So the float32 and the
    float64 chain give the same fp32 number."""
    assert case.lattice
    n = case.ntiles * len(R.TTA_VIEWS[tta])
    return np.random.default_rng(seed).integers(-1024, 1025, (n, C, case.T, case.T)).astype(np.float32)


def max_cover(case):
    return int(R.cover_count(case.h, case.w, case.T, case.overlap).max())


def prob_bound(nv, ncover):
    """Absolute bound of an fp32 prob-mode chain (the device's or numpy's) against the float64 chain, values in [0, 1].  Relative
    errors in units of 2^-24, to first order (all terms are positive, so they carry through sums and the quotient as they are):
        p_v = 1 / (1 + expf(-l))                     K_FUNC
        sum over nv views, * (1/nv)                  nv - 1 additions; the scaling by a power of two is exact
      a pixel in one tile ends here.  Otherwise, for n covering tiles:
        w = w1(ty) * w1(tx)                          two divisions and a product: 3
        acc = acc + w * q                            1 product, n - 1 additions (the first one adds to 0)   -> acc: K_FUNC + nv + n + 2
        wsum = wsum + w                              3 from w, n - 1 additions                              -> wsum: n + 2
        acc / wsum                                   1
    The clip to [0, 1] only moves a value towards the float64 one.  P_FLOOR: the sigmoid is 0 where expf(-l) overflows."""
    k = K_FUNC + (nv - 1)
    if ncover > 1:
        k += 2 * ncover + 6
    return k * U32 * (1.0 + 1e-6) + P_FLOOR


def logit_bound(nv, ncover, mag):
    """The same count for the logit mode (no function error) on logits of magnitude at most `mag`: the weighted mean of values within
    [-mag, mag] carries its relative roundings on sums of absolute values that stay below mag."""
    k = (nv - 1) + (2 * ncover + 6 if ncover > 1 else 0)
    return k * U32 * mag * (1.0 + 1e-6)


def logit_mask_bound(nv, ncover, mag):
    """Bound of sigmoid(blended logit), what the logit mode's mask compares: the sigmoid's own error plus its slope (at most 1/4)
    times the error of its argument."""
    return K_FUNC * U32 * (1.0 + 1e-6) + P_FLOOR + 0.25 * logit_bound(nv, ncover, mag)


def mask_band(p64, bound, thresh=THRESH):
    """Pixels whose float64 probability is within the bound of the threshold: either mask value is right there."""
    return np.abs(p64 - thresh) <= bound
