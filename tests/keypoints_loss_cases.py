"""Built cases and derived error bounds for vk_kp_loss (csrc/kp_loss.hip).  No GPU is needed to import this module.

Shapes: the kernel's own constants decide where it takes another path.  A workgroup has BLOCK = 256 threads, a thread owns VEC = 4
pixels on the vector path and 1 on the scalar path, and a plane gets min(2048 // (N C), HW // WG_PIXELS) workgroups (at least 1), with
WG_PIXELS = 2048.  So a thread's loop runs more than once from HW = BLOCK VEC + 4 = 1028 (vector) and BLOCK + 1 = 257 (scalar), and a
plane takes more than one workgroup from HW = 2 WG_PIXELS = 4096 (for N C <= 1024)."""
from __future__ import annotations

import numpy as np

import keypoints_loss_ref as R
from tail_cases import K_FUNC, P_FLOOR, TINY, U32

BLOCK, VEC, WG_PIXELS = 256, 4, 2048
HW_LOOP_VECTOR = BLOCK * VEC + 4
HW_LOOP_SCALAR = BLOCK + 1
HW_TWO_WORKGROUPS = 2 * WG_PIXELS
HWS = [1, 3, 4, 7, 1023, 1024, 1028, HW_LOOP_SCALAR, HW_LOOP_SCALAR + 4, HW_LOOP_VECTOR + 4, HW_TWO_WORKGROUPS, HW_TWO_WORKGROUPS + 4]
assert HW_LOOP_VECTOR in HWS

# (name, N, C, heat planes, bce planes, alpha, beta, w_heat, w_bce, pos_weight of the BCE planes or None)
CONFIGS = [
    ("n1c1_heat", 1, 1, [0], [], 2, 4, 1.0, 1.0, None),
    ("n3c1_bce_pw", 3, 1, [], [0], 2, 4, 1.0, 0.75, 3.0),
    ("n1c2_recipe", 1, 2, [1], [0], 2, 4, 0.5, 1.0, None),
    ("n3c2_heat_first_a0b0", 3, 2, [0], [1], 0, 0, 2.0, 1.0, 0.5),
    ("n3c3_heat_middle_a1b3", 3, 3, [1], [0], 1, 3, 1.0, 2.0, None),
    ("n1c3_heat_last_a4b0", 1, 3, [2], [], 4, 0, 1.0, 1.0, None),
    ("n3c16_a8b8", 3, 16, [0, 7, 15], [1, 2, 9], 8, 8, 0.75, 0.5, 2.0),
]
KINDS = ["kp", "kp_subpixel", "random", "zeros", "ones"]
SPECIAL_LOGITS = np.array([88.0, -88.0, 104.0, -104.0, 0.0, -0.0], np.float32)
SIGMA = 2.0


def ref_cfg(config, thr: float) -> dict:
    _, N, C, heat, bce, alpha, beta, w_heat, w_bce, pw = config
    return R.cfg(heat, bce, w_heat, w_bce, alpha, beta, thr, None if pw is None else [pw if c in bce else 1.0 for c in range(C)])


def logits(N: int, C: int, HW: int, seed: int) -> np.ndarray:
    """Uniform over [-30, 30], with +-88, +-104 and +-0 at the head of every plane (as many as fit, rotated by the plane)."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.uniform(-30.0, 30.0, (N, C, HW)).astype(np.float32)
    for p in range(N * C):
        k = min(HW, len(SPECIAL_LOGITS))
        x.reshape(N * C, HW)[p, :k] = np.roll(SPECIAL_LOGITS, p)[:k]
    return x


def vertices(N: int, HW: int, subpixel: bool, seed: int) -> np.ndarray:
    """float64 [N][M][4][2] on a 1 x HW map: integer vertices (entries of exactly 1.0), or vertices one sixteenth and more off the
    pixel centres (entries just below 1.0, and at and just below table[128])."""
    rng = np.random.default_rng(2000 + seed)
    M = 2
    xs = rng.integers(0, max(HW, 1), (N, M, 4)).astype(np.float64)
    ys = np.zeros_like(xs)
    if subpixel:
        xs += rng.integers(-8, 9, xs.shape) / 16.0
        ys += rng.integers(-8, 9, xs.shape) / 16.0
        xs[:, 0, 0] = np.floor(xs[:, 0, 0]) + 0.0625                     # one sixteenth off: table[1], just below 1.0
        ys[:, 0, 0] = 0.0
        xs[:, 0, 1], ys[:, 0, 1] = np.floor(xs[:, 0, 1]) + 0.5, 0.5      # D = 128 exactly: the threshold of positive_threshold
    return np.stack([xs, ys], axis=-1)


# ------------------------------------------------------------------------------------------------ bounds
def _pow_err(k: int, eps: float) -> float:
    """q^k by k - 1 left-to-right products of a factor with relative error eps"""
    return k * eps + max(k - 1, 0) * U32


def bounds(x, y, c: dict, grad_scale: float = 1.0):
    """Counted along k_kp_reduce / k_kp_finalize / k_kp_bwd, from K_FUNC, U32, TINY and P_FLOOR of tests/tail_cases.py.

    Pieces.  p and omp are r = 1 / (1 + e) or e r with e = expf(-|x|): the sigmoid expression (K_FUNC U32 relative) and at most one more
    fp32 product: E_S = (K_FUNC + 1) U32 each.  l1p = log1pf(e) is the softplus expression, K_FUNC U32; -log p = max(-x, 0) + l1p and
    -log(1 - p) = max(x, 0) + l1p add one fp32 sum of two non-negative terms: E_L = (K_FUNC + 1) U32.  1 - y is one fp32 difference of
    an exact y: U32.  A power q^k costs k times its factor's error plus k - 1 units (_pow_err).  Every further fp32 product or sum costs
    one unit; all sums below are of terms of one sign, so the relative errors carry over to the sum.
      heat value, positive   omp^a (-log p):                    _pow_err(a, E_S) + E_L + U32
      heat value, negative   ((1 - y)^b p^a) (-log(1 - p)):     _pow_err(b, U32) + _pow_err(a, E_S) + U32 + E_L + U32
      heat gradient, pos.    -(((a p) omp^a) (-log p) + omp^a omp):  the larger term E_S + _pow_err(a, E_S) + E_L + 3 U32, the sum U32
      heat gradient, neg.    (1 - y)^b (p^a p + ((a p^a) omp) (-log(1 - p))):  the larger term _pow_err(a, E_S) + E_S + E_L + 3 U32,
                             the sum U32, the outer factor _pow_err(b, U32) + U32
      BCE value              max(x, 0) - x y + l1p + ((pw - 1) y) softplus(-x): absolute, U32 |x y| + K_FUNC U32 l1p +
                             (E_L + 3 U32) |4th term| + 3 U32 (sum of the four magnitudes) for the three sums
      BCE gradient           p - y - ((pw - 1) y) omp: absolute, E_S p + (E_S + 3 U32) |3rd term| + 2 U32 (p + y + |3rd term|)
    Up to four element values are added in fp32 before they enter the fp64 sum (4 U32 of the group's magnitude); the fp64 sums cost
    nothing to first order (1e-12 relative covers them); every reported value is rounded to fp32 once (U32 of it).  The gradient is
    ((float) coefficient g) grad_scale: three more units.
    Where expf underflows the bound is absolute: a piece is wrong by at most P_FLOOR, a product that underflows loses at most TINY, and
    the later factors (alpha <= 8, a logarithm <= 105) amplify either by less than 2^10 over at most 2^5 operations:
    A_E = 2^13 P_FLOOR + 2^15 TINY per element, TINY more for each of the last two products of the gradient."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    N, C, HW = x64.shape
    ref = R.evaluate(x64, y64, c, grad_scale)
    E_S = E_L = (K_FUNC + 1.0) * U32
    A_E = 2.0 ** 13 * P_FLOOR + 2.0 ** 15 * TINY
    a, b = c["alpha"], c["beta"]
    so = 1.0 + 1e-6                                                     # second-order terms
    gs = abs(float(grad_scale))
    b_grad = np.zeros_like(x64)
    b_heat = b_bce = 0.0
    lp, l1mp, p, omp = R.pieces(x64)
    for q in c["heat"]:
        v, g, pos = R.heat_elements(x64[:, q], y64[:, q], c)
        rv = np.where(pos, _pow_err(a, E_S) + E_L + U32, _pow_err(b, U32) + _pow_err(a, E_S) + U32 + E_L + U32)
        P = max(int(pos.sum()), 1)
        b_heat += ((np.abs(v) * (rv + 4.0 * U32) * so).sum() + v.size * A_E + 1e-12 * np.abs(v).sum()) / P
        rg = np.where(pos, E_S + _pow_err(a, E_S) + E_L + 3.0 * U32 + U32,
                      _pow_err(a, E_S) + E_S + E_L + 3.0 * U32 + U32 + _pow_err(b, U32) + U32)
        k = abs(ref["coef"][q])
        b_grad[:, q] = k * gs * (np.abs(g) * (rg + 3.0 * U32) * so + A_E) + TINY * (gs + 1.0)
    b_heat = b_heat / max(len(c["heat"]), 1) + U32 * abs(ref["heat"])
    n_all = max(N * HW * len(c["bce"]), 1)
    for q in c["bce"]:
        pw = 1.0 if c["pos_weight"] is None else c["pos_weight"][q]
        xq, yq = x64[:, q], y64[:, q]
        l1p = -lp[:, q] - np.maximum(-xq, 0.0)
        t4 = np.abs((pw - 1.0) * yq * (-lp[:, q]))
        mags = np.maximum(xq, 0.0) + np.abs(xq * yq) + l1p + t4
        ev = U32 * np.abs(xq * yq) + K_FUNC * U32 * l1p + (E_L + 3.0 * U32) * t4 + 3.0 * U32 * mags
        v, g = R.bce_elements(xq, yq, pw)
        b_bce += ((ev * so + 4.0 * U32 * np.abs(v)).sum() + v.size * A_E + 1e-12 * mags.sum()) / n_all
        t3 = np.abs((pw - 1.0) * yq * omp[:, q])
        eg = E_S * p[:, q] + (E_S + 3.0 * U32) * t3 + 2.0 * U32 * (p[:, q] + np.abs(yq) + t3)
        k = abs(ref["coef"][q])
        b_grad[:, q] = k * gs * ((eg + 3.0 * U32 * np.abs(g)) * so + A_E) + TINY * (gs + 1.0)
    b_bce += U32 * abs(ref["bce"])
    b_total = abs(c["w_heat"]) * b_heat + abs(c["w_bce"]) * b_bce + U32 * abs(ref["total"])
    return ref, dict(total=b_total, heat=b_heat, bce=b_bce, grad=b_grad)
