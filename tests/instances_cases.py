"""Built cases for vk.instances: slot maps for the contingency kernel, hand-built tables for the matching kernel, and small maps for
the whole path.  No GPU is needed to import this module; tests/test_instances_cpu.py proves the cases on the restatement alone
(tests/instances_ref.py), tests/test_vk_instances_gpu.py runs the kernels on them.

The sizes are the smallest at which the kernels can go wrong: one pixel, one wave, one lane more than a wave, rows that are no
multiple of 4, widths that are (64, 256, 200) and are not (1, 65, 63, 129) multiples of 4 (the 16-byte path and the scalar path), and
(64, 256): 16384 pixels, eight workgroups of 2048 per image."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import geom_cases as GC

SIZES = ((1, 1), (1, 64), (1, 65), (3, 63), (5, 129), (37, 200), (64, 256))
CAPS = ((1, 1), (1, 256), (256, 1), (64, 64))
E2E_H, E2E_W = 96, 160


# ------------------------------------------------------------------------------------------------ slot maps for the contingency kernel
def slot_values(M: int) -> np.ndarray:
    return np.array([-7, -2, -1] + list(range(M)) + [M, M + 1, 2 ** 30], np.int64)


def uniform_maps(B: int, h: int, w: int, Mp: int, Mg: int, seed: int):
    """Both maps drawn uniformly from {-7, -2, -1, 0 .. M - 1, M, M + 1, 2^30}."""
    rng = np.random.default_rng(seed)
    p = rng.choice(slot_values(Mp), size=(B, h, w)).astype(np.int32)
    g = rng.choice(slot_values(Mg), size=(B, h, w)).astype(np.int32)
    return p, g


def alternating_maps(B: int, h: int, w: int, Mp: int, Mg: int):
    """The pair changes at every pixel (no run is longer than one), cycling through every cell of the table."""
    n = np.arange(B * h * w, dtype=np.int64).reshape(B, h, w)
    p = (n % (Mp + 1)) - 1                                   # -1 .. Mp - 1
    g = ((n // (Mp + 1) + n) % (Mg + 1)) - 1
    return p.astype(np.int32), g.astype(np.int32)


def constant_maps(B: int, h: int, w: int):
    z = np.zeros((B, h, w), np.int32)
    return z, z.copy()


def blob_maps(B: int, h: int, w: int, Mp: int, Mg: int, seed: int):
    """What the kernel is for: mostly background with a few rectangles, the two maps shifted against each other."""
    rng = np.random.default_rng(seed)
    p = np.full((B, h, w), -1, np.int32)
    g = np.full((B, h, w), -1, np.int32)
    for b in range(B):
        for s in range(min(Mp, Mg, 6)):
            y0, x0 = int(rng.integers(0, max(h - 1, 1))), int(rng.integers(0, max(w - 1, 1)))
            hh, ww = int(rng.integers(1, 12)), int(rng.integers(1, 90))
            p[b, y0:y0 + hh, x0:x0 + ww] = s
            g[b, y0 + 1:y0 + hh + 1, x0 + 2:x0 + ww + 3] = s
    return p, g


# ------------------------------------------------------------------------------------------------ built tables for the matching kernel
@dataclass
class MatchCase:
    name: str
    table: np.ndarray           # int32 [B][Mp + 1][Mg + 1]
    n_pred: np.ndarray          # int32 [B]
    n_gt: np.ndarray
    thr: np.ndarray             # float64 [K]
    dp: np.ndarray | None = None     # float64 [B][Mp]
    dg: np.ndarray | None = None     # float64 [B][Mg]


def _table(Mp, Mg, cells, B=1):
    t = np.zeros((B, Mp + 1, Mg + 1), np.int32)
    for (b, i, j), v in cells.items():
        t[b, i, j] = v
    return t


def _counts(*v):
    return np.array(v, np.int32)


THR10 = np.arange(0.5, 1.0, 0.05)
THR16 = 0.5 + np.arange(16) / 32.0


def match_cases():
    out = []
    # I = 1, Ap = 1, Ag = 2: IoU exactly 1/2, 3 I = 3 = Ap + Ag: not a candidate
    out.append(MatchCase("iou_exactly_half", _table(2, 2, {(0, 1, 1): 1, (0, 0, 1): 1, (0, 0, 0): 10}), _counts(1), _counts(1), THR10))
    # 3 I == Ap + Ag with larger numbers (I = 4, Ap = 5, Ag = 7), next to a pair just above (I = 5, Ap = 6, Ag = 8: 15 > 14)
    out.append(MatchCase("three_i_equals_sum", _table(2, 2, {(0, 1, 1): 4, (0, 1, 0): 1, (0, 0, 1): 3, (0, 2, 2): 5, (0, 2, 0): 1, (0, 0, 2): 3}),
                         _counts(2), _counts(2), THR10))
    # I = 3, U = 4: iou = 0.75 exactly; not matched at 0.75 (strict), matched just below
    t34 = _table(1, 1, {(0, 1, 1): 3, (0, 1, 0): 1})
    out.append(MatchCase("strict_at_075", t34, _counts(1), _counts(1), np.array([0.5, 0.75])))
    out.append(MatchCase("just_below_075", t34, _counts(1), _counts(1), np.array([0.5, np.nextafter(0.75, 0.0)])))
    # I = 2^29, the largest a map of fewer than 2^30 pixels can make a pair: 3 I and Ap + Ag are each above 2^30, and a kernel that
    # forms 3 I - (Ap + Ag) or 3 I + anything in int32 is wrong here; the test is evaluated in int64
    out.append(MatchCase("i_2_29", _table(1, 1, {(0, 1, 1): 2 ** 29, (0, 1, 0): 7, (0, 0, 1): 5, (0, 0, 0): 100}), _counts(1), _counts(1), THR10,
                         np.array([[40.0]]), np.array([[41.0]])))
    # empty sides
    out.append(MatchCase("empty_pred", _table(3, 3, {(0, 0, 1): 9, (0, 0, 2): 4, (0, 0, 0): 50}), _counts(0), _counts(2), THR10))
    out.append(MatchCase("empty_gt", _table(3, 3, {(0, 1, 0): 9, (0, 0, 0): 50}), _counts(1), _counts(0), THR10))
    out.append(MatchCase("both_empty", _table(3, 3, {(0, 0, 0): 64}), _counts(0), _counts(0), THR10))
    # count > M on either side, and a negative count
    full = _table(2, 2, {(0, 1, 1): 10, (0, 2, 2): 10, (1, 1, 1): 10, (1, 2, 2): 8, (1, 2, 0): 2, (2, 1, 1): 5}, B=3)
    out.append(MatchCase("count_above_m", full, _counts(5, 2, -3), _counts(2, 7, 1), THR10,
                         np.array([[10.0, 20.0], [10.0, 20.0], [1.0, 1.0]]), np.array([[11.0, 19.0], [10.0, 20.5], [1.0, 1.0]])))
    # a split (GT slot 0 covered by pred slots 0 and 1) and a merge (pred slot 2 covers GT slots 1 and 2)
    out.append(MatchCase("split_and_merge", _table(4, 4, {(0, 1, 1): 60, (0, 2, 1): 30, (0, 3, 2): 40, (0, 3, 3): 35, (0, 4, 4): 20, (0, 0, 4): 1,
                                                           (0, 0, 0): 500}), _counts(4), _counts(4), THR10,
                         np.array([[30.0, 20.0, 44.0, 18.0]]), np.array([[42.0, 25.0, 24.0, 18.5]])))
    # dg = 0 and dp = 0: counted in the absolute sums, left out of the relative ones
    out.append(MatchCase("zero_diagonals", _table(3, 3, {(0, 1, 1): 9, (0, 2, 2): 9, (0, 3, 3): 9, (0, 3, 0): 1}), _counts(3), _counts(3), THR10,
                         np.array([[0.0, 12.5, 30.25]]), np.array([[7.0, 0.0, 29.75]])))
    # no diagonals
    out.append(MatchCase("no_diagonals", _table(3, 3, {(0, 1, 2): 9, (0, 2, 1): 9, (0, 2, 0): 2, (0, 3, 3): 9, (0, 0, 3): 8}), _counts(3), _counts(3), THR10))
    # K = 1 and K = 16, M = 256, matched pairs across the permutation s -> 255 - s with IoU i / (i + 1) style values
    cells = {}
    for s in range(256):
        cells[(0, s + 1, 256 - s)] = 50 + s
        cells[(0, s + 1, 0)] = s % 17
        cells[(0, 0, 256 - s)] = s % 5
    big = _table(256, 256, cells)
    rng = np.random.default_rng(7)
    dpb = 20.0 + 60.0 * rng.random((1, 256))
    dgb = dpb * (1.0 + 0.04 * (rng.random((1, 256)) - 0.5))
    out.append(MatchCase("m256_k1", big, _counts(256), _counts(256), np.array([0.5]), dpb, dgb))
    out.append(MatchCase("m256_k16", big, _counts(256), _counts(256), THR16, dpb, dgb))
    out.append(MatchCase("m256_partial_counts", big, _counts(200), _counts(131), THR16, dpb, dgb))
    return out


def partition_case():
    """Seven images with different tables and diagonals; fed as one batch, as (3, 4) and as seven single images with accumulate."""
    rng = np.random.default_rng(11)
    B, M = 7, 8
    t = np.zeros((B, M + 1, M + 1), np.int32)
    for b in range(B):
        for s in range(M):
            t[b, s + 1, s + 1] = int(rng.integers(20, 200))
            t[b, s + 1, 0] = int(rng.integers(0, 40))
            t[b, 0, s + 1] = int(rng.integers(0, 40))
        t[b, 0, 0] = 1000
    dp = 10.0 + 80.0 * rng.random((B, M))
    dg = dp * (1.0 + 0.1 * (rng.random((B, M)) - 0.5))
    n_pred = np.array([8, 7, 8, 3, 0, 8, 6], np.int32)
    n_gt = np.array([8, 8, 5, 3, 2, 0, 6], np.int32)
    return MatchCase("partition", t, n_pred, n_gt, THR10, dp, dg)


# ------------------------------------------------------------------------------------------------ end to end
def _square(m, cy, cx, half, angle_deg=0.0, value=1.0):
    h, w = m.shape
    a = np.deg2rad(angle_deg)
    yy, xx = np.mgrid[0:h, 0:w]
    u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a)
    v = -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
    m[(np.abs(u) <= half) & (np.abs(v) <= half)] = value
    return m


def squares_case():
    """(prob, target) [2][96][160]: rotated squares; a touching pair in the prediction that is two objects in the target; one target
    square missing from the prediction; one extra in the prediction; one target square split in two by the prediction."""
    h, w = E2E_H, E2E_W
    tgt = np.zeros((2, h, w), np.float32)
    prob = np.zeros((2, h, w), np.float32)
    # image 0: three rotated squares found slightly too large / small, one missed, one extra
    _square(tgt[0], 24, 28, 11, 45)
    _square(prob[0], 24, 29, 12, 45, 0.9)
    _square(tgt[0], 26, 80, 10, 20)
    _square(prob[0], 26, 80, 9, 20, 0.8)
    _square(tgt[0], 70, 40, 12, 0)
    _square(prob[0], 71, 41, 12, 0, 0.95)
    _square(tgt[0], 70, 120, 8, 30)                       # missed
    _square(prob[0], 25, 135, 7, 10, 0.7)                 # extra
    # image 1: two target squares one background column apart, joined in the prediction (a merge); one target square that the
    # prediction cuts in two (a split)
    tgt[1, 20:40, 20:40] = 1
    tgt[1, 20:40, 41:61] = 1
    prob[1, 20:40, 20:61] = 0.9
    _square(tgt[1], 65, 110, 14, 0)
    _square(prob[1], 65, 110, 14, 0, 0.9)
    prob[1, 40:96, 109:112] = 0.1
    return prob, tgt


def real_mask(golden_dir, idx: int) -> np.ndarray:
    """uint8 {0, 1} [h][w]: mask idx of tests/golden/real_masks.npz (bit-packed rows)."""
    z = np.load(golden_dir / "real_masks.npz")
    h, w = (int(v) for v in z[f"shape_{idx}"])
    return np.unpackbits(z[f"bits_{idx}"], axis=1)[:, :w].reshape(h, w).astype(np.uint8)


def real_pair(golden_dir, idx: int, dy: int, dx: int):
    """One golden real mask, downsized by slicing to at most 96 x 160, against a shifted and eroded copy as the 'prediction'."""
    from oracle import geometry_oracle as G
    m = real_mask(golden_dir, idx)
    sy, sx = max(1, -(-m.shape[0] // E2E_H)), max(1, -(-m.shape[1] // E2E_W))
    m = np.ascontiguousarray(m[::sy, ::sx][:E2E_H, :E2E_W])
    pad = np.zeros((E2E_H, E2E_W), np.uint8)
    pad[:m.shape[0], :m.shape[1]] = m
    er = G.erode(pad * np.uint8(255), G.ellipse_kernel(3)) > 0
    pred = np.roll(np.roll(er, dy, axis=0), dx, axis=1)
    return pred.astype(np.float32) * np.float32(0.9), pad.astype(np.float32)


E2E_CFG = GC.Cfg(thresh=0.5, k=3, oi=1, ci=1, min_area=20, cap=64, outset=2)
