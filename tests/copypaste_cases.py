"""Built inputs for vk.copypaste, shared by tests/test_copypaste_cpu.py (which proves the restatement on them) and
tests/test_vk_copypaste_gpu.py (which holds the kernels to the restatement).  Nothing here needs a GPU or reads a file."""
from __future__ import annotations

import numpy as np

import copypaste_ref as R

PASTE_SIZES = (24, 30, 36, 64)              # 24, 36, 64: the 4-pixel vector path; 30: the scalar one
N_ITEMS = 7                                 # items of the paste stores; the last one is blank (zero image, nothing kept)
SCALES = (0.5, 1.0, 1.7, 2.0)


# ------------------------------------------------------------------------------------------------ slot maps for boxes / alpha
def _diamond(m, cy, cx, r, s):
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    m[np.abs(yy - cy) + np.abs(xx - cx) <= r] = s


def slot_map_cases():
    """(name, slots int32 [B][h][w], max_slots)."""
    rng = np.random.default_rng(34)
    out = []
    a = np.full((2, 30, 36), -1, np.int32)
    a[0, 3:9, 4:15] = 0
    _diamond(a[0], 20, 22, 6, 2)                    # slot 1 stays empty
    a[0, 28:30, 0:3] = -2                           # a component beyond the capacity of the slot map
    a[1, 0:30, 0] = 1                               # a full column at the left border
    a[1, 29, 5:36] = 0                              # a row at the bottom border, to the right border
    a[1, 10:14, 10:14] = -2
    out.append(("30x36", a, 4))
    b = np.full((1, 64, 33), -1, np.int32)
    b[0, 0, 0] = 0
    b[0, 63, 32] = 1
    b[0, 0, 32] = 2
    b[0, 63, 0] = 3
    b[0, 20:50, 30:33] = 4
    _diamond(b[0], 30, 12, 9, 5)
    out.append(("64x33 corners", b, 8))
    out.append(("1x1 kept", np.zeros((1, 1, 1), np.int32), 1))
    out.append(("1x1 empty", np.full((2, 1, 1), -1, np.int32), 3))
    out.append(("1x1 beyond", np.full((1, 1, 1), -2, np.int32), 2))
    c = rng.integers(-2, 256, size=(2, 19, 131)).astype(np.int32)          # every slot 0..255, about one pixel in 130 each, -1 and -2 too
    c[0].reshape(-1)[:256] = np.arange(256)
    out.append(("256 slots", c, 256))
    d = rng.integers(-1, 6, size=(1, 9, 70)).astype(np.int32)              # slots at and above max_slots are ignored
    out.append(("above max_slots", d, 3))
    e = np.full((1, 45, 150), -1, np.int32)
    e[0, 5:40, 10:140] = 1                                                 # crosses two tile columns and two tile rows
    e[0, 14:18, 60:70] = -1                                                # with a hole across a tile edge
    e[0, 0:45:2, 149] = 0                                                  # one slot in many pieces along the right border
    out.append(("tile edges", e, 2))
    f = (rng.random((1, 40, 67)) < 0.5).astype(np.int32) - 1               # dense noise: every tap pattern of the binomial
    out.append(("noise", f, 1))
    return out


# ------------------------------------------------------------------------------------------------ stores for the paste
def stores(S: int):
    """(images uint8 [N_ITEMS][S][S][3], masks, kept, alpha uint8 [N_ITEMS][S][S]): random images, built components (some in the image
    corners), kept and alpha from the restatement; masks = kept plus a few pixels of their own.  Item N_ITEMS - 1 is blank."""
    rng = np.random.default_rng(1000 + S)
    images = rng.integers(0, 256, size=(N_ITEMS, S, S, 3)).astype(np.uint8)
    slots = np.full((N_ITEMS, S, S), -1, np.int32)
    q = S // 4
    _diamond(slots[0], S // 2, S // 2, q, 0)
    slots[1, 0:q, 0:q + 2] = 0                                             # top-left corner
    slots[1, S - q:S, S - q - 1:S] = 1                                     # bottom-right corner
    slots[2, 0:q - 1, S - q:S] = 0                                         # top-right
    slots[2, S - q - 2:S, 0:q] = 1                                         # bottom-left
    _diamond(slots[3], q, q, q - 2, 0)
    _diamond(slots[3], S - q, S - q - 1, q - 3, 1)
    slots[4, q:3 * q, q + 1:2 * q] = 0
    slots[4, q:q + 3, 2 * q:3 * q] = 0                                     # an L
    slots[5] = np.where(rng.random((S, S)) < 0.3, 0, -1)                   # ragged: alpha takes every value
    images[N_ITEMS - 1] = 0
    kept, alpha = R.kept_alpha_ref(slots)
    masks = kept.copy()
    masks[0, 1, 1:4] = 1
    return images, masks, kept, alpha


def scaled(t: int, s: float) -> int:
    return max(1, int(np.floor(t * s + 0.5)))


def paste_cases(S: int):
    """(base_index, pastes): six samples over the N_ITEMS stores — no record, eight overlapping ones, every d4, every scale, one-pixel
    boxes with corner donors and boxes partly or wholly outside, and a repeated base item with another count."""
    q = S // 4
    r = R.rec
    centre = (0, q, q, 2 * q + 1, 2 * q - 2)                               # donor, sx0, sy0, sw, sh: sw != sh, so a quarter turn shows
    overlapping = [r(*centre, d4, 2 + 2 * d4, 1 + d4, scaled((2 * q - 2) if d4 & 1 else (2 * q + 1), 0.8),
                     scaled((2 * q + 1) if d4 & 1 else (2 * q - 2), 0.8)) for d4 in range(8)]
    small = (3, 2, 2, q - 1, q + 1)
    every_d4 = [r(*small, d4, (d4 % 4) * (S // 4), (d4 // 4) * (S // 2) + 1, (q + 1) if d4 & 1 else (q - 1), (q - 1) if d4 & 1 else (q + 1))
                for d4 in range(8)]
    every_scale = [r(4, q - 1, q - 2, q + 3, 2 * q + 2, 3, 2 + i * 3, S // 2 - 5 * i, scaled(2 * q + 2, s), scaled(q + 3, s))
                   for i, s in enumerate(SCALES)]
    edges = [r(1, 0, 0, 1, 1, 0, 5, 5, 1, 1),                              # 1 x 1 -> 1 x 1, the donor the corner pixel
             r(1, S - 1, S - 1, 1, 1, 5, 7, 2, 3, 2),                      # 1 x 1 -> 3 x 2
             r(1, 0, 0, q + 2, q, 6, -3, -2, q + 2, q + 2),                # corner donor; over the top-left corner
             r(1, S - q - 1, S - q, q + 1, q, 1, S - 4, S - 5, q, q + 1),  # corner donor; over the bottom-right corner
             r(2, S - q, 0, q, q - 1, 4, S - 3, -4, 2 * q, 2 * q - 2),     # over the top-right corner, scale 2
             r(2, 0, S - q - 2, q, q + 2, 2, -q + 2, S - 6, q, q + 2),     # over the bottom-left corner
             r(0, q, q, q, q, 0, S, 3, q, q),                              # wholly outside: right of the image
             r(0, q, q, q, q, 7, -2 * S, -2 * S, 2 * S, 2 * S - 1)]        # the largest box there is; it ends one pixel short of the image
    base = [5, 2, N_ITEMS - 1, 3, 4, 2]
    pastes = [[], overlapping, every_d4, every_scale, edges, overlapping[2:5]]
    return base, pastes


# ------------------------------------------------------------------------------------------------ a dataset description for the bank
def bank_tables():
    """(S, boxes int32 [5][256][5], counts, content): item 0 two components whose grown boxes are neighbours without a shared pixel;
    item 1 two far apart (one below min_area 200); item 2 two whose grown boxes share one column; item 3 nothing; item 4 seventeen
    components (more than max_components = 16)."""
    S = 128
    boxes = np.empty((5, 256, 5), np.int32)
    boxes[:] = (S, S, -1, -1, 0)
    counts = np.array([2, 2, 2, 0, 17], np.int32)
    content = np.array([(0, 0, 128, 128), (16, 0, 96, 128), (0, 24, 128, 80), (0, 0, 128, 128), (0, 0, 128, 128)], np.int32)
    boxes[0, 0] = (40, 50, 69, 79, 450)
    boxes[0, 1] = (78, 50, 100, 79, 500)            # 78 - 69 = 9 apart: grown by 4 they end at column 73 and begin at 74
    boxes[1, 0] = (2, 18, 25, 40, 300)              # near the content's left and top edges: the grown box is clipped to them
    boxes[1, 1] = (90, 80, 100, 90, 61)             # too small to give
    boxes[2, 0] = (30, 10, 50, 30, 400)
    boxes[2, 1] = (58, 10, 80, 30, 400)             # 58 - 50 = 8 apart: grown by 4 they share column 54
    for s in range(17):
        x0, y0 = 4 + 14 * (s % 9), 4 + 60 * (s // 9)    # 6 x 50 each, 8 columns and 10 rows apart: alone, but too many
        boxes[4, s] = (x0, y0, x0 + 5, y0 + 49, 300)
    return S, boxes, counts, content
