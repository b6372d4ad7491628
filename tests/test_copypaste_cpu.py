"""The restatement of vk.copypaste (tests/copypaste_ref.py) proved on its own, without a GPU: the alpha against exact rational
arithmetic and the values the gain promises, the paste against the identities of the fixed-point resampling (a scale-1 paste onto its
own place, the eight turns, clipping, list order), the sampler's invariants and the donor rule on built tables; then every argument
error of the three entry points, which the library finds before it touches a stream."""
import ctypes as C
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import copypaste_cases as CC
import copypaste_ref as R


# ------------------------------------------------------------------------------------------------ alpha
def test_acc_is_the_binomial_in_exact_arithmetic():
    """acc / 4096 is the 7 x 7 binomial blur, weights C(6, i) C(6, j) / 2^12, in exact rationals."""
    for name, slots, _ in CC.slot_map_cases():
        if name not in ("30x36", "noise", "1x1 kept"):
            continue
        kept = (slots[0] >= 0).astype(np.uint8)
        acc = R.acc_ref(kept)
        h, w = kept.shape
        rng = np.random.default_rng(0)
        pts = {(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0)} | {(int(rng.integers(h)), int(rng.integers(w))) for _ in range(60)}
        for y, x in pts:
            tot = Fraction(0)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    if 0 <= y + dy < h and 0 <= x + dx < w and kept[y + dy, x + dx]:
                        tot += Fraction(comb(6, dy + 3) * comb(6, dx + 3), 4096)
            assert Fraction(int(acc[y, x]), 4096) == tot, (name, y, x)
        assert acc.min() >= 0 and acc.max() <= 4096
    assert R.acc_ref(np.ones((9, 9), np.uint8))[4, 4] == 4096 and R.alpha_of(np.array([4096]))[0] == 255


def test_alpha_values_the_gain_promises():
    for name, slots, _ in CC.slot_map_cases():
        kept, alpha = R.kept_alpha_ref(slots)
        for b in range(len(slots)):
            k = kept[b].astype(bool)
            h, w = k.shape
            p = np.zeros((h + 6, w + 6), bool)
            p[3:3 + h, 3:3 + w] = k
            near = np.zeros((h, w), bool)                       # a kept pixel within Chebyshev distance 3
            for dy in range(7):
                for dx in range(7):
                    near |= p[dy:dy + h, dx:dx + w]
            assert (alpha[b][~near] == 0).all(), name
            # a kept pixel of a fully kept 2 x 2 block: the block holds the centre tap and a neighbour on each axis, acc >= (20 + 15)^2 = 1225 >= 512
            full = np.zeros((h, w), bool)
            if h > 1 and w > 1:
                blk = k[:-1, :-1] & k[1:, :-1] & k[:-1, 1:] & k[1:, 1:]
                full[:-1, :-1] |= blk
                full[1:, :-1] |= blk
                full[:-1, 1:] |= blk
                full[1:, 1:] |= blk
            assert (alpha[b][full] == 255).all(), name
    lone = np.full((1, 9, 9), -1, np.int32)
    lone[0, 4, 4] = 0
    kept, alpha = R.kept_alpha_ref(lone)
    assert alpha[0, 4, 4] == 199 and kept.sum() == 1            # 400 * 2040 + 2048 >> 12
    assert alpha[0, 1, 1] == 0 and alpha[0, 0, 0] == 0          # acc = 1: (2040 + 2048) >> 12 = 0
    assert (R.alpha_of(np.arange(512, 4097)) == 255).all() and R.alpha_of(np.array([510]))[0] == 254


def test_boxes_by_hand():
    name, slots, M = CC.slot_map_cases()[0]
    bx = R.boxes_ref(slots, M)
    assert bx[0, 0].tolist() == [4, 3, 14, 8, 66] and bx[0, 1].tolist() == [36, 30, -1, -1, 0] and bx[0, 2].tolist() == [16, 14, 28, 26, 85]
    assert bx[1, 1].tolist() == [0, 0, 0, 29, 30] and bx[1, 0].tolist() == [5, 29, 35, 29, 31]
    name, slots, M = CC.slot_map_cases()[6]
    assert name == "above max_slots" and R.boxes_ref(slots, M)[0, :, 4].sum() == ((slots >= 0) & (slots < 3)).sum()


# ------------------------------------------------------------------------------------------------ paste
@pytest.fixture(scope="module")
def st():
    return {S: CC.stores(S) for S in CC.PASTE_SIZES}


@pytest.mark.parametrize("S", CC.PASTE_SIZES)
def test_records_of_the_cases_are_valid(S, st):
    base, pastes = CC.paste_cases(S)
    assert len(base) == len(pastes) == 6 and max(len(p) for p in pastes) == R.MAX_PASTES and len(set(base)) < len(base) < CC.N_ITEMS
    for lst in pastes:
        for r in lst:
            assert 0 <= r["donor"] < CC.N_ITEMS and 0 <= r["d4"] <= 7
            assert r["sw"] >= 1 and r["sh"] >= 1 and r["sx0"] >= 0 and r["sy0"] >= 0 and r["sx0"] + r["sw"] <= S and r["sy0"] + r["sh"] <= S
            assert 1 <= r["dw"] <= 2 * S and 1 <= r["dh"] <= 2 * S and -2 * S <= r["dx0"] <= 2 * S and -2 * S <= r["dy0"] <= 2 * S
    rgb, msk = R.compose_ref(*st[S], base, pastes)
    images, masks = st[S][0], st[S][1]
    assert np.array_equal(rgb[0], images[base[0]]) and np.array_equal(msk[0], masks[base[0]])              # no record: a copy
    for j in range(1, 6):
        assert not np.array_equal(rgb[j], images[base[j]]), j


@pytest.mark.parametrize("S", CC.PASTE_SIZES)
def test_scale_one_paste_onto_its_own_place_is_the_base(S, st):
    """U = 256 i, so fx = 0 and the four weights are 65536, 0, 0, 0: val is the source byte; (a v + (255 - a) v + 127) // 255 = v."""
    images, masks, kept, alpha = st[S]
    q = S // 4
    for item, (x0, y0, w, h) in ((0, (q - 2, q - 1, 2 * q + 5, 2 * q + 3)), (1, (0, 0, q + 4, q + 3)), (5, (0, 0, S, S))):
        assert (np.arange(w) * 256 == R.axis_src(w, w)).all()
        rgb, msk = R.compose_ref(images, masks, kept, alpha, [item], [[R.rec(item, x0, y0, w, h, 0, x0, y0, w, h)]])
        assert (masks[item] >= kept[item]).all()                # the mask of an item holds its kept pixels: the OR adds nothing
        assert np.array_equal(rgb[0], images[item]) and np.array_equal(msk[0], masks[item])


@pytest.mark.parametrize("S", CC.PASTE_SIZES)
def test_the_eight_turns(S, st):
    """A scale-1 paste onto the blank item: the result of d4 is numpy's flip / rot90 of the result of d4 = 0."""
    images, masks, kept, alpha = st[S]
    blank = CC.N_ITEMS - 1
    q = S // 4
    x0, y0, w, h = q - 1, q, 2 * q, q + 3
    assert alpha[0][y0:y0 + h, x0:x0 + w].max() == 255 and kept[0][y0:y0 + h, x0:x0 + w].any()

    def run(d4):
        tw, th = (h, w) if d4 & 1 else (w, h)
        rgb, msk = R.compose_ref(images, masks, kept, alpha, [blank], [[R.rec(0, x0, y0, w, h, d4, 1, 2, tw, th)]])
        out_rgb, out_m = rgb[0][2:2 + th, 1:1 + tw].copy(), msk[0][2:2 + th, 1:1 + tw].copy()
        rgb[0][2:2 + th, 1:1 + tw] = 0
        msk[0][2:2 + th, 1:1 + tw] = 0
        assert not rgb.any() and not msk.any()                  # nothing outside the box
        return out_rgb, out_m

    r0, m0 = run(0)
    a = alpha[0][y0:y0 + h, x0:x0 + w].astype(np.int64)[..., None]
    assert np.array_equal(r0, (a * images[0][y0:y0 + h, x0:x0 + w] + 127) // 255) and np.array_equal(m0, kept[0][y0:y0 + h, x0:x0 + w])
    seen = set()
    for d4 in range(8):
        rd, md = run(d4)
        assert np.array_equal(rd, np.rot90(np.fliplr(r0) if d4 & 4 else r0, d4 & 3)), d4
        assert np.array_equal(md, np.rot90(np.fliplr(m0) if d4 & 4 else m0, d4 & 3)), d4
        seen.add(rd.tobytes())
    assert len(seen) == 8


@pytest.mark.parametrize("S", CC.PASTE_SIZES)
def test_clipping_at_the_four_borders(S, st):
    """A box pushed over a border gives the part of the unclipped result that is left, at its place, and nothing else."""
    images, masks, kept, alpha = st[S]
    blank = CC.N_ITEMS - 1
    q = S // 4
    src = (3, 2, 1, 2 * q - 3, 2 * q - 4)
    dw, dh = CC.scaled(2 * q - 3, 1.7), CC.scaled(2 * q - 4, 1.7)
    assert dw < S and dh < S
    inside, _ = R.compose_ref(images, masks, kept, alpha, [blank], [[R.rec(*src, 4, 0, 0, dw, dh)]])
    full = inside[0][:dh, :dw]
    assert full.any()
    for dx0, dy0 in ((-5, 1), (S - dw + 4, 0), (1, -3), (0, S - dh + 6), (-dw + 1, -dh + 1), (S - 1, S - 1), (-dw, 0), (0, S), (S, S), (-2 * S, 2 * S)):
        rgb, msk = R.compose_ref(images, masks, kept, alpha, [blank], [[R.rec(*src, 4, dx0, dy0, dw, dh)]])
        want = np.zeros((S, S, 3), np.uint8)
        ya, yb, xa, xb = max(dy0, 0), min(dy0 + dh, S), max(dx0, 0), min(dx0 + dw, S)
        if ya < yb and xa < xb:
            want[ya:yb, xa:xb] = full[ya - dy0:yb - dy0, xa - dx0:xb - dx0]
        assert np.array_equal(rgb[0], want), (dx0, dy0)


def test_list_order_matters_where_two_pastes_overlap_and_only_there(st):
    S = 64
    images, masks, kept, alpha = st[S]
    a = R.rec(4, 17, 16, 15, 32, 0, 10, 10, 15, 32)             # opaque interiors of item 4's component
    b = R.rec(0, 20, 20, 24, 24, 1, 18, 20, 24, 24)
    ab, mab = R.compose_ref(images, masks, kept, alpha, [6], [[a, b]])
    ba, mba = R.compose_ref(images, masks, kept, alpha, [6], [[b, a]])
    diff = (ab[0] != ba[0]).any(axis=2)
    assert diff.any()
    ys, xs = np.nonzero(diff)
    assert xs.min() >= 18 and xs.max() <= 24 and ys.min() >= 20 and ys.max() <= 41      # the intersection of the two boxes
    assert np.array_equal(mab, mba)                             # the mask is an OR: no order
    only_a, _ = R.compose_ref(images, masks, kept, alpha, [6], [[a]])
    only_b, _ = R.compose_ref(images, masks, kept, alpha, [6], [[b]])
    out = np.ones((S, S), bool)
    out[20:42, 18:25] = False
    in_a, in_b = np.zeros((S, S), bool), np.zeros((S, S), bool)
    in_a[10:42, 10:25], in_b[20:44, 18:42] = True, True
    assert np.array_equal(ab[0][in_a & out], only_a[0][in_a & out]) and np.array_equal(ab[0][in_b & out], only_b[0][in_b & out])


def test_axis_map_without_64_bit_division():
    """The kernel takes t * 128 = a d + r apart: (2 i + 1) a + ((2 i + 1) r) // d is the quotient, and every term stays below 2^32."""
    for t, d in ((1, 1), (1, 8192), (4096, 1), (4096, 8192), (4095, 8191), (37, 63), (3000, 7), (4096, 4096), (511, 8192)):
        i = np.arange(d, dtype=np.int64)
        a, r = (t * 128) // d, (t * 128) % d
        o = 2 * i + 1
        assert (o * r).max() < 2 ** 32 and (o * a + (o * r) // d).max() < 2 ** 32
        assert np.array_equal(np.clip(o * a + (o * r) // d - 128, 0, (t - 1) * 256), R.axis_src(t, d))


# ------------------------------------------------------------------------------------------------ bank records and sampler
def test_donor_rule_on_built_tables(vk):
    S, boxes, counts, content = CC.bank_tables()
    rec = R.records_ref(boxes, counts, content, S)
    assert rec["item"].tolist() == [0, 0, 1, 1, 2, 2] + [4] * 17 and rec["slot"].tolist() == [0, 1, 0, 1, 0, 1] + list(range(17))
    assert rec["donor"].tolist() == [1, 1, 1, 0, 0, 0] + [0] * 17
    assert tuple(rec[0])[2:6] == (36, 46, 73, 83) and tuple(rec[1])[2:6] == (74, 46, 104, 83)
    assert tuple(rec[2])[2:6] == (0, 16, 29, 44)                # clipped to the content's left and top edges
    assert tuple(rec[4])[2:6] == (26, 6, 54, 34) and tuple(rec[5])[2:6] == (54, 6, 84, 34)
    got = vk.copypaste.bank_records(boxes, counts, content, S)
    assert got.dtype == R.RECORD_DT == vk.copypaste.RECORD_DTYPE and np.array_equal(got, rec)
    for kw in (dict(max_components=17), dict(min_area=50), dict(margin=3), dict(margin=0, min_area=1, max_components=1)):
        assert np.array_equal(vk.copypaste.bank_records(boxes, counts, content, S, **kw), R.records_ref(boxes, counts, content, S, **kw)), kw
    assert R.records_ref(boxes, counts, content, S, max_components=17)["donor"].sum() == 3 + 17
    assert R.records_ref(boxes, counts, content, S, margin=3)["donor"].tolist()[4:6] == [1, 1]
    assert R.default_min_area(512) == 209 and R.default_min_area(64) == 200 == vk.copypaste.default_min_area(64)


def _bank(vk, **kw):
    S, boxes, counts, content = CC.bank_tables()
    return vk.InstanceBank.from_host(S, boxes, counts, content, **kw)


def test_sampler_invariants(vk):
    bank = _bank(vk)
    assert len(bank) == 5 and len(bank.donors) == 3 and len(bank.boxes_of(4)) == 17 and len(bank.boxes_of(3)) == 0
    gap = 2
    sm = vk.CopyPasteSampler(bank, seed=5, p=0.9, max_pastes=3, gap=gap)
    n_recs = 0
    sizes = set()
    for trial in range(300):
        item = trial % 5
        recs = sm.sample(item)
        assert len(recs) <= 3
        top, left, nh, nw = bank.content[item]
        boxes = [(r["dx0"], r["dy0"], r["dx0"] + r["dw"] - 1, r["dy0"] + r["dh"] - 1) for r in recs]
        for r, b in zip(recs, boxes):
            assert set(r) == set(R.REC_FIELDS)
            d = bank.donors[(bank.donors["item"] == r["donor"]) & (bank.donors["x0"] == r["sx0"]) & (bank.donors["y0"] == r["sy0"])]
            assert len(d) == 1 and r["sw"] == d[0]["x1"] - d[0]["x0"] + 1 and r["sh"] == d[0]["y1"] - d[0]["y0"] + 1
            tw, th = (r["sh"], r["sw"]) if r["d4"] & 1 else (r["sw"], r["sh"])
            assert 0.5 - 1.0 / tw <= r["dw"] / tw <= 1.25 + 1.0 / tw and 0.5 - 1.0 / th <= r["dh"] / th <= 1.25 + 1.0 / th
            assert left <= b[0] and b[2] <= left + nw - 1 and top <= b[1] and b[3] <= top + nh - 1
            grown = (b[0] - gap, b[1] - gap, b[2] + gap, b[3] + gap)
            for o in bank.boxes_of(item):
                assert not R.meets(grown, (o["x0"], o["y0"], o["x1"], o["y1"]))
            sizes.add((r["d4"], r["donor"]))
        for i in range(len(boxes)):
            for j in range(i):
                bi = boxes[i]
                assert not R.meets((bi[0] - gap, bi[1] - gap, bi[2] + gap, bi[3] + gap), boxes[j])
        n_recs += len(recs)
    assert n_recs > 200 and len({d4 for d4, _ in sizes}) == 8 and len({d for _, d in sizes}) == 2
    a, b = vk.CopyPasteSampler(bank, seed=11), vk.CopyPasteSampler(bank, seed=11)
    assert [a.sample(i % 5) for i in range(40)] == [b.sample(i % 5) for i in range(40)]
    c = vk.CopyPasteSampler(bank, seed=12)
    assert [a.sample(i % 5) for i in range(40)] != [c.sample(i % 5) for i in range(40)]
    none = vk.CopyPasteSampler(bank, seed=1, p=0.0)
    assert all(none.sample(i % 5) == [] for i in range(50))
    empty = vk.InstanceBank.from_host(128, CC.bank_tables()[1], np.zeros(5, np.int32), CC.bank_tables()[3])
    assert all(vk.CopyPasteSampler(empty, seed=1, p=1.0).sample(i) == [] for i in range(5))
    for kw in (dict(p=1.5), dict(max_pastes=9), dict(max_pastes=0), dict(scale=(0.0, 1.0)), dict(scale=(1.5, 1.0)), dict(scale=(1.0, 2.5)),
               dict(gap=-1), dict(tries=0)):
        with pytest.raises(ValueError):
            vk.CopyPasteSampler(bank, **kw)
    with pytest.raises(ValueError):
        sm.sample(5)


# ------------------------------------------------------------------------------------------------ argument errors
def test_library_exports_and_python_exports(vk):
    L = vk.lib()
    for name in ("vk_cp_boxes", "vk_cp_alpha", "vk_cp_paste"):
        assert hasattr(L, name) and name in vk._lib.SIGNATURES
    for name in ("copypaste", "InstanceBank", "CopyPasteSampler", "CopyPaste"):
        assert name in vk.__all__ and hasattr(vk, name)
    assert C.sizeof(vk._lib.vk_cp_rec) == 40 and vk._lib.CP_REC_FIELDS == R.REC_FIELDS and vk.copypaste.MAX_PASTES == R.MAX_PASTES == 8
    assert vk._lib.vk_cp_recs_dev_bytes(3) == 3 * (8 * 40 + 4)


def _bufs():
    return dict(slots=np.full(64, 7, np.int32), boxes=np.full(64, 7, np.int32), kept=np.full(64, 7, np.uint8), alpha=np.full(64, 7, np.uint8),
                images=np.full(256, 7, np.uint8), masks=np.full(64, 7, np.uint8), base=np.full(8, 7, np.int32), recs_dev=np.full(256, 7, np.int32),
                out_rgb=np.full(256, 7, np.uint8), out_mask=np.full(64, 7, np.uint8))


def _untouched(b):
    return all((v == 7).all() for v in b.values())


def _ptrs(b, names, null, off):
    return {k: (None if null == k else b[k].ctypes.data + (off[1] if off and off[0] == k else 0)) for k in names}


def test_boxes_and_alpha_refuse_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def boxes(batch=1, h=4, w=4, M=2, null=None, off=None):
        p = _ptrs(b, ("slots", "boxes"), null, off)
        rc = L.vk_cp_boxes(batch, h, w, p["slots"], M, p["boxes"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    def alpha(batch=1, h=4, w=4, null=None, off=None):
        p = _ptrs(b, ("slots", "kept", "alpha"), null, off)
        rc = L.vk_cp_alpha(batch, h, w, p["slots"], p["kept"], p["alpha"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=0), "map size"), (dict(h=16385), "map size"),
                     (dict(w=16385), "map size"), (dict(M=0), "max_slots"), (dict(M=257), "max_slots"), (dict(null="slots"), "null buffer"),
                     (dict(null="boxes"), "null buffer"), (dict(off=("slots", 2)), "misaligned"), (dict(off=("boxes", 1)), "misaligned")):
        rc, err = boxes(**kw)
        assert rc == -1 and word in err and "vk_cp_boxes" in err, (kw, err)
    for kw, word in ((dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=16385), "map size"),
                     (dict(null="slots"), "null buffer"), (dict(null="kept"), "null buffer"), (dict(null="alpha"), "null buffer"),
                     (dict(off=("slots", 2)), "misaligned")):
        rc, err = alpha(**kw)
        assert rc == -1 and word in err and "vk_cp_alpha" in err, (kw, err)


def test_paste_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()
    S = 8
    good = dict(donor=1, sx0=1, sy0=2, sw=3, sh=4, d4=5, dx0=-3, dy0=6, dw=7, dh=16)
    names = ("images", "masks", "kept", "alpha", "base", "recs_dev", "out_rgb", "out_mask")

    def call(n=2, S=S, n_items=2, counts=(1, 2), rec=None, at=(1, 1), null=None, off=None, host_null=None):
        cnt = (C.c_int32 * 2)(*counts)
        recs = (vk._lib.vk_cp_rec * 16)()
        for k in range(2):
            for j in range(8):
                recs[8 * k + j] = vk._lib.vk_cp_rec(*(good[f] for f in R.REC_FIELDS))
        if rec is not None:
            recs[8 * at[0] + at[1]] = vk._lib.vk_cp_rec(*(dict(good, **rec)[f] for f in R.REC_FIELDS))
        p = _ptrs(b, names, null, off)
        rc = L.vk_cp_paste(n, S, n_items, p["images"], p["masks"], p["kept"], p["alpha"], p["base"], None if host_null == "counts" else cnt,
                           None if host_null == "recs" else recs, p["recs_dev"], p["out_rgb"], p["out_mask"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    cases = [(dict(n=0), "batch"), (dict(n=65536), "batch"), (dict(S=0), "S = 0"), (dict(S=4097), "S = 4097"), (dict(n_items=0), "no items"),
             (dict(host_null="counts"), "null buffer"), (dict(host_null="recs"), "null buffer"), (dict(counts=(1, 9)), "count 9"),
             (dict(counts=(-1, 0)), "count -1"), (dict(rec=dict(donor=2)), "donor 2"), (dict(rec=dict(donor=-1)), "donor -1"),
             (dict(rec=dict(sw=0)), "donor box"), (dict(rec=dict(sh=0)), "donor box"), (dict(rec=dict(sx0=-1)), "donor box"),
             (dict(rec=dict(sy0=-1)), "donor box"), (dict(rec=dict(sx0=6)), "donor box"), (dict(rec=dict(sy0=5)), "donor box"),
             (dict(rec=dict(sw=2 ** 31 - 1)), "donor box"), (dict(rec=dict(sx0=2 ** 31 - 1)), "donor box"), (dict(rec=dict(d4=8)), "d4 8"),
             (dict(rec=dict(d4=-1)), "d4 -1"), (dict(rec=dict(dw=0)), "destination size"), (dict(rec=dict(dh=0)), "destination size"),
             (dict(rec=dict(dw=17)), "destination size"), (dict(rec=dict(dh=17)), "destination size"), (dict(rec=dict(dx0=-17)), "destination origin"),
             (dict(rec=dict(dx0=17)), "destination origin"), (dict(rec=dict(dy0=-17)), "destination origin"), (dict(rec=dict(dy0=17)), "destination origin"),
             (dict(rec=dict(dy0=-2 ** 31)), "destination origin"), (dict(rec=dict(d4=9), at=(0, 0)), "sample 0 record 0")]
    cases += [(dict(null=k), "null buffer") for k in names]
    cases += [(dict(off=(k, 2)), "misaligned") for k in names]
    for kw, word in cases:
        rc, err = call(**kw)
        assert rc == -1 and word in err and "vk_cp_paste" in err, (kw, err)
    # a record behind a sample's count is not looked at: the same call with a bad record there passes the checks (and would launch), so
    # only its message is compared: sample 0 has one record, its second one is bad, the error is that of the next bad thing
    rc, err = call(rec=dict(d4=9), at=(0, 1), n_items=0)
    assert rc == -1 and "no items" in err
    rc, err = call(rec=dict(d4=9), at=(0, 1), counts=(1, 9))
    assert rc == -1 and "count 9" in err


def test_python_entry_points_refuse_wrong_arguments(vk):
    with pytest.raises(ValueError, match="DeviceDataset"):
        vk.InstanceBank("no")
    with pytest.raises(ValueError, match="DeviceDataset"):
        vk.CopyPaste("no")
    with pytest.raises(ValueError, match="at most 8"):
        vk.copypaste._recs_array([[dict(zip(R.REC_FIELDS, range(10)))] * 9])
    counts, recs = vk.copypaste._recs_array([[], [R.rec(*range(10))]])
    assert list(counts) == [0, 1] and len(recs) == 16 and [getattr(recs[8], f) for f in R.REC_FIELDS] == list(range(10))
    with pytest.raises(ValueError, match="boxes"):
        vk.copypaste.bank_records(np.zeros((2, 4, 4)), [0, 0], np.zeros((2, 4)), 64)
