"""Host side of vk.instances (no GPU): the restatement (tests/instances_ref.py) against brute force over pixel sets and against
hand-computed values, its behaviour on the reference's own label masks, and the argument checks of vk_geom_slot_map /
vk_inst_contingency / vk_inst_match through the loaded library and of the Python entry points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import geom_cases as GC
import instances_cases as IC
import instances_ref as R
from conftest import GOLDEN
from oracle import geometry_oracle as G

F64 = np.float64


# ------------------------------------------------------------------------------------------------ restatement vs brute force
@pytest.mark.parametrize("kind", ["uniform", "alternating", "blobs"])
@pytest.mark.parametrize("caps", [(1, 1), (3, 5), (64, 64)])
def test_table_equals_pixel_sets(kind, caps):
    Mp, Mg = caps
    h, w = 9, 21
    if kind == "uniform":
        p, g = IC.uniform_maps(2, h, w, Mp, Mg, seed=3)
    elif kind == "alternating":
        p, g = IC.alternating_maps(2, h, w, Mp, Mg)
    else:
        p, g = IC.blob_maps(2, h, w, Mp, Mg, seed=5)
    t = R.contingency_ref(p, g, Mp, Mg)
    assert t.dtype == np.int32 and t.shape == (2, Mp + 1, Mg + 1)
    for b in range(2):
        assert np.array_equal(t[b], R.contingency_brute(p[b], g[b], Mp, Mg))
        assert int(t[b].sum()) == h * w


def test_slot_map_on_a_built_map():
    """Three components in raster order of their first pixel: 6 px, 1 px, 4 px.  min_area 2 drops the single pixel (-1 on foreground),
    capacity 1 sends the second kept one to -2."""
    m = np.zeros((5, 9), np.float32)
    m[0:2, 0:3] = 1          # label 1, 6 px
    m[0, 5] = 1              # label 2, 1 px
    m[3:5, 6:8] = 1          # label 3, 4 px
    s, n = R.slot_map_ref(m, GC.Cfg(min_area=1, cap=8))
    assert n == 3 and s[0, 0] == 0 and s[0, 5] == 1 and s[4, 7] == 2 and s[2, 4] == -1
    s, n = R.slot_map_ref(m, GC.Cfg(min_area=2, cap=8))
    assert n == 2 and s[0, 0] == 0 and s[0, 5] == -1 and s[4, 7] == 1
    s, n = R.slot_map_ref(m, GC.Cfg(min_area=2, cap=1))
    assert n == 2 and s[0, 0] == 0 and s[0, 5] == -1 and s[4, 7] == -2
    assert sorted(np.unique(s).tolist()) == [-2, -1, 0]


# ------------------------------------------------------------------------------------------------ candidates are unique
def _all_tables():
    for c in IC.match_cases() + [IC.partition_case()]:
        for b in range(c.table.shape[0]):
            yield c.name, c.table[b], int(c.n_pred[b]), int(c.n_gt[b])
    for (h, w) in IC.SIZES:
        for (Mp, Mg) in IC.CAPS:
            for name, (p, g) in (("uniform", IC.uniform_maps(1, h, w, Mp, Mg, 1)), ("alternating", IC.alternating_maps(1, h, w, Mp, Mg)),
                                 ("blobs", IC.blob_maps(1, h, w, Mp, Mg, 2))):
                yield f"{name}_{h}x{w}_{Mp}_{Mg}", R.contingency_ref(p, g, Mp, Mg)[0], Mp, Mg
    prob, tgt = IC.squares_case()
    _, _, _, table = R.object_metrics_ref(prob, tgt, IC.E2E_CFG)
    for b in range(2):
        yield f"squares_{b}", table[b], IC.E2E_CFG.cap, IC.E2E_CFG.cap


def test_candidates_are_unique_on_every_case():
    seen = 0
    for name, table, n_pred, n_gt in _all_tables():
        Mp, Mg = table.shape[0] - 1, table.shape[1] - 1
        cand, _, _ = R.candidates(table, min(max(n_pred, 0), Mp), min(max(n_gt, 0), Mg))
        assert len({s for s, _ in cand}) == len(cand), name          # at most one per row
        assert len({t for _, t in cand}) == len(cand), name          # at most one per column
        seen += len(cand)
    assert seen > 300


# ------------------------------------------------------------------------------------------------ hand-computed PQ / SQ / RQ
def test_pq_sq_rq_by_hand():
    thr = np.array([0.5, 0.75])
    # table 1: two pred, two GT; pair (0, 0): I 8, Ap 10, Ag 8 -> U 10, IoU 0.8; pair (1, 1): I 6, Ap 9, Ag 7 -> U 10, IoU 0.6
    t = np.zeros((1, 3, 3), np.int32)
    t[0, 1, 1], t[0, 1, 0], t[0, 2, 2], t[0, 2, 0], t[0, 0, 2] = 8, 2, 6, 3, 1
    m = R.match_ref(t, [2], [2], thr)
    s = R.summarize_ref(R.totals_ref(m["per_image"]))
    assert m["pair_gt"].tolist() == [[0, 1]] and m["pair_iou"].tolist() == [[0.8, 0.6]]
    assert s["tp"].tolist() == [2, 1] and s["fp"].tolist() == [0, 1] and s["fn"].tolist() == [0, 1]
    assert s["sq"].tolist() == [(0.8 + 0.6) / 2, 0.8] and s["rq"].tolist() == [1.0, 0.5]
    assert s["pq"].tolist() == [(0.8 + 0.6) / 2, 0.8 / 2.0] and s["precision"].tolist() == [1.0, 0.5]
    assert math.isnan(s["mean_abs_d"][0]) is False and s["mean_abs_d"][0] == 0.0 and math.isnan(s["mean_rel_d"][0])
    # table 2: three pred, two GT, one pair only: I 9, Ap 9, Ag 12 -> U 12, IoU 0.75: matched at 0.5, not at 0.75 (strict)
    t = np.zeros((1, 4, 3), np.int32)
    t[0, 1, 1], t[0, 0, 1], t[0, 2, 0], t[0, 3, 2], t[0, 0, 2] = 9, 3, 5, 1, 9
    m = R.match_ref(t, [3], [2], thr, np.array([[30.0, 1.0, 1.0]]), np.array([[32.0, 1.0]]))
    s = R.summarize_ref(R.totals_ref(m["per_image"]))
    assert m["pair_gt"].tolist() == [[0, -1, -1]] and m["pair_iou"][0, 0] == 0.75 and m["pair_derr"][0, 0] == -2.0
    assert s["tp"].tolist() == [1, 0] and s["fp"].tolist() == [2, 3] and s["fn"].tolist() == [1, 2]
    assert s["sq"][0] == 0.75 and math.isnan(s["sq"][1])
    assert s["rq"][0] == 2.0 / 5.0 and s["rq"][1] == 0.0
    assert s["pq"][0] == 0.75 / 2.5 and s["pq"][1] == 0.0
    assert s["mean_abs_d"][0] == 2.0 and s["mean_rel_d"][0] == 2.0 / 32.0 and s["mean_signed_rel_d"][0] == -2.0 / 32.0
    assert s["mean_hv_rel"][0] == (32.0 / 30.0) * (32.0 / 30.0) - 1.0 and s["max_abs_d"].tolist() == [2.0, 0.0]
    # table 3: nothing on either side: every ratio has a zero denominator
    m = R.match_ref(np.full((1, 2, 2), 0, np.int32), [0], [0], thr)
    s = R.summarize_ref(R.totals_ref(m["per_image"]))
    for name in ("precision", "recall", "f1", "rq", "pq"):
        assert s[name].tolist() == [1.0, 1.0], name
    for name in ("sq", "mean_abs_d", "mean_rel_d", "mean_signed_rel_d", "mean_hv_rel"):
        assert np.isnan(s[name]).all(), name


def test_built_match_cases_say_what_they_claim():
    cases = {c.name: c for c in IC.match_cases()}

    def run(name):
        c = cases[name]
        m = R.match_ref(c.table, c.n_pred, c.n_gt, c.thr, c.dp, c.dg)
        return m, R.totals_ref(m["per_image"])

    m, t = run("iou_exactly_half")
    assert m["pair_gt"][0, 0] == -1 and t["tp"].tolist() == [0] * 10 and t["fp"][0] == 1 and t["fn"][0] == 1
    m, t = run("three_i_equals_sum")
    assert m["pair_gt"][0].tolist() == [-1, 1] and m["pair_iou"][0, 1] == 5.0 / 9.0
    m, t = run("strict_at_075")
    assert t["tp"].tolist() == [1, 0]
    m, t = run("just_below_075")
    assert t["tp"].tolist() == [1, 1]
    m, t = run("i_2_29")
    assert m["pair_gt"][0, 0] == 0 and 3 * 2 ** 29 + 2 ** 30 > 2 ** 31 - 1 and m["pair_iou"][0, 0] == float(2 ** 29) / float(2 ** 29 + 12)
    for name, fp, fn in (("empty_pred", 0, 2), ("empty_gt", 1, 0), ("both_empty", 0, 0)):
        m, t = run(name)
        assert t["tp"][0] == 0 and t["fp"][0] == fp and t["fn"][0] == fn
    m, t = run("count_above_m")
    assert t["overflow_pred"][0] == 1 and t["overflow_gt"][0] == 1 and t["n_pred_used"][0] == 2 + 2 + 0 and t["n_gt_used"][0] == 2 + 2 + 1
    m, t = run("split_and_merge")
    assert t["n_split"][0] == 1 and t["n_merge"][0] == 1 and m["pair_gt"][0].tolist() == [0, -1, 1, 3]      # the merged pred slot still covers GT slot 1 by 40 / 75
    m, t = run("zero_diagonals")
    assert t["tp"][0] == 3 and t["n_rel"][0] == 1 and t["sum_abs_d"][0] == (7.0 + 12.5) + 0.5
    m, t = run("no_diagonals")
    assert t["tp"][0] == 3 and t["tp"][1] == 2 and t["sum_abs_d"][0] == 0.0 and t["n_rel"][0] == 0 and (m["pair_derr"] == 0).all()
    m, t = run("m256_k16")
    assert t["tp"][0] == 256 and 0 < t["tp"][15] < 256 and (np.diff(t["tp"]) <= 0).all()


def test_totals_do_not_depend_on_the_batching():
    c = IC.partition_case()
    m = R.match_ref(c.table, c.n_pred, c.n_gt, c.thr, c.dp, c.dg)
    whole = R.totals_ref(m["per_image"])
    two = R.totals_ref(m["per_image"][3:], R.totals_ref(m["per_image"][:3]))
    one = None
    for b in range(7):
        one = R.totals_ref(m["per_image"][b:b + 1], one)
    assert whole.tobytes() == two.tobytes() == one.tobytes()
    assert whole["n_images"].tolist() == [7] * 10 and whole["tp"][0] > 20


# ------------------------------------------------------------------------------------------------ the reference's own label masks
@pytest.mark.parametrize("idx", [0, 3])
def test_real_mask_against_itself_and_its_erosion(idx):
    mask = IC.real_mask(GOLDEN, idx)[::4, ::4]
    cfg = GC.Cfg(thresh=0.5, min_area=1, cap=256)
    probs = mask.astype(np.float32)[None]
    s, tot, _, table = R.object_metrics_ref(probs, probs, cfg)
    n = int(tot["n_gt_used"][0])
    assert n >= 1 and tot["tp"].tolist() == [n] * 10 and s["pq"].tolist() == [1.0] * 10 and s["sq"].tolist() == [1.0] * 10
    assert s["mean_abs_d"].tolist() == [0.0] * 10 and s["max_abs_d"].tolist() == [0.0] * 10 and (tot["n_split"] == 0).all()
    assert np.all(s["mean_hv_rel"][np.isfinite(s["mean_hv_rel"])] == 0.0)
    # one-pixel erosion (3 x 3 cross) of a mask whose objects are large next to their border: every object stays a candidate
    big = IC.real_mask(GOLDEN, idx)
    er = (G.erode(big * np.uint8(255), G.ellipse_kernel(3)) > 0).astype(np.float32)[None]
    sl_p, cp = R.slot_map_ref(er[0], cfg)
    sl_g, cg = R.slot_map_ref(big.astype(np.float32), cfg)
    table = R.contingency_ref(sl_p[None], sl_g[None], 256, 256)
    m = R.match_ref(table, [cp], [cg], R.DEFAULT_THR)
    found = set(m["pair_gt"][0][m["pair_gt"][0] >= 0].tolist())
    assert cg >= 1 and cp == cg and found == set(range(cg))


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _desc(vk, h=8, w=8, cap=4):
    return vk._lib.vk_geom_desc(h, w, 0.5, 1, 0, 0, 1, cap)


def test_library_exports_and_python_exports(vk):
    L = vk.lib()
    for name in ("vk_geom_slot_map", "vk_inst_contingency", "vk_inst_match"):
        assert hasattr(L, name) and name in vk._lib.SIGNATURES
    assert "instances" in vk.__all__ and "ObjectMetrics" in vk.__all__ and "object_metrics" in vk.__all__
    assert vk.instances.STATS_DTYPE == R.STATS_DT and C.sizeof(vk._lib.vk_inst_stats) == R.STATS_DT.itemsize == 136
    assert np.array_equal(vk.instances.DEFAULT_IOU_THRESHOLDS, R.DEFAULT_THR)
    assert vk.instances.GT_PRESET == dict(bin_thresh=0.5, min_area=1, morph_kernel=1)


def test_slot_map_refuses_bad_arguments(vk):
    L = vk.lib()
    d = _desc(vk)
    need = L.vk_geom_workspace_bytes(C.byref(d), 2)
    ws = np.full(need // 8 + 64, 7, np.int64)
    base = (ws.ctypes.data + 255) // 256 * 256
    out = np.full(2 * 64, 7, np.int32)

    def call(desc=d, batch=2, ws_p=base, ws_b=need, out_p=out.ctypes.data):
        rc = L.vk_geom_slot_map(C.byref(desc) if desc is not None else None, batch, ws_p, ws_b, out_p, None)
        assert (out == 7).all() and (ws == 7).all()
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(desc=None), "null descriptor"), (dict(ws_p=None), "null buffer"), (dict(out_p=None), "null buffer"),
                     (dict(ws_b=need - 1), "workspace too small"), (dict(ws_p=base + 8), "256-byte aligned"), (dict(batch=0), "batch"),
                     (dict(out_p=out.ctypes.data + 2), "misaligned"), (dict(desc=_desc(vk, 4096, 16384 * 16)), "map size"),
                     (dict(desc=_desc(vk, 0, 8)), "map size"), (dict(desc=_desc(vk, cap=0)), "max_components")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)
    # the descriptor's own limits (4096 rows, 16384 columns) keep a map below 2^30 pixels; that bound itself is reached through
    # vk_inst_contingency, which takes h and w as they are (test_contingency_refuses_bad_arguments)


def _cont_call(vk, batch=1, h=4, w=4, Mp=2, Mg=2, pred=True, gt=True, table=True, off=0):
    L = vk.lib()
    p = np.full(64, 7, np.int32)
    g = np.full(64, 7, np.int32)
    t = np.full(1024, 7, np.int32)
    rc = L.vk_inst_contingency(batch, h, w, p.ctypes.data + off if pred else None, g.ctypes.data if gt else None, Mp, Mg,
                               t.ctypes.data if table else None, None)
    assert (t == 7).all() and (p == 7).all() and (g == 7).all()
    return rc, L.vk_last_error_string().decode()


def test_contingency_refuses_bad_arguments(vk):
    for kw, word in ((dict(Mp=0), "Mp = 0"), (dict(Mp=257), "Mp = 257"), (dict(Mg=0), "Mg = 0"), (dict(Mg=257), "Mg = 257"),
                     (dict(pred=False), "null"), (dict(gt=False), "null"), (dict(table=False), "null"), (dict(batch=0), "batch"),
                     (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=-1), "map size"), (dict(h=1 << 15, w=1 << 15), "2^30"),
                     (dict(h=1, w=1 << 30), "2^30"), (dict(h=1 << 20, w=1 << 20), "2^30"), (dict(off=2), "misaligned")):
        rc, err = _cont_call(vk, **kw)
        assert rc == -1 and word in err, (kw, err)


def _match_call(vk, batch=1, Mp=2, Mg=2, K=2, thr=(0.5, 0.75), null=None, dp=False, sp=8, sg=8, off=None):
    L = vk.lib()
    rec = R.STATS_DT.itemsize
    bufs = dict(table=np.full(64, 7, np.int32), n_pred=np.full(4, 7, np.int32), n_gt=np.full(4, 7, np.int32),
                pair_gt=np.full(16, 7, np.int32), pair_iou=np.full(16, 7.0), pair_derr=np.full(16, 7.0),
                per_image=np.full(16 * rec // 8, 7, np.int64), totals=np.full(16 * rec // 8, 7, np.int64))
    th = None if thr is None else np.asarray(thr, F64)
    d = np.full(16, 7.0)

    def ptr(name):
        if null == name:
            return None
        return bufs[name].ctypes.data + (off[1] if off and off[0] == name else 0)

    rc = L.vk_inst_match(batch, Mp, Mg, ptr("table"), ptr("n_pred"), ptr("n_gt"), K, None if th is None else th.ctypes.data,
                         d.ctypes.data if dp else None, sp, d.ctypes.data if dp else None, sg, ptr("pair_gt"), ptr("pair_iou"),
                         ptr("pair_derr"), ptr("per_image"), ptr("totals"), 0, None)
    for name, b in bufs.items():
        assert (b == 7).all(), name
    return rc, L.vk_last_error_string().decode()


def test_match_refuses_bad_arguments(vk):
    for name in ("table", "n_pred", "n_gt", "pair_gt", "pair_iou", "pair_derr", "per_image", "totals"):
        rc, err = _match_call(vk, null=name)
        assert rc == -1 and "null" in err, name
    rc, err = _match_call(vk, thr=None)
    assert rc == -1 and "null" in err
    for kw, word in ((dict(Mp=0), "Mp = 0"), (dict(Mp=257), "Mp = 257"), (dict(Mg=0), "Mg = 0"), (dict(Mg=257), "Mg = 257"),
                     (dict(K=0), "K = 0"), (dict(K=17, thr=0.5 + np.arange(17) / 64.0), "K = 17"), (dict(batch=0), "batch"),
                     (dict(off=("table", 2)), "misaligned"), (dict(off=("pair_iou", 4)), "misaligned"), (dict(off=("totals", 4)), "misaligned"),
                     (dict(dp=True, sp=12), "stride"), (dict(dp=True, sg=0), "stride")):
        rc, err = _match_call(vk, **kw)
        assert rc == -1 and word in err, (kw, err)


@pytest.mark.parametrize("thr,word", [((0.75, 0.5), "ascending"), ((0.5, 0.5), "ascending"), ((0.5, np.nan), "finite"), ((0.5, np.inf), "finite"),
                                      ((-np.inf, 0.6), "finite"), ((0.49, 0.6), "outside"), ((np.nextafter(0.5, 0.0), 0.6), "outside"),
                                      ((0.5, 1.0), "outside"), ((0.5, 1.5), "outside")])
def test_match_refuses_a_bad_threshold_list(vk, thr, word):
    rc, err = _match_call(vk, thr=thr)
    assert rc == -1 and word in err


# ------------------------------------------------------------------------------------------------ Python entry points
def test_python_entry_points_refuse_wrong_arguments(vk):
    I = vk.instances
    p, t = torch.rand(2, 8, 8), torch.zeros(2, 8, 8)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        I.detect(p)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        I.detect_gt(t)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.object_metrics(p, t)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.ObjectMetrics().update(p, t)
    with pytest.raises(ValueError):
        I.detect(p, fit="circle")
    with pytest.raises(ValueError):
        I.detect(p[0])
    with pytest.raises(ValueError):
        vk.ObjectMetrics(max_components=257)
    with pytest.raises(ValueError):
        vk.ObjectMetrics().update(p, t[:1])
    with pytest.raises(ValueError):
        vk.ObjectMetrics().compute()
    with pytest.raises(ValueError):
        I.contingency(None, None)
    for thr in ([0.75, 0.5], [0.5, 0.5], [0.4], [1.0], [float("nan")], [], np.zeros((2, 2)), 0.5 + np.arange(17) / 64.0):
        with pytest.raises(ValueError):
            vk.ObjectMetrics(iou_thresholds=thr)


def test_summarize_equals_the_restatement(vk):
    c = IC.partition_case()
    m = R.match_ref(c.table, c.n_pred, c.n_gt, c.thr, c.dp, c.dg)
    for tot in (R.totals_ref(m["per_image"]), R.totals_ref(m["per_image"][4:5]), np.zeros(3, R.STATS_DT)):
        a, b = vk.instances.summarize(tot, c.thr[:len(tot)]), R.summarize_ref(tot, c.thr[:len(tot)])
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
