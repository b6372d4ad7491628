"""vk.instances on the device against the restatement of tests/instances_ref.py: equality of bytes everywhere.

Slot map, contingency table, matching on built tables (no pixels involved), and the whole path on small built and real maps.
Measured on an MI355X when this file was written: every case passes bit for bit (figures in profiles/instances/README.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import geom_cases as GC
import instances_cases as IC
import instances_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SENT32 = -1515870811          # 0xA5A5A5A5 as int32
GUARD = 64                    # elements


def _dev():
    return torch.device("cuda:0")


def _guarded(n, dtype, fill, off=0):
    """A buffer of n elements inside a larger one filled with `fill`, starting `off` elements after a 256-byte boundary."""
    buf = torch.full((n + 2 * GUARD + off,), fill, dtype=dtype, device=_dev())
    return buf, buf[GUARD + off:GUARD + off + n]


def _guards_ok(buf, n, fill, off=0):
    return bool((buf[:GUARD + off] == fill).all().item()) and bool((buf[GUARD + off + n:] == fill).all().item())


# ================================================================================================ slot map
def _run_slot_map(vk, kind, probs, cfg):
    L = vk._lib
    lib = L.lib()
    t = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).to(_dev())
    B, h, w = (int(v) for v in t.shape)
    desc = L.vk_geom_desc(h, w, float(cfg.thresh), int(cfg.k), int(cfg.oi), int(cfg.ci), int(cfg.min_area), int(cfg.cap))
    nbytes = int(lib.vk_geom_workspace_bytes(C.byref(desc), B))
    assert nbytes > 0
    dt = GC.DET_DT if kind == "rect" else GC.QUAD_DT
    ws = torch.full((nbytes,), GC.SENT, dtype=torch.uint8, device=_dev())
    clean = torch.empty(B * h * w, dtype=torch.uint8, device=_dev())
    dets = torch.zeros(B * cfg.cap * dt.itemsize, dtype=torch.uint8, device=_dev())
    counts = torch.zeros(B, dtype=torch.int32, device=_dev())
    sbuf, slots = _guarded(B * h * w, torch.int32, SENT32)
    st = L.current_stream()
    if kind == "rect":
        L.check(lib.vk_geom_minarearect(C.byref(desc), B, t.data_ptr(), clean.data_ptr(), dets.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                        nbytes, st), "vk_geom_minarearect")
    else:
        L.check(lib.vk_geom_quadrilateral(C.byref(desc), int(cfg.outset), B, t.data_ptr(), clean.data_ptr(), dets.data_ptr(),
                                          counts.data_ptr(), ws.data_ptr(), nbytes, st), "vk_geom_quadrilateral")
    before = ws.clone()
    L.check(lib.vk_geom_slot_map(C.byref(desc), B, ws.data_ptr(), nbytes, slots.data_ptr(), st), "vk_geom_slot_map")
    torch.cuda.synchronize()
    assert torch.equal(ws, before), "vk_geom_slot_map wrote to the workspace"
    assert _guards_ok(sbuf, B * h * w, SENT32), "a guard element around the slot map was written"
    recs = dets.cpu().numpy().view(dt).reshape(B, cfg.cap)
    return slots.cpu().numpy().reshape(B, h, w), counts.cpu().numpy(), recs, clean.cpu().numpy().reshape(B, h, w)


@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["rect", "quad"])
def test_slot_map(vk, size, kind):
    h, w = size
    probs = np.stack([GC.noise(h, w, d, 77 * h + w + i) for i, d in enumerate(GC.DENSITIES)]).astype(np.float32)
    seen = set()
    for cap in (1, 3, 64):
        cfg = GC.Cfg(min_area=3, cap=cap, outset=1)
        slots, counts, recs, clean = _run_slot_map(vk, kind, probs, cfg)
        for b in range(probs.shape[0]):
            ref, n = R.slot_map_ref(probs[b], cfg)
            tag = (size, kind, cap, b)
            assert int(counts[b]) == n, tag
            assert np.array_equal(slots[b], ref), (tag, np.argwhere(slots[b] != ref)[:4].tolist())
            assert np.array_equal(clean[b] != 0, (ref >= 0) | (ref == -2)), tag
            for s in range(min(n, cap)):
                assert int((slots[b] == s).sum()) == int(recs[b, s]["area"]), (tag, s)
            seen |= set(np.unique(slots[b]).tolist())
    if h * w >= 63:
        assert -1 in seen and 0 in seen
    if size in ((37, 200), (64, 256)):
        fg_dropped = any(((GC.front(probs[b], GC.Cfg())[0] > 0) & (R.slot_map_ref(probs[b], GC.Cfg(min_area=3, cap=64))[0] == -1)).any()
                         for b in range(3))
        assert -2 in seen and fg_dropped          # a component beyond the list, and foreground below min_area


# ================================================================================================ contingency
def _run_contingency(vk, p, g, Mp, Mg, off_p=0, off_g=0):
    lib = vk.lib()
    B, h, w = p.shape
    n = B * h * w
    pb, pv = _guarded(n, torch.int32, SENT32, off_p)
    gb, gv = _guarded(n, torch.int32, SENT32, off_g)
    pv.copy_(torch.from_numpy(p.reshape(-1)))
    gv.copy_(torch.from_numpy(g.reshape(-1)))
    assert pv.data_ptr() % 16 == 4 * (off_p % 4) and gv.data_ptr() % 16 == 4 * (off_g % 4)
    cells = B * (Mp + 1) * (Mg + 1)
    tb, tv = _guarded(cells, torch.int32, SENT32)
    vk._lib.check(lib.vk_inst_contingency(B, h, w, pv.data_ptr(), gv.data_ptr(), Mp, Mg, tv.data_ptr(), vk._lib.current_stream()),
                  "vk_inst_contingency")
    torch.cuda.synchronize()
    assert _guards_ok(tb, cells, SENT32), "a guard element around the table was written"
    assert _guards_ok(pb, n, SENT32, off_p) and _guards_ok(gb, n, SENT32, off_g)
    return tv.cpu().numpy().reshape(B, Mp + 1, Mg + 1)


@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["uniform", "alternating", "blobs"])
def test_contingency(vk, size, kind):
    h, w = size
    for Mp, Mg in IC.CAPS:
        for B in (1, 3):
            if kind == "uniform":
                p, g = IC.uniform_maps(B, h, w, Mp, Mg, seed=h * 1000 + w + B)
            elif kind == "alternating":
                p, g = IC.alternating_maps(B, h, w, Mp, Mg)
            else:
                p, g = IC.blob_maps(B, h, w, Mp, Mg, seed=h + w + B)
            ref = R.contingency_ref(p, g, Mp, Mg)
            for off_p, off_g in ((0, 0), (1, 1), (1, 0)):
                tag = (size, kind, Mp, Mg, B, off_p, off_g)
                got = _run_contingency(vk, p, g, Mp, Mg, off_p, off_g)
                assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), (tag, np.argwhere(got != ref)[:4].tolist())
                assert (got.reshape(B, -1).sum(axis=1) == h * w).all(), tag
            again = _run_contingency(vk, p, g, Mp, Mg)
            assert again.tobytes() == ref.tobytes(), (size, kind, Mp, Mg, B, "second run")


def test_contingency_constant_map(vk):
    """(64, 256) all (0, 0): one counter takes h w."""
    for B in (1, 3):
        p, g = IC.constant_maps(B, 64, 256)
        for Mp, Mg in IC.CAPS:
            got = _run_contingency(vk, p, g, Mp, Mg)
            ref = np.zeros((B, Mp + 1, Mg + 1), np.int32)
            ref[:, 1, 1] = 64 * 256
            assert got.tobytes() == ref.tobytes() == R.contingency_ref(p, g, Mp, Mg).tobytes()
            assert _run_contingency(vk, p, g, Mp, Mg, 1, 1).tobytes() == ref.tobytes()


# ================================================================================================ matching on built tables
def _run_match(vk, table, n_pred, n_gt, thr, dp=None, dg=None, totals=None, record_stride=False):
    """vk_inst_match on host-built inputs.  record_stride: the diagonals sit in 96- and 104-byte records (vk_geom_det / vk_geom_quad
    strides) at the records' d_mean offsets instead of in plain arrays."""
    L = vk._lib
    lib = L.lib()
    dev = _dev()
    B, Mp, Mg = table.shape[0], table.shape[1] - 1, table.shape[2] - 1
    thr = np.ascontiguousarray(thr, np.float64)
    K = len(thr)
    rec = R.STATS_DT.itemsize
    t = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    npd = torch.from_numpy(np.asarray(n_pred, np.int32)).to(dev)
    ngd = torch.from_numpy(np.asarray(n_gt, np.int32)).to(dev)
    pgb, pg = _guarded(B * Mp, torch.int32, SENT32)
    pib, pi = _guarded(B * Mp, torch.float64, -7.0)
    pdb, pd = _guarded(B * Mp, torch.float64, -7.0)
    peb, pe = _guarded(B * K * rec // 8, torch.int64, -7)
    if totals is None:
        tob, to = _guarded(K * rec // 8, torch.int64, -7)
        acc = 0
    else:
        tob, to = _guarded(K * rec // 8, torch.int64, -7)
        to.copy_(torch.from_numpy(totals.view(np.int64).reshape(-1)))
        acc = 1
    dpp = dgp = None
    sp = sg = 8
    keep = []
    if dp is not None:
        if record_stride:
            a = np.zeros((B * Mp, 96), np.uint8)
            a[:, 88:96] = np.ascontiguousarray(dp, np.float64).reshape(-1, 1).view(np.uint8)
            b = np.zeros((B * Mg, 104), np.uint8)
            b[:, 96:104] = np.ascontiguousarray(dg, np.float64).reshape(-1, 1).view(np.uint8)
            ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            dpp, dgp, sp, sg = ta.data_ptr() + 88, tb.data_ptr() + 96, 96, 104
        else:
            ta = torch.from_numpy(np.ascontiguousarray(dp, np.float64)).to(dev)
            tb = torch.from_numpy(np.ascontiguousarray(dg, np.float64)).to(dev)
            dpp, dgp = ta.data_ptr(), tb.data_ptr()
        keep += [ta, tb]
    L.check(lib.vk_inst_match(B, Mp, Mg, t.data_ptr(), npd.data_ptr(), ngd.data_ptr(), K, thr.ctypes.data, dpp, sp, dgp, sg, pg.data_ptr(),
                              pi.data_ptr(), pd.data_ptr(), pe.data_ptr(), to.data_ptr(), acc, L.current_stream()), "vk_inst_match")
    torch.cuda.synchronize()
    assert _guards_ok(pgb, B * Mp, SENT32) and _guards_ok(pib, B * Mp, -7.0) and _guards_ok(pdb, B * Mp, -7.0)
    assert _guards_ok(peb, B * K * rec // 8, -7) and _guards_ok(tob, K * rec // 8, -7)
    return dict(pair_gt=pg.cpu().numpy().reshape(B, Mp), pair_iou=pi.cpu().numpy().reshape(B, Mp), pair_derr=pd.cpu().numpy().reshape(B, Mp),
                per_image=pe.cpu().numpy().view(R.STATS_DT).reshape(B, K), totals=to.cpu().numpy().view(R.STATS_DT).reshape(K))


def _assert_match_equal(got, ref, tot_ref, tag):
    for name in ("pair_gt", "pair_iou", "pair_derr", "per_image"):
        if got[name].tobytes() != ref[name].tobytes():
            if name == "per_image":
                for f in R.STATS_DT.names:
                    assert got[name][f].tobytes() == ref[name][f].tobytes(), (tag, name, f, got[name][f], ref[name][f])
            raise AssertionError((tag, name, got[name], ref[name]))
    for f in R.STATS_DT.names:
        assert got["totals"][f].tobytes() == tot_ref[f].tobytes(), (tag, "totals", f, got["totals"][f], tot_ref[f])


_MATCH_CASES = IC.match_cases()


@pytest.mark.parametrize("case", _MATCH_CASES, ids=[c.name for c in _MATCH_CASES])
def test_match_on_built_tables(vk, case):
    ref = R.match_ref(case.table, case.n_pred, case.n_gt, case.thr, case.dp, case.dg)
    tot = R.totals_ref(ref["per_image"])
    got = _run_match(vk, case.table, case.n_pred, case.n_gt, case.thr, case.dp, case.dg)
    _assert_match_equal(got, ref, tot, case.name)
    if case.dp is not None:
        got = _run_match(vk, case.table, case.n_pred, case.n_gt, case.thr, case.dp, case.dg, record_stride=True)
        _assert_match_equal(got, ref, tot, case.name + " (record strides)")
    # accumulate: the same images added to the totals once more
    again = _run_match(vk, case.table, case.n_pred, case.n_gt, case.thr, case.dp, case.dg, totals=tot)
    _assert_match_equal(again, ref, R.totals_ref(ref["per_image"], tot), case.name + " (accumulate)")


def test_match_partition_invariance(vk):
    c = IC.partition_case()
    ref = R.match_ref(c.table, c.n_pred, c.n_gt, c.thr, c.dp, c.dg)
    tot = R.totals_ref(ref["per_image"])
    whole = _run_match(vk, c.table, c.n_pred, c.n_gt, c.thr, c.dp, c.dg)
    _assert_match_equal(whole, ref, tot, "partition (7)")

    def part(lo, hi, totals):
        return _run_match(vk, c.table[lo:hi], c.n_pred[lo:hi], c.n_gt[lo:hi], c.thr, c.dp[lo:hi], c.dg[lo:hi], totals=totals)["totals"]

    two = part(3, 7, part(0, 3, None))
    one = None
    for b in range(7):
        one = part(b, b + 1, one)
    assert whole["totals"].tobytes() == two.tobytes() == one.tobytes() == tot.tobytes()


# ================================================================================================ end to end
def _dict_equal(a, b, tag):
    assert set(a) == set(b), (tag, set(a) ^ set(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k, a[k], b[k])


def _e2e(vk, prob, tgt, fit, cfg):
    dev = _dev()
    ref_dict, ref_tot, ref_per, ref_table = R.object_metrics_ref(prob, tgt, cfg, fit)
    kw = dict(bin_thresh=cfg.thresh, min_area=cfg.min_area, morph_kernel=cfg.k, open_iter=cfg.oi, close_iter=cfg.ci)
    tp, tt = torch.from_numpy(prob).to(dev), torch.from_numpy(tgt).to(dev)
    I = vk.instances
    # the pieces
    pred = I.detect(tp, fit=fit, fit_outset_px=cfg.outset, max_components=cfg.cap, **kw)
    gt = I.detect_gt(tt, fit=fit, fit_outset_px=cfg.outset, max_components=cfg.cap)
    ps, pc, pd, precs = R.detect_ref(prob, cfg, fit)
    gt_cfg = GC.Cfg(thresh=0.5, min_area=1, cap=cfg.cap, outset=cfg.outset)
    gs, gc, gd, grecs = R.detect_ref(tgt, gt_cfg, fit)
    assert np.array_equal(pred.slots.cpu().numpy(), ps) and np.array_equal(gt.slots.cpu().numpy(), gs)
    assert pred.counts.cpu().tolist() == pc.tolist() and gt.counts.cpu().tolist() == gc.tolist()
    for got, exp in zip(pred.records() + gt.records(), precs + grecs):
        assert got["d_mean"].tobytes() == exp["d_mean"].tobytes() and np.array_equal(got["area"], exp["area"])
    table = I.contingency(pred, gt)
    assert table.cpu().numpy().tobytes() == ref_table.tobytes()
    res = I.match(pred, gt, table=table).cpu()
    assert res.per_image.tobytes() == ref_per.tobytes() and res.totals.tobytes() == ref_tot.tobytes()
    _dict_equal(res.metrics(), ref_dict, (fit, "match"))
    # everything in one call, and over an epoch cut in two ways
    _dict_equal(vk.object_metrics(tp, tt, fit=fit, max_components=cfg.cap, fit_outset_px=cfg.outset, **kw), ref_dict, (fit, "object_metrics"))
    om = vk.ObjectMetrics(fit=fit, max_components=cfg.cap, fit_outset_px=cfg.outset, **kw)
    for b in range(prob.shape[0]):
        om.update(tp[b:b + 1], tt[b:b + 1])
    assert om.n_images == prob.shape[0] and om.totals().tobytes() == ref_tot.tobytes()
    _dict_equal(om.compute(), ref_dict, (fit, "ObjectMetrics"))
    return ref_dict, ref_tot


@pytest.mark.parametrize("fit", ["rect", "quad"])
def test_end_to_end_built_squares(vk, fit):
    prob, tgt = IC.squares_case()
    d, tot = _e2e(vk, prob, tgt, fit, IC.E2E_CFG)
    # what the case was built to hold: 5 + 1 predictions against 4 + 3 targets, a missed, an extra, a merge and a split
    assert tot["n_pred_used"][0] == 4 + 3 and tot["n_gt_used"][0] == 4 + 3
    assert tot["n_merge"][0] == 1 and tot["n_split"][0] == 1
    assert tot["tp"][0] == 3 + 0 and tot["fp"][0] == 4 and tot["fn"][0] == 4
    assert 0 < d["mean_abs_d"][0] < 4 and d["max_abs_d"][0] < 6


@pytest.mark.parametrize("idx,shift", [(0, (1, 0)), (2, (0, 1))])
def test_end_to_end_real_masks(vk, idx, shift):
    prob, tgt = IC.real_pair(GOLDEN, idx, *shift)
    assert prob.shape == (IC.E2E_H, IC.E2E_W) and tgt.sum() > 0
    cfg = GC.Cfg(thresh=0.5, k=1, min_area=4, cap=64, outset=1)
    d, tot = _e2e(vk, prob[None], tgt[None], "rect", cfg)
    assert tot["n_gt_used"][0] >= 1


# ================================================================================================ one front end
def _lists_equal(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert list(a) == list(b), (tag, i, list(a), list(b))
        for k in a:
            if isinstance(b[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, i, k, a[k], b[k])
            else:
                assert type(a[k]) is type(b[k]) and a[k] == b[k], (tag, i, k, a[k], b[k])


def _both_paths(vk, fit, tp, cap, outset, **kw):
    """detect with and without the slot map and the reference-shaped batch function on the same maps, the 200-pixel floor deciding."""
    Gm = vk.geometry
    full = vk.instances.detect(tp, fit=fit, min_area=200, fit_outset_px=outset, max_components=cap, **kw)
    bare = vk.instances.detect(tp, fit=fit, min_area=200, fit_outset_px=outset, max_components=cap, slots=False, **kw)
    assert bare.slots is None and full.slots is not None and full.slots.dtype == torch.int32 and full.slots.shape == tp.shape
    for name in ("clean", "raw", "counts"):
        a, b = getattr(full, name), getattr(bare, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (fit, name)
    if fit == "rect":
        clean, lists = vk.postprocess_minarearect_batch(tp, min_area_frac=0.0, max_components=cap, **kw)
    else:
        clean, lists = vk.postprocess_quadrilateral_batch(tp, min_area_frac=0.0, fit_outset_px=outset, max_components=cap, **kw)
    assert clean.dtype == torch.uint8 and torch.equal(clean, bare.clean)
    rows = bare.records()
    to_dicts = Gm._records if fit == "rect" else Gm._quad_records
    assert len(lists) == len(rows) == tp.shape[0]
    for b in range(len(rows)):
        _lists_equal(lists[b], to_dicts(rows[b]), (fit, b))
    return bare, rows, lists


@pytest.mark.parametrize("fit", ["rect", "quad"])
def test_front_end_paths_agree(vk, fit):
    prob, _ = IC.squares_case()
    cfg = IC.E2E_CFG
    bare, rows, lists = _both_paths(vk, fit, torch.from_numpy(prob).to(_dev()), cfg.cap, cfg.outset, bin_thresh=cfg.thresh,
                                    morph_kernel=cfg.k, open_iter=cfg.oi, close_iter=cfg.ci)
    # instances_ref.detect_ref at min_area 200: areas 545, 321, 621 / 816, 373, 373 (the extra square of image 0 is below the floor)
    assert bare.counts.cpu().tolist() == [3, 3] and [r["area"].tolist() for r in rows] == [[545, 321, 621], [816, 373, 373]]
    assert [[d["area"] for d in lst] for lst in lists] == [[621, 545, 321], [816, 373, 373]]


@pytest.mark.parametrize("fit", ["rect", "quad"])
def test_front_end_capacity(vk, fit):
    """Five 16 x 16 squares (256 px, above the floor) and two slots: the count says five, both paths list labels 1 and 2."""
    m = np.zeros((1, 48, 160), np.float32)
    for i in range(5):
        m[0, 16:32, 8 + 30 * i:24 + 30 * i] = 1.0
    bare, rows, lists = _both_paths(vk, fit, torch.from_numpy(m).to(_dev()), 2, 0, bin_thresh=0.5, morph_kernel=1, open_iter=0, close_iter=0)
    assert bare.counts.cpu().tolist() == [5] and bare.raw.shape[1] == 2
    assert rows[0]["label"].tolist() == [1, 2] and rows[0]["area"].tolist() == [256, 256]
    assert [d["label"] for d in lists[0]] == [1, 2]                                        # equal areas: the sort keeps label order


def test_invalid_quad_record_is_in_records_not_in_the_list(vk):
    case = next(c for c in GC.branch_cases() if c.name == "square2")                       # a 2 x 2 square: no quadrilateral fits
    cfg = case.cfg
    dets = vk.instances.detect(torch.from_numpy(case.probs()).to(_dev()), fit="quad", bin_thresh=cfg.thresh, min_area=cfg.min_area,
                               morph_kernel=cfg.k, open_iter=cfg.oi, close_iter=cfg.ci, fit_outset_px=cfg.outset, max_components=cfg.cap,
                               slots=False)
    rows = dets.records()
    assert len(rows) == 1 and rows[0]["valid"].tolist() == [0] and rows[0]["area"].tolist() == [4]
    assert vk.geometry._quad_records(rows[0]) == []
