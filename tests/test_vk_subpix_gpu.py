"""vk.subpix on the device against the restatement of tests/subpix_ref.py: equality of the bytes of the whole record array.

The records are built by hand (tests/subpix_cases.py), so no geometry call runs except in the last test, which takes the whole path
detect -> refine -> match at 96 x 160 against the same path through the references."""
import ctypes as C

import numpy as np
import pytest
import torch

import geom_cases as GC
import instances_cases as IC
import instances_ref as IR
import subpix_cases as SC
import subpix_ref as R

pytestmark = pytest.mark.gpu

GUARD = 512                   # bytes


def _dev():
    return torch.device("cuda:0")


def _params(vk, p):
    if p["method"] == R.CORNER:
        return vk.subpix.params("corner", win=p["win"], zero_zone=p["zero_zone"], max_iter=p["max_iter"], eps=p["eps"])
    return vk.subpix.params("lines", lo=p["lo"], hi=p["hi"], n_stations=p["n_stations"], reach=p["reach"], level=p["level"],
                            max_shift=p["max_shift"])


def _run(vk, case, recs):
    """vk_subpix_refine into a buffer filled with 0xA5 between two guards -> structured [B][M]."""
    L = vk._lib
    dev = _dev()
    B, M = recs.shape
    h, w = case.prob.shape[1:]
    prob = torch.from_numpy(case.prob).to(dev)
    raw = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).to(dev)
    counts = torch.from_numpy(case.counts.astype(np.int32)).to(dev)
    aff = None if case.affine is None else torch.from_numpy(np.ascontiguousarray(case.affine, np.float64)).to(dev)
    nb = B * M * R.QUAD_DT.itemsize
    buf = torch.full((nb + 2 * GUARD,), GC.SENT, dtype=torch.uint8, device=dev)
    out = buf[GUARD:GUARD + nb]
    assert out.data_ptr() % 8 == 0
    before = (prob.clone(), raw.clone(), counts.clone())
    dt = recs.dtype
    p = _params(vk, case.params)
    L.check(L.lib().vk_subpix_refine(C.byref(p), B, h, w, prob.data_ptr(), raw.data_ptr(), dt.itemsize, dt.fields["box"][1],
                                     dt.fields["valid"][1] if "valid" in dt.names else -1, counts.data_ptr(), M, L.ptr(aff), out.data_ptr(),
                                     L.current_stream()), "vk_subpix_refine")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == GC.SENT).all().item()) and bool((buf[GUARD + nb:] == GC.SENT).all().item()), "a guard byte was written"
    assert torch.equal(before[1], raw) and torch.equal(before[2], counts) and before[0].view(torch.int32).equal(prob.view(torch.int32))
    return out.cpu().numpy().view(R.QUAD_DT).reshape(B, M)


def _assert_equal(got, ref, tag):
    if got.tobytes() == ref.tobytes():
        return
    for idx in np.ndindex(got.shape):
        for f in R.QUAD_DT.names:
            assert got[idx][f].tobytes() == ref[idx][f].tobytes(), (tag, idx, f, got[idx][f], ref[idx][f])
    raise AssertionError((tag, "bytes differ outside the fields"))


_CASES = SC.gpu_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_refine_on_built_records(vk, case):
    recs = SC.records(case.kind, case.boxes, case.valid)
    sent = np.full(recs.shape + (R.QUAD_DT.itemsize,), GC.SENT, np.uint8).reshape(-1).view(R.QUAD_DT).reshape(recs.shape)
    ref = R.refine_ref(case.prob, recs, case.counts, case.params, case.affine, out=sent)          # untouched slots keep the sentinel
    got = _run(vk, case, recs)
    _assert_equal(got, ref, case.name)
    assert _run(vk, case, recs).tobytes() == got.tobytes(), (case.name, "second run")


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_refine_on_the_truth_draws(vk, sigma):
    """The draws the CPU file holds against analytic truth, one record per image: the device gives the restatement's bytes there too,
    so the accuracy proved on the host is the accuracy of the kernel."""
    draws = SC.square_draws(sigma)[:6]
    prob = np.stack([d.prob for d in draws])
    boxes = np.stack([d.box for d in draws])[:, None, :]
    for params in (R.corner_params(), R.lines_params()):
        case = SC.Case("draws", prob, boxes, np.ones(len(draws), np.int32), params)
        recs = SC.records("rect", boxes)
        got = _run(vk, case, recs)
        _assert_equal(got, R.refine_ref(prob, recs, case.counts, params), ("draws", sigma, params["method"]))
        err = np.abs(got["d_mean"][:, 0] - np.array([d.d_true for d in draws]))
        assert (err <= (0.8 if params["method"] == R.CORNER else 0.4)).all(), err


@pytest.mark.parametrize("fit", ["rect", "quad"])
@pytest.mark.parametrize("method", ["corner", "lines"])
def test_detect_refine_match(vk, fit, method):
    """The whole path at 96 x 160 through the Python interface, against the same path through the references."""
    prob, tgt = IC.squares_case()
    cfg = IC.E2E_CFG
    dev = _dev()
    S, I = vk.subpix, vk.instances
    tp, tt = torch.from_numpy(prob).to(dev), torch.from_numpy(tgt).to(dev)
    kw = dict(bin_thresh=cfg.thresh, min_area=cfg.min_area, morph_kernel=cfg.k, open_iter=cfg.oi, close_iter=cfg.ci)
    aff = np.array([[2.0, 3.0, 6.0], [0.0, 0.0, 1.5]])
    level = 0.5
    rkw = dict(method=method) if method == "corner" else dict(method=method, level=level)
    params = R.corner_params() if method == "corner" else R.lines_params(level=level)
    pred = I.detect(tp, fit=fit, fit_outset_px=cfg.outset, max_components=cfg.cap, **kw)
    gt = I.detect_gt(tt, fit=fit, fit_outset_px=cfg.outset, max_components=cfg.cap)
    fp, fg = S.refine(pred, tp, affine=aff, **rkw), S.refine(gt, tt, affine=aff, **rkw)
    assert isinstance(fp, S.RefinedDetections) and fp.slots is pred.slots and fp.counts is pred.counts and fp.record_bytes == 200
    assert fp.diag_offset == 192 and fp.record_dtype == R.QUAD_DT
    # the references
    gt_cfg = GC.Cfg(thresh=0.5, k=1, oi=0, ci=0, min_area=1, cap=cfg.cap, outset=cfg.outset)
    ps, pc, _, precs = IR.detect_ref(prob, cfg, fit)
    gs, gc, _, grecs = IR.detect_ref(tgt, gt_cfg, fit)
    dp, dg = np.zeros((2, cfg.cap)), np.zeros((2, cfg.cap))
    for b in range(2):
        for recs, got, d in ((precs[b], fp.records()[b], dp), (grecs[b], fg.records()[b], dg)):
            ref = R.refine_ref((prob if d is dp else tgt)[b:b + 1], recs[None], [len(recs)], params, aff[b:b + 1])[0]
            _assert_equal(got, ref, (fit, method, b))
            d[b, :len(recs)] = ref["d_mean"]
    table = IR.contingency_ref(ps, gs, cfg.cap, cfg.cap)
    m = IR.match_ref(table, pc, gc, IR.DEFAULT_THR, dp, dg)
    tot = IR.totals_ref(m["per_image"])
    res = I.match(fp, fg).cpu()
    assert res.per_image.tobytes() == m["per_image"].tobytes() and res.totals.tobytes() == tot.tobytes()
    assert res.pair_derr.tobytes() == m["pair_derr"].tobytes()
    # ObjectMetrics(refine=...) is that path; refine=None is the path without it
    om = vk.ObjectMetrics(fit=fit, max_components=cfg.cap, fit_outset_px=cfg.outset, refine=dict(affine=aff, **rkw), **kw)
    om.update(tp, tt)
    assert om.totals().tobytes() == tot.tobytes()
    plain = vk.object_metrics(tp, tt, fit=fit, max_components=cfg.cap, fit_outset_px=cfg.outset, **kw)
    ref_plain, tot_plain = IR.object_metrics_ref(prob, tgt, cfg, fit)[:2]
    assert all(plain[k].tobytes() == ref_plain[k].tobytes() for k in ref_plain)
    assert tot["tp"][0] >= 3 and tot["tp"].tolist() == tot_plain["tp"].tolist() and tot["sum_abs_d"][0] != tot_plain["sum_abs_d"][0]


def test_postprocess_lists(vk):
    prob, _ = IC.squares_case()
    cfg = IC.E2E_CFG
    tp = torch.from_numpy(prob).to(_dev())
    for fit in ("rect", "quad"):
        clean, lists = vk.subpix.postprocess(tp, fit=fit, method="lines", bin_thresh=cfg.thresh, min_area=cfg.min_area, max_components=cfg.cap)
        dets = vk.instances.detect(tp, fit=fit, bin_thresh=cfg.thresh, min_area=cfg.min_area, max_components=cfg.cap)
        fine = vk.subpix.refine(dets, tp, method="lines")
        assert torch.equal(clean, dets.clean) and len(lists) == 2
        for b in range(2):
            recs = [r for r in fine.records()[b] if r["valid"]]
            assert len(lists[b]) == len(recs) >= 1
            assert [d["area"] for d in lists[b]] == sorted((int(r["area"]) for r in recs), reverse=True)
            by_label = {int(r["label"]): r for r in recs}
            for d in lists[b]:
                r = by_label[d["label"]]
                assert d["d_mean"] == float(r["d_mean"]) and d["d1"] == float(r["d1"]) and d["box"].dtype == np.int32
                assert d["box_subpix"].shape == (4, 2) and d["box_subpix"].tobytes() == r["vs"].tobytes()
                assert np.abs(d["box_subpix_map"] - d["box"]).max() <= 6.0 and d["subpix_flags"].shape == (4,)
