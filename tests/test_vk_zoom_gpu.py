"""vk.zoom on the device against the restatement of tests/zoom_ref.py: the bytes of the window records, the bits of the gathered
network inputs, the bytes of the merged records; then the whole pass on rendered squares through a stand-in segmenter.

The three kernels run on the built cases of tests/zoom_cases.py, into sentinel-filled buffers between guards.  In the whole pass the
restatement chain computes everything itself except the two sigmoids: a float32 exp is not the same bits on the host and on the
device, so the chain is handed the probabilities the device made of inputs that are first shown to be the restatement's, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import geom_cases as GC
import subpix_ref as SR
import zoom_cases as ZC
import zoom_ref as Z

pytestmark = pytest.mark.gpu

GUARD = 512                   # bytes


def _dev():
    return torch.device("cuda:0")


def _guarded(nbytes: int, align: int = 8):
    buf = torch.full((nbytes + 2 * GUARD,), GC.SENT, dtype=torch.uint8, device=_dev())
    out = buf[GUARD:GUARD + nbytes]
    assert out.data_ptr() % align == 0
    return buf, out


def _guards_ok(buf, nbytes):
    return bool((buf[:GUARD] == GC.SENT).all().item()) and bool((buf[GUARD + nbytes:] == GC.SENT).all().item())


def _up(a: np.ndarray) -> torch.Tensor:
    """Any numpy array -> its bytes on the device, 8-byte aligned."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros((raw.size + 7) // 8, dtype=torch.int64, device=_dev()).view(torch.uint8)
    t[:raw.size] = torch.from_numpy(raw.copy()).to(_dev())
    return t


# ------------------------------------------------------------------------------------------------ windows
_WCASES = ZC.window_cases()


@pytest.mark.parametrize("case", _WCASES, ids=[c.name for c in _WCASES])
def test_windows_equal_the_restatement(vk, case):
    L = vk._lib
    recs = ZC.records(case.kind, case.boxes, case.valid)
    B, M = recs.shape
    dt = recs.dtype
    cap = case.params["max_windows"]
    sent = np.full(cap * Z.WINDOW_DT.itemsize, GC.SENT, np.uint8).view(Z.WINDOW_DT)
    ref, n_ref = Z.windows_ref(recs, case.counts, case.affine, case.sizes, case.params, out=sent)
    raw, counts, sizes = _up(recs), _up(case.counts.astype(np.int32)), _up(case.sizes.astype(np.int32))
    aff = None if case.affine is None else _up(np.asarray(case.affine, np.float64))
    p = L.vk_zoom_params(case.params["S"], cap, case.params["margin"], case.params["s_min"], case.params["s_max"])
    for _ in range(2):
        nb = cap * Z.WINDOW_DT.itemsize
        buf, out = _guarded(nb)
        nbuf, nout = _guarded(4, 4)
        L.check(L.lib().vk_zoom_windows(C.byref(p), B, raw.data_ptr(), dt.itemsize, dt.fields["box"][1],
                                        dt.fields["valid"][1] if "valid" in dt.names else -1, counts.data_ptr(), M, L.ptr(aff), sizes.data_ptr(),
                                        out.data_ptr(), nout.data_ptr(), L.current_stream()), "vk_zoom_windows")
        torch.cuda.synchronize()
        assert _guards_ok(buf, nb) and _guards_ok(nbuf, 4), "a guard byte was written"
        n = int(nout.cpu().numpy().view(np.int32)[0])
        got = out.cpu().numpy().view(Z.WINDOW_DT)
        assert n == n_ref
        for k in range(cap):
            assert got[k].tobytes() == ref[k].tobytes(), (case.name, k, got[k], ref[k])


def test_windows_over_several_chunks(vk):
    """B * max_components = 3 * 200 slots: the scan crosses three chunks of 256; every third record is invalid."""
    rng = np.random.default_rng(5)
    B, M = 3, 200
    ctr = rng.integers(40, 200, (B, M, 2))
    r = rng.integers(3, 40, (B, M))
    boxes = np.stack([ctr[..., 0] - r, ctr[..., 1] - r, ctr[..., 0] + r, ctr[..., 1] - r, ctr[..., 0] + r, ctr[..., 1] + r, ctr[..., 0] - r,
                      ctr[..., 1] + r], axis=-1).astype(np.int32)
    valid = (np.arange(B * M).reshape(B, M) % 3 != 1).astype(np.int32)
    recs = ZC.records("quad", boxes, valid)
    counts = np.array([200, 131, 777], np.int32)
    sizes = np.array([[240, 320]] * 3, np.int32)
    p = Z.params(S=48, max_windows=300)
    ref, n_ref = Z.windows_ref(recs, counts, None, sizes, p)
    dets = vk.geometry.Detections("quad", None, _up(recs).view(B, M, recs.dtype.itemsize), _up(counts).view(torch.int32)[:B], None, M)
    win, cnt = vk.zoom.windows(dets, sizes, None, S=48, max_windows=300)
    assert int(cnt.item()) == n_ref == 300
    assert win.cpu().numpy().reshape(-1).view(Z.WINDOW_DT).tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------------ gather
def _device_images():
    """The images as views with ROW_PAD bytes behind every row, so that the rows start at every alignment."""
    out = []
    for im in ZC.gather_images():
        h, w = im.shape[:2]
        base = torch.full((h, 3 * w + ZC.ROW_PAD), 77, dtype=torch.uint8, device=_dev())
        base[:, :3 * w] = torch.from_numpy(im.reshape(h, 3 * w)).to(_dev())
        view = base[:, :3 * w].unflatten(1, (w, 3))
        assert h == 1 or view.stride() == (3 * w + ZC.ROW_PAD, 3, 1)       # torch does not keep the stride of a one-row view
        out.append(view)
    return out


@pytest.mark.parametrize("S", ZC.GATHER_S)
@pytest.mark.parametrize("pad", [0, 114])
def test_gather_equals_the_restatement(vk, S, pad):
    L = vk._lib
    win = ZC.gather_windows(S)
    n = len(win)
    imgs = _device_images()
    ref = Z.gather_ref(ZC.gather_images(), win, n, S, pad)
    wdev = _up(win)
    tab = vk.zoom._image_table(imgs)
    tab_dev = torch.empty(3 * len(imgs), dtype=torch.int64, device=_dev())
    results = []
    for flags in (0, L.VK_ZOOM_STAGED):
        nb = n * 3 * S * S * 4
        buf, out = _guarded(nb, 4)
        L.check(L.lib().vk_zoom_gather(n, S, wdev.data_ptr(), len(imgs), tab, tab_dev.data_ptr(), pad, flags, out.data_ptr(), L.current_stream()),
                "vk_zoom_gather")
        torch.cuda.synchronize()
        assert _guards_ok(buf, nb), "a guard byte was written"
        got = out.cpu().numpy().view(np.float32).reshape(n, 3, S, S)
        for k in range(n):
            assert got[k].tobytes() == ref[k].tobytes(), (S, pad, flags, k, win[k], np.argwhere(got[k].view(np.int32) != ref[k].view(np.int32))[:4])
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes()                   # the staged and the direct path


def test_gather_at_scale_one_is_tile_preprocess(vk):
    """s = 1 with an integer origin inside the image: the tile of vk.tiling.tile_preprocess (tta none, T = S), an existing kernel."""
    S = 16
    img = ZC.gather_images()[3]                                           # 64 x 96
    dimg = _device_images()[3]
    grid = vk.tiling.tile_grid(64, 96, tile=S, overlap=0)
    tiles = vk.tiling.tile_preprocess(torch.from_numpy(img).to(_dev()), grid, "none", _dev())
    win = np.array([(0, t, 0, 0, float(grid.origin(t)[1]), float(grid.origin(t)[0]), 1.0) for t in range(grid.ntiles)], Z.WINDOW_DT)
    x = vk.zoom.gather([dimg], _up(win), len(win), S)
    assert torch.equal(x, tiles)


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("kind", ["rect", "quad"])
@pytest.mark.parametrize("counts", [(3, 5, 3), (3, 5, 2), (0, -1, 1)])
def test_merge_equals_the_restatement(vk, kind, counts):
    L = vk._lib
    t = ZC.merge_table(kind)
    cnt = np.array(counts, np.int32)
    B, M = t.coarse.shape
    sent_q = np.full(B * M * SR.QUAD_DT.itemsize, GC.SENT, np.uint8).view(SR.QUAD_DT).reshape(B, M)
    sent_s = np.full(B * M * 4, GC.SENT, np.uint8).view(np.int32).reshape(B, M)
    sent_f = np.full(B * M * 8, GC.SENT, np.uint8).view(np.float64).reshape(B, M)
    dt = t.recs2.dtype
    for n in (t.n, 0):
        ro, rs, rf = Z.merge_ref(ZC.MERGE_S, ZC.MERGE_AGREE, t.win, n, t.recs2, t.counts2, t.quads2, cnt, t.coarse, sent_q, sent_s, sent_f)
        win, recs2, counts2, quads2 = _up(t.win), _up(t.recs2), _up(t.counts2), _up(t.quads2)
        coarse, dcnt = _up(t.coarse), _up(cnt)
        bq, oq = _guarded(B * M * 200)
        bs, os_ = _guarded(B * M * 4, 4)
        bf, of = _guarded(B * M * 8)
        second = (recs2.data_ptr(), dt.itemsize, dt.fields["box"][1], dt.fields["valid"][1] if "valid" in dt.names else -1, counts2.data_ptr(),
                  t.recs2.shape[1], quads2.data_ptr()) if n else (None, 0, 0, -1, None, 0, None)
        L.check(L.lib().vk_zoom_merge(ZC.MERGE_S, ZC.MERGE_AGREE, n, win.data_ptr(), *second, B, M, dcnt.data_ptr(), coarse.data_ptr(),
                                      oq.data_ptr(), os_.data_ptr(), of.data_ptr(), L.current_stream()), "vk_zoom_merge")
        torch.cuda.synchronize()
        assert _guards_ok(bq, B * M * 200) and _guards_ok(bs, B * M * 4) and _guards_ok(bf, B * M * 8), "a guard byte was written"
        gs = os_.cpu().numpy().view(np.int32).reshape(B, M)
        assert gs.tolist() == rs.tolist(), (kind, counts, n)
        assert of.cpu().numpy().tobytes() == rf.tobytes()
        gq = oq.cpu().numpy().view(SR.QUAD_DT).reshape(B, M)
        for idx in np.ndindex(B, M):
            assert gq[idx].tobytes() == ro[idx].tobytes(), (kind, counts, n, idx)


# ------------------------------------------------------------------------------------------------ the whole pass
def _first_pass(vk, scenes):
    """Letterbox (ground-coloured border) -> stand-in -> sigmoid -> detect, on the device."""
    dev = _dev()
    imgs = [torch.from_numpy(sc.img).to(dev) for sc in scenes]
    x = torch.cat([vk.prepost.preprocess(im, ZC.LB, "centered", dev, pad_value=ZC.PAD)[0] for im in imgs])
    prob = torch.sigmoid(ZC.standin(x))[:, 0].contiguous()
    dets = vk.geometry.detect(prob, fit=ZC.FIT, max_components=4)
    aff = np.stack([vk.subpix.letterbox_affine(ZC.H, ZC.W, ZC.LB, "centered")] * len(scenes))
    return imgs, prob, dets, aff


def _calls(fn):
    seen = []

    def wrapped(x):
        seen.append(tuple(x.shape))
        return fn(x)
    return wrapped, seen


@pytest.mark.parametrize("method", ["corner", "lines"])
@pytest.mark.parametrize("batch", [2, 3])
def test_refine_detections_on_rendered_squares(vk, method, batch):
    """Maps with 0, 1 and 3 indentations: four windows, so batch = 3 ends on a chunk with two zero tiles and batch = 2 is two full
    chunks."""
    scenes = ZC.batch_scenes()
    imgs, prob, dets, aff = _first_pass(vk, scenes)
    assert dets.counts.tolist() == [0, 1, 3]
    rargs = dict(level=0.5) if method == "lines" else {}
    seg, seen = _calls(ZC.standin)
    fine = vk.zoom.refine_detections(seg, imgs, dets, prob, affine=aff, S=ZC.LB, method=method, batch=batch, max_components2=4,
                                     pad_value=ZC.PAD, refine_args=rargs)
    assert isinstance(fine, vk.ZoomedDetections) and fine.slots is dets.slots and fine.counts is dets.counts and fine.record_bytes == 200
    assert seen == [(batch, 3, ZC.LB, ZC.LB)] * (-(-4 // batch)) and fine.second["n"] == 4
    # the same sequence by separate calls
    Zm, S = vk.zoom, vk.subpix
    coarse = S.refine(dets, prob, method=method, affine=aff, **rargs)
    win, cnt = Zm.windows(dets, [[ZC.H, ZC.W]] * 3, aff, S=ZC.LB)
    n = int(cnt.item())
    x = Zm.gather(imgs, win, n, ZC.LB, pad_value=ZC.PAD)
    prob2 = torch.sigmoid(torch.cat([ZC.standin(x[i:i + 1]) for i in range(n)])[:, 0].float())
    dets2 = vk.geometry.detect(prob2, fit=ZC.FIT, max_components=4)
    fine2 = S.refine(dets2, prob2, method=method, affine=Zm.window_affine(win)[:n], **rargs)
    raw, status, scale = Zm.merge(win, n, dets2, fine2, coarse, ZC.LB)
    assert torch.equal(fine.raw, raw) and torch.equal(fine.status, status) and torch.equal(fine.scale, scale)
    assert torch.equal(fine.second["x"], x) and torch.equal(fine.second["prob"], prob2) and torch.equal(fine.coarse.raw, coarse.raw)
    # the restatement chain: its own windows and inputs (the device's bits), then the device's probabilities of those inputs
    host_prob2 = fine.second["prob"].cpu().numpy()

    def second_prob(xr):
        assert xr.tobytes() == fine.second["x"].cpu().numpy().tobytes()
        assert np.abs(ZC.second_pass_prob(xr) - host_prob2).max() <= 1e-6
        return host_prob2

    ref = ZC.chain_ref([sc.img for sc in scenes], prob.cpu().numpy(), method, cap=4, cap2=4, second_prob=second_prob)
    assert np.abs(np.stack([ZC.first_pass_prob(sc.img) for sc in scenes]) - prob.cpu().numpy()).max() <= 1e-6
    assert ref["n"] == 4 and win.cpu().numpy().reshape(-1).view(Z.WINDOW_DT)[:4].tobytes() == ref["win"][:4].tobytes()
    assert fine.status.cpu().numpy().tolist() == ref["status"].tolist() and fine.scale.cpu().numpy().tobytes() == ref["scale"].tobytes()
    got = fine.raw.cpu().numpy().reshape(-1).view(SR.QUAD_DT).reshape(3, 4)
    for b, cntb in enumerate((0, 1, 3)):
        for s in range(cntb):
            assert got[b, s].tobytes() == ref["out"][b, s].tobytes(), (method, b, s, got[b, s], ref["out"][b, s])
            assert int(ref["status"][b, s]) & Z.ZOOMED
    # the diagonals against the truth, in source pixels
    truth = _truth_by_slot(scenes, got)
    for (b, s), d_true in truth.items():
        err = abs(float(got[b, s]["d_mean"]) - d_true)
        bound = float(ref["scale"][b, s]) * ZC.SUBPIX_BOUND[method]
        print("zoom %s map %d slot %d: s = %.3f, |d - d_true| = %.3f (bound %.3f)" % (method, b, s, ref["scale"][b, s], err, bound))
        assert err <= bound, (method, b, s, err, bound)
    # postprocess: the same records as lists
    clean, lists = Zm.postprocess(ZC.standin, imgs, prob, fit=ZC.FIT, method=method, affine=aff, S=ZC.LB, max_components=4,
                                  zoom_args=dict(batch=batch, max_components2=4, pad_value=ZC.PAD, refine_args=rargs))
    assert torch.equal(clean, dets.clean) and [len(r) for r in lists] == [0, 1, 3]
    for b in range(3):
        by_label = {int(r["label"]): (s, r) for s, r in enumerate(got[b, :len(lists[b])])}
        for d in lists[b]:
            s, r = by_label[d["label"]]
            assert d["d_mean"] == float(r["d_mean"]) and d["box_subpix"].tobytes() == r["vs"].tobytes()
            assert d["zoom_status"] == int(ref["status"][b, s]) and d["zoom_scale"] == float(ref["scale"][b, s])


def _truth_by_slot(scenes, recs):
    """(map, slot) -> the true diagonal of the square whose centre is nearest the record's vertices' mean."""
    out = {}
    for b, sc in enumerate(scenes):
        for s in range(len(sc.squares)):
            c = recs[b, s]["vs"].reshape(4, 2).mean(axis=0)
            k = int(np.argmin([np.hypot(c[0] - q[0], c[1] - q[1]) for q in sc.squares]))
            assert np.hypot(c[0] - sc.squares[k][0], c[1] - sc.squares[k][1]) < 20.0
            out[(b, s)] = sc.d_true[k]
    assert len(out) == sum(len(sc.squares) for sc in scenes)
    return out


@pytest.mark.parametrize("method", ["corner", "lines"])
def test_zoomed_detections_match_better_than_coarse(vk, method):
    """vk.instances.match takes the zoomed detections as they are; against a ground truth that carries the true diagonals the mean
    relative diagonal error is smaller than with the coarse refinement alone."""
    scenes = ZC.batch_scenes()
    imgs, prob, dets, aff = _first_pass(vk, scenes)
    rargs = dict(level=0.5) if method == "lines" else {}
    fine = vk.zoom.refine_detections(ZC.standin, imgs, dets, prob, affine=aff, S=ZC.LB, method=method, batch=2, max_components2=4,
                                     pad_value=ZC.PAD, refine_args=rargs)
    target = (prob >= 0.5).float()
    gt = vk.instances.detect_gt(target, fit=ZC.FIT, max_components=4)
    fg = vk.subpix.refine(gt, target, method=method, affine=aff, **rargs)
    recs = fg.raw.cpu().numpy().reshape(-1).view(SR.QUAD_DT).reshape(3, 4).copy()
    for (b, s), d_true in _truth_by_slot(scenes, recs).items():
        recs[b, s]["d1"] = recs[b, s]["d2"] = recs[b, s]["d_mean"] = d_true
    fg.raw.copy_(_up(recs).view(3, 4, 200))
    zoomed = vk.instances.match(fine, fg).metrics()
    coarse = vk.instances.match(fine.coarse, fg).metrics()
    print("mean_rel_d %s: zoomed %.5f, coarse %.5f" % (method, zoomed["mean_rel_d"][0], coarse["mean_rel_d"][0]))
    assert zoomed["tp"][0] == coarse["tp"][0] == 4
    assert zoomed["mean_rel_d"][0] < coarse["mean_rel_d"][0]


def test_segmenter_measure(vk):
    """Segmenter.measure with a module that is the stand-in: the zoom pass's list, and zoom=False the coarse one."""

    class StandIn(torch.nn.Module):
        def forward(self, x):
            return ZC.standin(x)

    sc = ZC.batch_scenes()[1]
    seg = vk.Segmenter(StandIn(), img_size=ZC.LB, device=_dev())
    # the Segmenter letterboxes onto black, which the stand-in reads as indentation: keep to the detection that is the square
    for zoom in (True, False):
        rows = seg.measure(sc.img, fit=ZC.FIT, zoom=zoom, **(dict(batch=2, max_components2=4, pad_value=ZC.PAD) if zoom else {}))
        sq = [d for d in rows if abs(d["box_subpix"][:, 0].mean() - sc.squares[0][0]) < 20 and abs(d["box_subpix"][:, 1].mean() - sc.squares[0][1]) < 20]
        assert len(sq) == 1 and abs(sq[0]["d_mean"] - sc.d_true[0]) < 8.0
        assert ("zoom_status" in sq[0]) == zoom
        if zoom:
            assert sq[0]["zoom_status"] & vk.zoom.STATUS["zoomed"] and 1.0 < sq[0]["zoom_scale"] < 8.0
