"""vk.render on the device against the restatement of tests/render_ref.py: canvas bytes, primitive-record bytes, drawn and skipped
counts; then the whole path on rendered squares through a stand-in segmenter, and Segmenter.render.

The four kernels run on the built cases of tests/render_cases.py, into sentinel-filled buffers between guards: guards, stride padding
and unwritten slots must come back untouched."""
import ctypes as C
import itertools
from functools import lru_cache

import numpy as np
import pytest
import torch

import geom_cases as GC
import render_cases as RC
import render_ref as R
import subpix_ref as SR
import zoom_cases as ZC

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


def _strided(img: np.ndarray, pad: int, fill: int = 77) -> torch.Tensor:
    """uint8 [h][w][c] or [h][w] -> a device view whose rows are `pad` bytes apart beyond their length."""
    h, w = img.shape[:2]
    row = img.reshape(h, -1)
    base = torch.full((h, row.shape[1] + pad), fill, dtype=torch.uint8, device=_dev())
    base[:, :row.shape[1]] = torch.from_numpy(np.ascontiguousarray(row)).to(_dev())
    return base, base[:, :row.shape[1]]


# ------------------------------------------------------------------------------------------------ panels
_PCASES = RC.panel_cases()


@pytest.mark.parametrize("rgb", [False, True], ids=["bgr", "rgb"])
@pytest.mark.parametrize("case", _PCASES, ids=[c.name for c in _PCASES])
def test_val_panels_equal_the_restatement(vk, case, rgb):
    L = vk._lib
    N, _, H, W = case.x.shape
    stride = 12 * W + case.pad
    sent = np.full((N, H, stride), GC.SENT, np.uint8)
    ref = R.val_panels_ref(case.x, case.y, case.prob, color=case.color, rgb=rgb, out=sent, row_stride=stride)
    x, y, pr = (torch.from_numpy(a).to(_dev()) for a in (case.x, case.y, case.prob))
    nb = N * H * stride
    buf, out = _guarded(nb, 1)
    bl = L.vk_render_blend((C.c_uint8 * 3)(*case.color), 0, 1.0, 0.35, 0.0)
    L.check(L.lib().vk_render_val_panels(N, H, W, x.data_ptr(), y.data_ptr(), pr.data_ptr(), (C.c_double * 3)(*R.MEAN), (C.c_double * 3)(*R.STD),
                                         C.byref(bl), L.VK_RENDER_RGB if rgb else 0, out.data_ptr(), stride, L.current_stream()), "vk_render_val_panels")
    torch.cuda.synchronize()
    assert _guards_ok(buf, nb), "a guard byte was written"
    got = out.cpu().numpy().reshape(N, H, stride)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:6]
    assert (got[:, :, 12 * W:] == GC.SENT).all()
    # the Python entry point: the same canvas without the padding
    can = vk.render.val_panels(x, y, pr, color=case.color, order="rgb" if rgb else "bgr")
    assert can.shape == (N, H, 4 * W, 3) and np.array_equal(can.cpu().numpy().reshape(N, H, 12 * W), ref[:, :, :12 * W])


def test_save_individual_visuals(vk, tmp_path):
    """The files PIL reads back are the canvas within JPEG error: the bound is what a PIL round trip of the restatement's canvas at the
    same quality loses."""
    import io

    from PIL import Image
    case = _PCASES[2]
    rng = np.random.default_rng(3)
    x = np.concatenate([case.x, rng.normal(0, 1, case.x.shape).astype(np.float32)])
    y = np.concatenate([case.y, case.y])
    pr = np.concatenate([case.prob, rng.random(case.prob.shape).astype(np.float32)])
    N, _, H, W = x.shape
    names = ["a_%d" % i for i in range(N)]
    for quality in (95, 60):
        out_dir = tmp_path / ("q%d" % quality)
        vk.render.save_individual_visuals(*(torch.from_numpy(a).to(_dev()) for a in (x, y, pr)), names, out_dir, quality=quality)
        ref = R.val_panels_ref(x, y, pr, rgb=True).reshape(N, H, 4 * W, 3)
        for i, name in enumerate(names):
            got = np.asarray(Image.open(out_dir / (name + ".jpg")).convert("RGB")).astype(int)
            bio = io.BytesIO()
            Image.fromarray(ref[i]).save(bio, format="JPEG", quality=quality)
            trip = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert("RGB")).astype(int)
            bound = int(np.abs(trip - ref[i].astype(int)).max())
            err = int(np.abs(got - ref[i].astype(int)).max())
            print("quality %d image %d: max |file - canvas| = %d (round trip of the restatement: %d)" % (quality, i, err, bound))
            assert got.shape == (H, 4 * W, 3) and err <= bound


# ------------------------------------------------------------------------------------------------ primitives
_RCASES = RC.prim_cases()


@pytest.mark.parametrize("case", _RCASES, ids=[c.name for c in _RCASES])
def test_primitives_equal_the_restatement(vk, case):
    L = vk._lib
    B, M = case.recs.shape
    dt = case.recs.dtype
    sent = np.full(B * M * R.PRIM_DT.itemsize, GC.SENT, np.uint8).view(R.PRIM_DT).reshape(B, M)
    ref, drawn_ref, skipped_ref = R.primitives_ref(case.recs, case.counts, case.mode, case.field, case.affine, thickness=case.thickness,
                                                   text_scale=case.text_scale, out=sent)
    raw, counts = _up(case.recs), _up(case.counts.astype(np.int32))
    aff = None if case.affine is None else _up(np.asarray(case.affine, np.float64))
    st = vk.render._style(R.PALETTE, R.DIAG_COLOR, case.thickness, case.text_scale)
    nb = B * M * R.PRIM_DT.itemsize
    for _ in range(2):
        buf, out = _guarded(nb)
        bd, od = _guarded(4 * B, 4)
        bs, os_ = _guarded(4 * B, 4)
        L.check(L.lib().vk_render_primitives(B, raw.data_ptr(), dt.itemsize, dt.fields[case.field][1],
                                             dt.fields["valid"][1] if "valid" in dt.names else -1, dt.fields["d_mean"][1],
                                             dt.fields["cx"][1] if "cx" in dt.names else -1, case.mode, counts.data_ptr(), M, L.ptr(aff), C.byref(st),
                                             out.data_ptr(), od.data_ptr(), os_.data_ptr(), L.current_stream()), "vk_render_primitives")
        torch.cuda.synchronize()
        assert _guards_ok(buf, nb) and _guards_ok(bd, 4 * B) and _guards_ok(bs, 4 * B), "a guard byte was written"
        assert od.cpu().numpy().view(np.int32).tolist() == drawn_ref.tolist()
        assert os_.cpu().numpy().view(np.int32).tolist() == skipped_ref.tolist()
        got = out.cpu().numpy().view(R.PRIM_DT).reshape(B, M)
        for idx in np.ndindex(B, M):
            assert got[idx].tobytes() == ref[idx].tobytes(), (case.name, idx, got[idx], ref[idx])


def test_primitives_with_more_slots_than_threads(vk):
    """max_components = 600 with 520 used: a thread takes more than one slot, the counts cross the waves."""
    rng = np.random.default_rng(9)
    M = 600
    ctr, rad = rng.integers(0, 3000, (1, M, 2)), rng.integers(1, 50, (1, M))
    boxes = np.stack([ctr[..., 0] - rad, ctr[..., 1] - rad, ctr[..., 0] + rad, ctr[..., 1] - rad, ctr[..., 0] + rad, ctr[..., 1] + rad,
                      ctr[..., 0] - rad, ctr[..., 1] + rad], axis=-1)
    boxes[0, ::37, 0] = R.MAX_COORD + 5                                   # some skipped
    recs = RC._records("quad", boxes, rng.integers(1, 40, (1, M)), rng.uniform(0, 2000, (1, M)), valid=(np.arange(M) % 5 != 2)[None, :])
    counts = np.array([520], np.int32)
    ref, drawn_ref, skipped_ref = R.primitives_ref(recs, counts, R.COORD_BOX, "box")
    dets = vk.geometry.Detections("quad", None, _up(recs).view(1, M, recs.dtype.itemsize), _up(counts).view(torch.int32)[:1], None, M)
    prims, drawn, skipped = vk.render.primitives(dets)
    assert drawn.tolist() == drawn_ref.tolist() and skipped.tolist() == skipped_ref.tolist() and skipped_ref[0] > 5 and drawn_ref[0] > 256
    assert prims.cpu().numpy().reshape(-1).view(R.PRIM_DT).tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------------ draw
_DCASES = RC.draw_cases()


@lru_cache(maxsize=None)
def _draw_reference(i: int):
    c = _DCASES[i]
    return R.draw_ref(c.src, c.mask, c.thresh, c.color, 1.0, c.alpha, prims=c.prims, drawn=c.drawn)


@pytest.mark.parametrize("i", range(len(_DCASES)), ids=[c.name for c in _DCASES])
def test_draw_equals_the_restatement(vk, i):
    """Every subset of the three outputs, the tile-binned and the direct form, strided sources and outputs."""
    L = vk._lib
    c = _DCASES[i]
    ref = _draw_reference(i)
    h, w = c.src.shape[:2]
    _, src = _strided(c.src, RC.ROW_PAD)
    src = src.unflatten(1, (w, 3))
    if c.mask.dtype == np.uint8:
        _, mask = _strided(c.mask, 3)
        kind, mstride = L.VK_RENDER_MASK_U8, w + 3
    else:
        mask = torch.from_numpy(np.pad(c.mask, ((0, 0), (0, 2)))).to(_dev())[:, :w]
        kind, mstride = L.VK_RENDER_MASK_F32, 4 * (w + 2)
    M = 1 if c.prims is None else len(c.prims)
    prims = None if c.prims is None else _up(c.prims)
    drawn = None if c.prims is None else _up(np.array([c.drawn], np.int32))
    bl = L.vk_render_blend((C.c_uint8 * 3)(*c.color), 0, 1.0, c.alpha, 0.0)
    view_dev = torch.empty(11, dtype=torch.int64, device=_dev())
    ostride = 3 * w + 7
    nb = h * ostride
    for subset in itertools.product((False, True), repeat=3):
        if not any(subset):
            continue
        results = []
        for flags in (0, L.VK_RENDER_DIRECT):
            bufs = [_guarded(nb, 1) if want else None for want in subset]
            view = L.vk_render_view(src.data_ptr(), 3 * w + RC.ROW_PAD, mask.data_ptr(), mstride, (C.c_uint64 * 3)(), (C.c_int64 * 3)(), h, w)
            for o, g in enumerate(bufs):
                if g is not None:
                    view.out[o], view.out_stride[o] = g[1].data_ptr(), ostride
            L.check(L.lib().vk_render_draw(1, C.byref(view), view_dev.data_ptr(), kind, c.thresh, C.byref(bl), L.ptr(prims), L.ptr(drawn), M if prims is not None else 0,
                                           flags, L.current_stream()), "vk_render_draw")
            torch.cuda.synchronize()
            got = []
            for o, g in enumerate(bufs):
                if g is None:
                    got.append(None)
                    continue
                assert _guards_ok(g[0], nb), "a guard byte was written"
                a = g[1].cpu().numpy().reshape(h, ostride)
                assert (a[:, 3 * w:] == GC.SENT).all(), "stride padding was written"
                a = a[:, :3 * w].reshape(h, w, 3)
                assert np.array_equal(a, ref[o]), (c.name, subset, flags, o, np.argwhere(a != ref[o])[:6])
                got.append(a)
            results.append(got)
        for o in range(3):
            assert (results[0][o] is None) == (results[1][o] is None) and (results[0][o] is None or np.array_equal(results[0][o], results[1][o]))


def test_draw_a_batch_of_maps_of_different_sizes(vk):
    """Three maps in one call: blockIdx.z picks the map, tiles beyond a smaller map's size do nothing."""
    L = vk._lib
    picks = [k for k, c in enumerate(_DCASES) if c.name in ("40x70_u8", "1x1_point", "40x70_refused_and_short")]
    M = max(len(_DCASES[k].prims) for k in picks)
    plist = np.zeros((len(picks), M), R.PRIM_DT)
    drawn = np.zeros(len(picks), np.int32)
    views = (L.vk_render_view * len(picks))()
    keep, outs = [], []
    for j, k in enumerate(picks):
        c = _DCASES[k]
        h, w = c.src.shape[:2]
        plist[j, :len(c.prims)] = c.prims
        drawn[j] = c.drawn
        src, mask = torch.from_numpy(c.src).to(_dev()), torch.from_numpy(c.mask).to(_dev())
        o = [torch.full((h, w, 3), GC.SENT, dtype=torch.uint8, device=_dev()) for _ in range(3)]
        keep += [src, mask]
        outs.append(o)
        views[j] = L.vk_render_view(src.data_ptr(), 3 * w, mask.data_ptr(), w, (C.c_uint64 * 3)(*(t.data_ptr() for t in o)), (C.c_int64 * 3)(3 * w, 3 * w, 3 * w), h, w)
    view_dev = torch.empty(11 * len(picks), dtype=torch.int64, device=_dev())
    # one blend for the call: the first case's colour
    c0 = _DCASES[picks[0]]
    bl = L.vk_render_blend((C.c_uint8 * 3)(*c0.color), 0, 1.0, c0.alpha, 0.0)
    L.check(L.lib().vk_render_draw(len(picks), views, view_dev.data_ptr(), L.VK_RENDER_MASK_U8, 0.5, C.byref(bl), _up(plist).data_ptr(), _up(drawn).data_ptr(),
                                   M, 0, L.current_stream()), "vk_render_draw")
    torch.cuda.synchronize()
    for j, k in enumerate(picks):
        c = _DCASES[k]
        ref = R.draw_ref(c.src, c.mask, 0.5, c0.color, 1.0, c0.alpha, prims=c.prims, drawn=c.drawn)
        for o in range(3):
            assert np.array_equal(outs[j][o].cpu().numpy(), ref[o]), (c.name, o)


def test_overlay_and_compose_canvas(vk):
    c = [d for d in _DCASES if d.name == "40x70_u8"][0]
    f = [d for d in _DCASES if d.name == "40x70_f32_reversed"][0]
    vo, vb, vv = R.draw_ref(c.src, c.mask, 0.5, (0, 140, 255), 1.0, 0.35)
    canvas = vk.render.compose_canvas(c.src, c.mask)
    assert canvas.shape == (40, 210, 3) and np.array_equal(canvas.cpu().numpy(), np.hstack([vo, vb, vv]))
    assert np.array_equal(vk.render.overlay(c.src, c.mask).cpu().numpy(), R.draw_ref(c.src, c.mask, 0.5, (0, 0, 255), 1.0, 0.35)[2])
    got = vk.render.overlay(torch.from_numpy(f.src).to(_dev()), f.mask, color=(10, 30, 50), alpha=0.5, thresh=f.thresh)
    assert np.array_equal(got.cpu().numpy(), R.draw_ref(f.src, f.mask, f.thresh, (10, 30, 50), 1.0, 0.5)[2])


# ------------------------------------------------------------------------------------------------ reduce
@pytest.mark.parametrize("k", RC.REDUCE_K)
def test_reduce_equals_the_restatement(vk, k):
    L = vk._lib
    for img in RC.reduce_images():
        h, w = img.shape[:2]
        oh, ow = -(-h // k), -(-w // k)
        ref = R.reduce_ref(img, k)
        _, src = _strided(img, RC.ROW_PAD)
        dstride = 3 * ow + 4
        buf, out = _guarded(oh * dstride, 1)
        L.check(L.lib().vk_render_reduce(h, w, k, src.data_ptr(), 3 * w + RC.ROW_PAD, out.data_ptr(), dstride, L.current_stream()), "vk_render_reduce")
        torch.cuda.synchronize()
        assert _guards_ok(buf, oh * dstride), "a guard byte was written"
        a = out.cpu().numpy().reshape(oh, dstride)
        assert (a[:, 3 * ow:] == GC.SENT).all() and np.array_equal(a[:, :3 * ow].reshape(oh, ow, 3), ref), (k, h, w)
        assert np.array_equal(vk.render.box_reduce(torch.from_numpy(img).to(_dev()), k).cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ the whole path
def _padded(recs_list, M):
    out = np.zeros((len(recs_list), M), recs_list[0].dtype)
    for b, r in enumerate(recs_list):
        out[b, :len(r)] = r
    return out


def test_detect_refine_draw_on_rendered_squares(vk):
    """Rendered squares -> letterbox -> stand-in -> vk.geometry.detect -> vk.subpix.refine -> draw_detections_on_three given the handle:
    the restatement drawing the .records() of the same handle, and the same call given the list of dicts."""
    dev = _dev()
    scenes = ZC.batch_scenes()
    imgs = [torch.from_numpy(sc.img).to(dev) for sc in scenes]
    x = torch.cat([vk.prepost.preprocess(im, ZC.LB, "centered", dev, pad_value=ZC.PAD)[0] for im in imgs])
    prob = torch.sigmoid(ZC.standin(x))[:, 0].contiguous()
    dets = vk.geometry.detect(prob, fit=ZC.FIT, max_components=4)
    aff = np.stack([vk.subpix.letterbox_affine(ZC.H, ZC.W, ZC.LB, "centered")] * len(scenes))
    fine = vk.subpix.refine(dets, prob, affine=aff)
    assert dets.counts.tolist() == [0, 1, 3]
    counts = dets.counts.cpu().numpy()
    recs = _padded(fine.records(counts), 4)
    lists = vk.zoom._lists(dets, fine, ZC.FIT)
    for b in (0, 2):
        img = scenes[b].img
        mask = (img[..., 0] < 120).astype(np.uint8) * 255
        pref, dref, _ = R.primitives_ref(recs[b:b + 1].view(SR.QUAD_DT), counts[b:b + 1], R.COORD_VS, "vs")
        ref = R.draw_ref(img, mask, 0.5, (0, 0, 255), 1.0, 0.35, prims=pref[0], drawn=int(dref[0]))
        got = vk.render.draw_detections_on_three(imgs[b], mask, None, fine, index=b)
        again = vk.render.draw_detections_on_three(img, torch.from_numpy(mask).to(dev), None, lists[b])
        for o in range(3):
            assert got[o].shape == (ZC.H, ZC.W, 3) and np.array_equal(got[o].cpu().numpy(), ref[o]), (b, o)
            assert torch.equal(got[o], again[o]), (b, o)
        assert int(dref[0]) == int(counts[b]) and ((ref[0] != img).any() == (counts[b] > 0))
    # the first pass's int32 boxes through the letterbox's affine row, and an overlay made beforehand
    b = 1
    img = scenes[b].img
    mask = (img[..., 0] < 120).astype(np.uint8) * 255
    drecs = _padded(dets.records(counts), 4)
    pref, dref, _ = R.primitives_ref(drecs[b:b + 1], counts[b:b + 1], R.COORD_BOX, "box", affine=aff[b:b + 1], thickness=3, text_scale=3)
    ref = R.draw_ref(img, mask, 0.5, (0, 0, 255), 1.0, 0.35, prims=pref[0], drawn=int(dref[0]))
    over = vk.render.overlay(imgs[b], mask)
    got = vk.render.draw_detections_on_three(imgs[b], mask, over, dets, index=b, affine=aff, thickness=3, text_scale=3)
    for o in range(3):
        assert np.array_equal(got[o].cpu().numpy(), ref[o]), o
    red = vk.render.draw_detections_on_three(imgs[b], mask, None, dets, index=b, affine=aff, thickness=3, text_scale=3, reduce=4)
    for o in range(3):
        assert red[o].shape == (ZC.H // 4, ZC.W // 4, 3) and torch.equal(red[o], vk.render.box_reduce(got[o], 4))


def test_segmenter_render(vk):
    """Segmenter.render on a 96 x 64 image with a module that is the stand-in: shapes, the reduce path, and vis_o away from every
    primitive's bounding box is the source image."""

    class StandIn(torch.nn.Module):
        def forward(self, x):
            return ZC.standin(x)

    img = ZC.render([(47.3, 31.6, 21.0, 0.35)], h=64, w=96)
    seg = vk.Segmenter(StandIn(), img_size=ZC.LB, device=_dev())
    kw = dict(fit=ZC.FIT, batch=2, max_components2=4, pad_value=ZC.PAD)
    rows, vis_o, vis_b, vis_v = seg.render(img, **kw)
    assert [v.shape for v in (vis_o, vis_b, vis_v)] == [(64, 96, 3)] * 3 and all(v.dtype == np.uint8 for v in (vis_o, vis_b, vis_v))
    areas = [d["area"] for d in rows]
    assert 1 <= len(rows) < 10 and areas == sorted(areas, reverse=True)
    recs = np.zeros((1, len(rows)), SR.QUAD_DT)
    for i, d in enumerate(rows):
        recs[0, i]["valid"], recs[0, i]["area"], recs[0, i]["vs"], recs[0, i]["d_mean"] = 1, len(rows) - i, d["box_subpix"].reshape(8), d["d_mean"]
    prims, drawn, _ = R.primitives_ref(recs, np.array([len(rows)]), R.COORD_VS, "vs")
    away = np.ones((64, 96), bool)
    for p in prims[0, :drawn[0]]:
        x0, y0, x1, y1 = (int(v) for v in p["bbox"])
        away[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = False
    assert np.array_equal(vis_o[away], img[away]) and (vis_o != img).any()
    assert set(np.unique(vis_b[away])) <= {0, 255} and (vis_b[away][:, 0] == vis_b[away][:, 2]).all()
    r2 = seg.render(img, reduce=2, **kw)
    assert [v.shape for v in r2[1:]] == [(32, 48, 3)] * 3
    for full, small in zip((vis_o, vis_b, vis_v), r2[1:]):
        assert np.array_equal(small, R.reduce_ref(full, 2))
    assert [d["d_mean"] for d in r2[0]] == [d["d_mean"] for d in rows] == [d["d_mean"] for d in seg.measure(img, **kw)]
