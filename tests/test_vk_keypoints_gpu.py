"""vk.keypoints on the device against the restatement of tests/keypoints_ref.py: equality of bytes.

Every output lies in a sentinel-filled buffer between two guard zones; what a call must not touch (guards, slots above the count,
plane 0 beside plane 1, its inputs) is compared afterwards.  The cases are built by hand (tests/keypoints_cases.py); the last tests
take the whole path detect_gt -> targets -> refine -> match through the Python interface."""
import ctypes as C

import numpy as np
import pytest
import torch

import geom_cases as GC
import keypoints_cases as KC
import keypoints_ref as R
import subpix_cases as SC

pytestmark = pytest.mark.gpu

GUARD = 512                   # bytes
SENT_F = np.frombuffer(bytes([GC.SENT] * 4), np.float32)[0]


def _dev():
    return torch.device("cuda:0")


def _guarded(nbytes, align=16, shift=0):
    """A sentinel-filled uint8 buffer, and the offset of an `align`-aligned (+ shift) zone of nbytes between two guards."""
    buf = torch.full((nbytes + 2 * GUARD + 64,), GC.SENT, dtype=torch.uint8, device=_dev())
    off = GUARD + (-(buf.data_ptr() + GUARD)) % align + shift
    return buf, off


def _guards_intact(buf, off, nbytes):
    return bool((buf[:off] == GC.SENT).all().item()) and bool((buf[off + nbytes:] == GC.SENT).all().item())


def _upload(recs):
    raw = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy())
    pad = torch.zeros((raw.numel() + 7) // 8 + 1, dtype=torch.int64, device=_dev()).view(torch.uint8)       # 8-byte aligned
    pad[:raw.numel()] = raw.to(_dev())
    return pad[:raw.numel()]


# ------------------------------------------------------------------------------------------------ vk_kp_targets
_LAYOUTS = ("dense", "plane1", "odd_stride", "misaligned")


def _run_targets(vk, case, layout, flags=0):
    """-> (float32 [B][h][w] read back, the bytes between the maps that must still be the sentinel)."""
    L = vk._lib
    B, M = case.recs.shape
    h, w = case.h, case.w
    stride = {"dense": h * w, "plane1": 2 * h * w, "odd_stride": h * w + 3, "misaligned": h * w}[layout]
    first = h * w if layout == "plane1" else 0                # plane 1 begins one plane into the tensor
    n_el = first + (B - 1) * stride + h * w
    buf, off = _guarded(4 * n_el, 16, 4 if layout == "misaligned" else 0)
    raw, counts = _upload(case.recs), torch.from_numpy(case.counts.astype(np.int32)).to(_dev())
    tab = torch.from_numpy(KC.table(case.r16)).to(_dev())
    before = (raw.clone(), counts.clone(), tab.clone())
    dt = case.recs.dtype
    L.check(L.lib().vk_kp_targets(B, h, w, raw.data_ptr(), dt.itemsize, dt.fields[case.field][1], case.vert_type,
                                  dt.fields["valid"][1] if "valid" in dt.names else -1, counts.data_ptr(), M, tab.data_ptr(), tab.numel(),
                                  buf.data_ptr() + off + 4 * first, stride, flags, L.current_stream()), "vk_kp_targets")
    torch.cuda.synchronize()
    assert _guards_intact(buf, off, 4 * n_el), (case.name, layout, "a guard byte was written")
    assert torch.equal(before[0], raw) and torch.equal(before[1], counts) and before[2].view(torch.int32).equal(tab.view(torch.int32))
    host = buf[off:off + 4 * n_el].cpu().numpy().view(np.float32)
    maps = np.stack([host[first + b * stride:first + b * stride + h * w].reshape(h, w) for b in range(B)])
    keep = np.ones(n_el, bool)
    for b in range(B):
        keep[first + b * stride:first + b * stride + h * w] = False
    return maps, host[keep]


_TCASES = KC.target_cases()


@pytest.fixture(scope="module")
def target_refs():
    return {c.name: c.expected() for c in _TCASES}


@pytest.mark.parametrize("case", _TCASES, ids=[c.name for c in _TCASES])
def test_targets_on_built_records(vk, case, target_refs):
    ref = target_refs[case.name]
    for layout in _LAYOUTS:
        got, between = _run_targets(vk, case, layout)
        assert got.tobytes() == ref.tobytes(), (case.name, layout, np.argwhere(got.view(np.int32) != ref.view(np.int32))[:4])
        assert (between.view(np.int32) == SENT_F.view(np.int32)).all(), (case.name, layout, "plane 0 or the gap between two maps was written")
    if KC.table(case.r16).size <= vk._lib.VK_KP_TABLE_LDS_MAX:
        for flags in (vk._lib.VK_KP_TABLE_MEMORY, vk._lib.VK_KP_TABLE_LDS):
            for layout in ("dense", "odd_stride"):
                assert _run_targets(vk, case, layout, flags)[0].tobytes() == ref.tobytes(), (case.name, layout, flags)


def test_targets_both_store_paths_run(vk):
    """The layouts above take both store paths on one case: width 64 dense is the 16-byte path, the odd stride and the misaligned base
    the scalar path; an odd width is scalar in every layout."""
    names = {c.name: c for c in _TCASES}
    assert names["64x16_corners"].w % 4 == 0 and names["80x72_r96"].w % 4 == 0 and names["1x7"].w % 4 != 0


# ------------------------------------------------------------------------------------------------ vk_kp_peaks
def _run_peaks(vk, case, strided=False):
    L = vk._lib
    lib = L.lib()
    B, h, w = case.heat.shape
    stride = h * w + (5 if strided else 0)
    heat = torch.full((B * stride + 8,), float("nan"), dtype=torch.float32, device=_dev())
    for b in range(B):
        heat[b * stride:b * stride + h * w] = torch.from_numpy(case.heat[b].reshape(-1)).to(_dev())
    before = heat.clone()
    nb = B * case.max_peaks * 16
    buf, off = _guarded(nb, 4)
    cbuf, coff = _guarded(4 * B, 4)
    need = lib.vk_kp_peaks_workspace_bytes(B, h, w)
    assert need == B * ((h * w + 1023) // 1024) * 260
    ws = torch.full((need // 4 + 1,), -1515870811, dtype=torch.int32, device=_dev())        # 0xA5A5A5A5: not cleared
    L.check(lib.vk_kp_peaks(B, h, w, heat.data_ptr(), stride, case.min_peak, case.r, case.max_peaks, buf.data_ptr() + off,
                            cbuf.data_ptr() + coff, ws.data_ptr(), need, L.current_stream()), "vk_kp_peaks")
    torch.cuda.synchronize()
    assert _guards_intact(buf, off, nb) and _guards_intact(cbuf, coff, 4 * B), (case.name, "a guard byte was written")
    assert before.view(torch.int32).equal(heat.view(torch.int32))
    return (buf[off:off + nb].cpu().numpy().view(R.PEAK_DT).reshape(B, case.max_peaks), cbuf[coff:coff + 4 * B].cpu().numpy().view(np.int32))


_PCASES = KC.peak_cases()


@pytest.mark.parametrize("case", _PCASES, ids=[c.name for c in _PCASES])
def test_peaks_on_built_maps(vk, case):
    B = case.heat.shape[0]
    sent = np.full((B, case.max_peaks, 16), GC.SENT, np.uint8).reshape(-1).view(R.PEAK_DT).reshape(B, case.max_peaks)
    ref, ref_counts = R.peaks_ref(case.heat, case.min_peak, case.r, case.max_peaks, out=sent)        # untouched slots keep the sentinel
    for strided in (False, True):
        got, counts = _run_peaks(vk, case, strided)
        assert counts.tolist() == ref_counts.tolist(), (case.name, strided)
        assert got.tobytes() == ref.tobytes(), (case.name, strided)


def test_peaks_python_interface(vk):
    case = {c.name: c for c in _PCASES}["batch3"]
    two = torch.full((3, 2, 40, 70), float("nan"), device=_dev())
    two[:, 1] = torch.from_numpy(case.heat).to(_dev())
    pk = vk.keypoints.peaks(two[:, 1], min_peak=case.min_peak, nms_radius=case.r, max_peaks=case.max_peaks)       # plane 1 read in place
    ref, counts = R.peaks_ref(case.heat, case.min_peak, case.r, case.max_peaks)
    assert pk.counts.cpu().tolist() == counts.tolist()
    for b, recs in enumerate(pk.records()):
        assert recs.tobytes() == ref[b, :min(counts[b], case.max_peaks)].tobytes()
    gt = np.stack([ref[0]["x"][:4], ref[0]["y"][:4]], axis=1)
    assert vk.keypoints.vertex_metrics(pk.records()[0][:4], gt, 0.5)["tp"] == 4


# ------------------------------------------------------------------------------------------------ vk_kp_refine
def _kp_params(vk, p):
    return vk.keypoints.params("parabola" if p["method"] == R.PARABOLA else "centroid", p["search"], p["cwin"], p["min_peak"], p["floor_frac"])


def _run_refine(vk, case, strided=False):
    L = vk._lib
    B, M = case.recs.shape
    h, w = case.heat.shape[1:]
    stride = h * w + (7 if strided else 0)
    heat = torch.full((B * stride + 8,), 3.0, dtype=torch.float32, device=_dev())
    for b in range(B):
        heat[b * stride:b * stride + h * w] = torch.from_numpy(case.heat[b].reshape(-1)).to(_dev())
    raw, counts = _upload(case.recs), torch.from_numpy(case.counts.astype(np.int32)).to(_dev())
    aff = None if case.affine is None else torch.from_numpy(np.ascontiguousarray(case.affine, np.float64)).to(_dev())
    nb = B * M * R.QUAD_DT.itemsize
    buf, off = _guarded(nb, 8)
    before = (heat.clone(), raw.clone(), counts.clone())
    dt = case.recs.dtype
    p = _kp_params(vk, case.params)
    L.check(L.lib().vk_kp_refine(C.byref(p), B, h, w, heat.data_ptr(), stride, raw.data_ptr(), dt.itemsize, dt.fields["box"][1],
                                 dt.fields["valid"][1] if "valid" in dt.names else -1, counts.data_ptr(), M, L.ptr(aff), buf.data_ptr() + off,
                                 L.current_stream()), "vk_kp_refine")
    torch.cuda.synchronize()
    assert _guards_intact(buf, off, nb), (case.name, "a guard byte was written")
    assert before[0].view(torch.int32).equal(heat.view(torch.int32)) and torch.equal(before[1], raw) and torch.equal(before[2], counts)
    return buf[off:off + nb].cpu().numpy().view(R.QUAD_DT).reshape(B, M)


def _assert_records(got, ref, tag):
    if got.tobytes() == ref.tobytes():
        return
    for idx in np.ndindex(got.shape):
        for f in R.QUAD_DT.names:
            assert got[idx][f].tobytes() == ref[idx][f].tobytes(), (tag, idx, f, got[idx][f], ref[idx][f])
    raise AssertionError((tag, "bytes differ outside the fields"))


_RCASES = KC.refine_cases()


@pytest.mark.parametrize("case", _RCASES, ids=[c.name for c in _RCASES])
def test_refine_on_built_records(vk, case):
    sent = np.full(case.recs.shape + (R.QUAD_DT.itemsize,), GC.SENT, np.uint8).reshape(-1).view(R.QUAD_DT).reshape(case.recs.shape)
    ref = R.refine_ref(case.heat, case.recs, case.counts, case.params, case.affine, out=sent)
    got = _run_refine(vk, case)
    _assert_records(got, ref, case.name)
    _assert_records(_run_refine(vk, case, strided=True), ref, (case.name, "strided"))
    assert _run_refine(vk, case).tobytes() == got.tobytes(), (case.name, "second run")


# ------------------------------------------------------------------------------------------------ the whole path on the device
def _squares_mask():
    m = np.zeros((2, 96, 160), np.float32)
    for b, (cx, cy, rad, ang) in enumerate(((50.0, 48.0, 30.0, 0.2), (100.0, 50.0, 34.0, 0.7))):
        m[b] = SC.polygon_coverage(96, 160, SC.square_vertices(cx, cy, rad, ang)) >= 0.5
    m[0] = np.maximum(m[0], SC.polygon_coverage(96, 160, SC.square_vertices(125.0, 40.0, 18.0, 0.4)) >= 0.5)
    return m


def _whole_path(vk, mask_np):
    """detect_gt -> targets -> refine -> match on the device; the restated chain on the records read back."""
    K, I = vk.keypoints, vk.instances
    mask = torch.from_numpy(mask_np).to(_dev())
    dets = I.detect_gt(mask, fit="quad", fit_outset_px=0, max_components=8)
    heat = K.targets(dets)
    B, h, w = mask_np.shape
    host = dets.raw.cpu().numpy().reshape(-1).view(dets.record_dtype).reshape(B, 8)
    counts = dets.counts.cpu().numpy()
    ref_heat = R.targets_ref(host, counts, h, w, R.gaussian_table(2.0))
    assert heat.cpu().numpy().tobytes() == ref_heat.tobytes()
    n_valid = 0
    for method, code in (("parabola", R.PARABOLA), ("centroid", R.CENTROID)):
        fine = K.refine(dets, heat, method=method)
        got = fine.raw.cpu().numpy().reshape(-1).view(R.QUAD_DT).reshape(B, 8)
        ref = R.refine_ref(ref_heat, host, counts, R.kp_params(code), out=np.zeros((B, 8), R.QUAD_DT))
        _assert_records(got, ref, method)
        for b in range(B):
            for s in range(min(int(counts[b]), 8)):
                if host[b, s]["valid"] and not got[b, s]["flags"].any():
                    n_valid += 1
                    assert (got[b, s]["v"] == host[b, s]["box"]).all()                  # v == box
                    assert got[b, s]["d_mean"] == host[b, s]["d_mean"]
        res = I.match(fine, fine).cpu()
        n = int(sum(min(int(c), 8) for c in counts))
        assert int(res.totals["tp"][0]) == n and int(res.totals["fp"][0]) == 0 and int(res.totals["fn"][0]) == 0
        assert float(res.totals["sum_abs_d"][0]) == 0.0
    return n_valid


def test_whole_path_on_built_squares(vk):
    assert _whole_path(vk, _squares_mask()) >= 4


def test_whole_path_on_a_micrograph_scene(vk):
    ds = vk.MicrographDataset(4, size=80, seed=3, device=_dev())
    mask = ds.masks([1, 3]).float().cpu().numpy()              # three indentations, their vertices further apart than the search window
    assert mask.any()
    assert _whole_path(vk, mask) >= 4


def test_with_targets_and_make_targets(vk):
    K = vk.keypoints
    ds = vk.MicrographDataset(4, size=80, seed=3, device=_dev())
    batches = list(K.with_targets(ds.loader(2, shuffle=False), sigma=1.5))
    plain = list(ds.loader(2, shuffle=False))
    assert len(batches) == len(plain) == 2
    for (x2, y2, n2), (x, y, n) in zip(batches, plain):
        assert n2 == n and torch.equal(x2, x) and tuple(y2.shape) == (2, 2, 80, 80) and y2.dtype == torch.float32
        mine = K.make_targets(y, sigma=1.5)
        assert torch.equal(y2, mine) and torch.equal(y2[:, 0], y[:, 0])
        dets = vk.instances.detect_gt(y[:, 0], fit="quad", fit_outset_px=0)
        assert torch.equal(y2[:, 1], K.targets(dets, sigma=1.5))
        again = K.make_targets(y, sigma=1.5)
        assert again.cpu().numpy().tobytes() == mine.cpu().numpy().tobytes()          # two runs, the same bytes
        assert float(y2[:, 1].max()) <= 1.0 and float(y2[:, 1].min()) >= 0.0
    # through vk.subpix on the mask first: float64 vertices
    y = plain[0][1]
    fine = K.make_targets(y, refine=dict(method="lines"))
    dets = vk.subpix.refine(vk.instances.detect_gt(y[:, 0], fit="quad", fit_outset_px=0), y[:, 0].contiguous(), method="lines")
    host = dets.raw.cpu().numpy().reshape(-1).view(R.QUAD_DT).reshape(2, 64)
    ref = R.targets_ref(host, dets.counts.cpu().numpy(), 80, 80, R.gaussian_table(2.0), "v", R.VERT_F64)
    assert fine[:, 1].cpu().numpy().tobytes() == ref.tobytes()


def test_postprocess_lists(vk):
    K = vk.keypoints
    mask = torch.from_numpy(_squares_mask()).to(_dev())
    dets = vk.instances.detect_gt(mask, fit="quad", fit_outset_px=0)
    probs2 = torch.stack([mask, K.targets(dets)], dim=1)
    clean, lists = K.postprocess(probs2, fit="quad", bin_thresh=0.5, min_area=1, morph_kernel=1, fit_outset_px=0)
    assert len(lists) == 2 and [len(r) for r in lists] == [2, 1] and clean.shape == mask.shape
    for rows in lists:
        for d in rows:
            assert d["box_subpix"].shape == (4, 2) and d["subpix_flags"].shape == (4,) and not d["subpix_flags"].any()
            assert (d["box_subpix_map"] == d["box"]).all() and d["d_mean"] > 0
