"""The restatement of vk.boundary (tests/boundary_ref.py) proved on its own, without a GPU: the separable transform against all pairs
and against scipy, phi against the scipy construction of the boundary loss, the statistics against hand values, the degenerate pairs and
the nearest-rank rule; then every argument error of the four entry points, which the library finds before it touches a stream."""
import ctypes as C

import numpy as np
import pytest

import boundary_cases as BC
import boundary_ref as R


def _all_maps():
    for h, w in BC.CPU_SHAPES:
        for name, m in BC.patterns(h, w):
            yield "%dx%d %s" % (h, w, name), m


# ------------------------------------------------------------------------------------------------ the transform
def test_separable_equals_brute_force():
    for name, m in _all_maps():
        for s in BC.SITES:
            got, want = R.edt_sq(m, s), R.edt_sq(m, s, brute=True)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, s)
            site = R.sites_of(m != 0, s)
            assert (got[site] == 0).all() and ((got == R.NONE).all() if not site.any() else (got[~site] > 0).all() and got.max() < R.INF), (name, s)


def test_edge_is_the_inner_boundary():
    a, _ = BC.squares_pair()
    e = R.edge_of(a != 0)
    assert e.sum() == 76 and e[10, 10:30].all() and e[29, 10:30].all() and e[10:30, 10].all() and not e[11:29, 11:29].any()
    assert not R.edge_of(np.ones((5, 7), bool)).any()                       # beyond the border counts as foreground
    b = np.zeros((6, 6), bool)
    b[0:3, 3:6] = True
    assert R.edge_of(b).sum() == 5 and not R.edge_of(b)[0, 4] and not R.edge_of(b)[0, 5] and not R.edge_of(b)[1, 5]
    assert R.edge_of(np.ones((1, 1), bool)).sum() == 0 and R.edge_of(np.zeros((1, 1), bool)).sum() == 0


def test_f32_maps_carry_the_threshold_itself():
    for name, m in _all_maps():
        f = BC.as_f32(m)
        assert f.dtype == np.float32 and np.array_equal(R.foreground(f, 0.5), m != 0), name
    f = BC.as_f32(BC.patterns(33, 65)[7][1])
    assert (f == np.float32(0.5)).any() and (f == np.nextafter(np.float32(0.5), np.float32(2))).any()


def test_separable_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in _all_maps():
        for s in BC.SITES:
            site = R.sites_of(m != 0, s)
            if not site.any():
                continue
            want = np.rint(ndi.distance_transform_edt(~site) ** 2).astype(np.int64)
            assert np.array_equal(R.edt_sq(m, s), want), (name, s)


def test_phi_is_the_scipy_construction():
    """Kervadec et al.'s one_hot2dist: negmask = ~posmask; res = distance(negmask) * negmask - (distance(posmask) - 1) * posmask, and
    zeros for an empty mask.  (Their code leaves a FULL mask to scipy, which has no background to measure from; here it is 0.)"""
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in _all_maps():
        pos = m != 0
        got = R.phi(m)
        assert got.dtype == np.float32 and got.shape == m.shape
        if not pos.any() or pos.all():
            assert (got == 0).all(), name
            continue
        neg = ~pos
        want = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos
        assert np.allclose(got, want, rtol=0, atol=1e-4), name
        assert (got[pos] <= 0).all() and (got[neg] >= 1).all() and (got[R.edge_of(pos)] == 0).all(), name


def test_phi_without_scipy_properties():
    a, _ = BC.squares_pair()
    f = R.phi(a)
    assert f[0, 0] == np.float32(np.sqrt(200.0)) and f[10, 10] == 0 and f[20, 20] == np.float32(1.0 - 10.0) and f[9, 15] == 1
    assert R.phi_from_d2(np.array([R.NONE, 0, 0, 9]), np.array([0, R.NONE, 4, 0])).tolist() == [0.0, 0.0, -1.0, 3.0]


# ------------------------------------------------------------------------------------------------ the statistics
def test_hand_values_of_the_two_squares():
    a, b = BC.squares_pair()
    r = R.stats(a, b, tol2=BC.TOL2, band2=BC.BAND2)
    assert r["n_pred"] == r["n_gt"] == 76 and r["area_pred"] == r["area_gt"] == 400
    assert r["max2_pg"] == r["max2_gp"] == 25 and r["q95_2_pg"] == 17 and r["flags"] == 0
    m = R.metrics(r, 3)
    assert abs(m["assd"] - 3.2316540947811) < 1e-12 and m["hd"] == 5.0 and m["hd95"] == np.sqrt(17.0)
    assert r["within_pg"][3:] == [0] * 5 and r["within_pg"][0] <= r["within_pg"][1] <= r["within_pg"][2] <= 76
    # the band of a 20 x 20 square at band2 = 4: the two outer rings, 400 - 16 * 16
    assert R.stats(a, a, tol2=BC.TOL2, band2=4)["band_union"] == 400 - 256
    assert R.metrics(r, 3, scale=2.5)["hd"] == 12.5 and R.metrics(r, 3, scale=2.5)["nsd"] == m["nsd"]


def test_degenerate_pairs():
    cases = {name: (p, g) for name, p, g in BC.pair_cases()}
    r = R.stats(*cases["identical"])
    m = R.metrics(r, 3)
    assert r["max2_pg"] == r["max2_gp"] == r["q95_2_pg"] == 0 and r["sum_pg"] == 0.0 and m["nsd"] == [1.0] * 3 and m["boundary_iou"] == 1.0
    for name, flag in (("pred empty", 1), ("gt empty", 2)):
        r = R.stats(*cases[name])
        m = R.metrics(r, 3)
        assert r["flags"] == flag and r["max2_pg"] == r["q95_2_gp"] == -1 and r["sum_pg"] == r["sum_gp"] == 0.0 and r["within_gp"] == [0] * 8
        assert m["hd"] == m["hd95"] == m["assd"] == float("inf") and m["nsd"] == [0.0] * 3 and m["boundary_iou"] == 0.0
    r = R.stats(*cases["both empty"])
    m = R.metrics(r, 3)
    assert r["flags"] == 3 and r["n_pred"] == r["n_gt"] == 0 and m["hd"] == m["hd95"] == m["assd"] == 0.0 and m["nsd"] == [1.0] * 3
    assert m["boundary_iou"] == 1.0
    r = R.stats(*cases["one pixel"])                 # (20, 31) against the square rows 14..33, columns 13..32: one column inside its right side
    assert r["n_pred"] == 1 and r["area_pred"] == 1 and r["max2_pg"] == r["q95_2_pg"] == 1 and r["sum_pg"] == 1.0 and r["within_pg"][:3] == [1, 1, 1]
    assert r["max2_gp"] == (31 - 13) ** 2 + (33 - 20) ** 2
    r = R.stats(*cases["border"])                    # 12 x 18 in the corner: the bottom row and the left column only
    assert r["n_pred"] == 18 + 12 - 1 and r["area_pred"] == 12 * 18
    r = R.stats(*cases["full vs square"])            # a full mask has no boundary although it is not empty
    assert r["flags"] == 0 and r["n_pred"] == 0 and r["max2_gp"] == -1 and R.metrics(r, 3)["hd"] == float("inf")
    assert r["band_inter"] == 0 and r["band_union"] == 400 - 256
    r = R.stats(*cases["full vs full"])
    assert r["n_pred"] == r["n_gt"] == 0 and R.metrics(r, 3)["hd"] == 0.0 and R.metrics(r, 3)["boundary_iou"] == 1.0


def test_nearest_rank():
    assert [R.nearest_rank(n) for n in (1, 19, 20, 21, 100)] == [1, 19, 19, 20, 95]
    for n in (1, 19, 20, 21, 100):
        k = R.nearest_rank(n)
        assert 1 <= k <= n and 100 * k >= 95 * n > 100 * (k - 1)            # the smallest rank that covers 95 %
    # n values 0, 1, 4, ..., (n - 1)^2 on a line: the record picks element k - 1, not numpy's interpolation
    for n in (19, 20, 21, 100):
        pred = np.zeros((3, 2 * n + 2), np.uint8)
        gt = np.zeros_like(pred)
        gt[1, 0] = 1
        pred[1, 0:2 * n:2] = 1                      # n isolated pixels at distance 0, 2, 4, ... from the one gt pixel
        r = R.stats(pred, gt)
        assert r["n_pred"] == n and r["q95_2_pg"] == (2 * (R.nearest_rank(n) - 1)) ** 2 and r["max2_pg"] == (2 * (n - 1)) ** 2


def test_loss_reference():
    a, _ = BC.squares_pair()
    f = R.phi(a)
    v, g = R.loss(np.zeros(f.shape), f)
    assert v == 0.5 * f.astype(np.float64).sum() / f.size and np.array_equal(g, f.astype(np.float64) / 4 / f.size)
    x = np.random.default_rng(0).normal(size=f.shape) * 3
    v0, g0 = R.loss(x, f)
    i = (7, 9)
    e = np.zeros(f.shape)
    e[i] = 1e-6
    assert abs((R.loss(x + e, f)[0] - R.loss(x - e, f)[0]) / 2e-6 - g0[i]) < 1e-9
    assert np.allclose(R.loss(x, f, 3.0)[1], 3.0 * f.astype(np.float64) * R.sigmoid64(x) * (1 - R.sigmoid64(x)) / f.size, rtol=1e-12, atol=0)
    assert R.loss(np.full(f.shape, 40.0), f)[1][0, 0] == f[0, 0] * (1.0 / (1.0 + np.exp(-40.0))) * (np.exp(-40.0) / (1.0 + np.exp(-40.0))) / f.size > 0


# ------------------------------------------------------------------------------------------------ argument errors
def test_library_exports_and_python_exports(vk):
    Lb = vk.lib()
    for name in ("vk_edt_sq", "vk_edt_workspace_bytes", "vk_boundary_phi", "vk_boundary_stats", "vk_boundary_stats_workspace_bytes",
                 "vk_boundary_loss"):
        assert hasattr(Lb, name) and name in vk._lib.SIGNATURES
    for name in ("boundary", "BoundaryLoss", "BoundaryMetrics"):
        assert name in vk.__all__ and hasattr(vk, name)
    assert C.sizeof(vk._lib.vk_boundary_rec) == 216 == vk.boundary.RECORD_DTYPE.itemsize
    for f, _ in vk._lib.vk_boundary_rec._fields_:
        assert getattr(vk._lib.vk_boundary_rec, f).offset == vk.boundary.RECORD_DTYPE.fields[f][1], f
    assert vk.boundary.NONE == R.NONE and vk.boundary.MAX_SIDE == R.MAX_SIDE
    assert Lb.vk_edt_workspace_bytes(3, 7, 5) == 3 * 7 * 5 * 4 and Lb.vk_edt_workspace_bytes(1, 4097, 1) == 0 and Lb.vk_edt_workspace_bytes(0, 1, 1) == 0
    assert Lb.vk_boundary_stats_workspace_bytes(2, 7, 5) >= 5 * 2 * 7 * 5 * 4 and Lb.vk_boundary_stats_workspace_bytes(1, 0, 1) == 0
    assert [vk.boundary.radius_sq(t) for t in (0, 1, 1.5, 2, 2.9, 3)] == [0, 1, 2, 4, 8, 9]


def _bufs():
    return dict(src=np.full(256, 7, np.float32), gt=np.full(256, 7, np.float32), d2=np.full(256, 7, np.int32), d2b=np.full(256, 7, np.int32),
                phi=np.full(256, 7, np.float32), ws=np.full(65536, 7, np.int64), out=np.full(64, 7, np.int64), logits=np.full(256, 7, np.float32),
                grad=np.full(256, 7, np.float32), loss=np.full(4, 7, np.float32))


def _untouched(b):
    return all((v == 7).all() for v in b.values())


def _ptrs(b, names, null, off):
    return {k: (None if null == k else b[k].ctypes.data + (off[1] if off and off[0] == k else 0)) for k in names}


def _run(vk, who, call, cases):
    Lb = vk.lib()
    for kw, word in cases:
        b = _bufs()
        rc = call(b, **kw)
        err = Lb.vk_last_error_string().decode()
        assert rc == -1 and word in err and who in err, (who, kw, rc, err)
        assert _untouched(b), (who, kw)


def test_edt_refuses_bad_arguments(vk):
    Lb = vk.lib()

    def call(b, batch=1, h=4, w=4, kind=1, thresh=0.5, sites=0, ws_bytes=64, null=None, off=None):
        p = _ptrs(b, ("src", "d2", "ws"), null, off)
        return Lb.vk_edt_sq(batch, h, w, p["src"], kind, thresh, sites, p["d2"], p["ws"], ws_bytes, None)

    _run(vk, "vk_edt_sq", call, [
        (dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=0), "map size"), (dict(h=4097), "map size"),
        (dict(w=4097), "map size"), (dict(kind=2), "kind 2"), (dict(kind=-1), "kind -1"), (dict(thresh=float("nan")), "NaN"),
        (dict(sites=3), "sites 3"), (dict(sites=-1), "sites -1"), (dict(sites=0x103), "sites"), (dict(sites=0x203), "sites"), (dict(sites=0x300), "sites"), (dict(sites=0x400), "sites"),
        (dict(null="src"), "null buffer"), (dict(null="d2"), "null buffer"), (dict(null="ws"), "null buffer"),
        (dict(off=("src", 2)), "misaligned"), (dict(off=("d2", 1)), "misaligned"), (dict(off=("ws", 2)), "misaligned"),
        (dict(ws_bytes=63), "workspace"), (dict(ws_bytes=0), "workspace")])


def test_phi_refuses_bad_arguments(vk):
    Lb = vk.lib()

    def call(b, batch=1, h=4, w=4, null=None, off=None):
        p = _ptrs(b, ("d2", "d2b", "phi"), null, off)
        return Lb.vk_boundary_phi(batch, h, w, p["d2"], p["d2b"], p["phi"], None)

    _run(vk, "vk_boundary_phi", call, [
        (dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=4097), "map size"),
        (dict(null="d2"), "null buffer"), (dict(null="d2b"), "null buffer"), (dict(null="phi"), "null buffer"),
        (dict(off=("d2", 2)), "misaligned"), (dict(off=("d2b", 1)), "misaligned"), (dict(off=("phi", 3)), "misaligned")])


def test_stats_refuses_bad_arguments(vk):
    Lb = vk.lib()
    need = Lb.vk_boundary_stats_workspace_bytes(1, 4, 4)
    assert 0 < need <= 65536 * 8

    def call(b, batch=1, h=4, w=4, pk=1, pt=0.5, gk=1, gt=0.5, n_tol=3, tol=(1, 4, 9), band2=4, ws_bytes=need, null=None, off=None, tol_null=False):
        p = _ptrs(b, ("src", "gt", "out", "ws"), null, off)
        t = None if tol_null else (C.c_int32 * 8)(*tol)
        return Lb.vk_boundary_stats(batch, h, w, p["src"], pk, pt, p["gt"], gk, gt, n_tol, t, band2, p["out"], p["ws"], ws_bytes, None)

    _run(vk, "vk_boundary_stats", call, [
        (dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=4097), "map size"), (dict(pk=2), "pred kind 2"),
        (dict(gk=7), "gt kind 7"), (dict(pt=float("nan")), "pred threshold"), (dict(gt=float("nan")), "gt threshold"),
        (dict(n_tol=-1), "tolerances"), (dict(n_tol=9), "tolerances"), (dict(tol_null=True), "tol2"), (dict(tol=(1, -4, 9)), "tol2[1]"),
        (dict(band2=-1), "band2"), (dict(null="src"), "null buffer"), (dict(null="gt"), "null buffer"), (dict(null="out"), "null buffer"),
        (dict(null="ws"), "null buffer"), (dict(off=("src", 2)), "misaligned"), (dict(off=("gt", 1)), "misaligned"),
        (dict(off=("out", 4)), "misaligned"), (dict(off=("ws", 4)), "misaligned"), (dict(ws_bytes=need - 1), "workspace")])


def test_loss_refuses_bad_arguments(vk):
    Lb = vk.lib()
    W = vk._lib.VK_BOUNDARY_LOSS_WS_BYTES
    assert W == 32768

    def call(b, n=1, c=1, hw=16, ws_bytes=W, null=None, off=None):
        p = _ptrs(b, ("logits", "phi", "grad", "loss", "ws"), null, off)
        return Lb.vk_boundary_loss(n, c, hw, p["logits"], p["phi"], 1.0, p["grad"], p["loss"], p["ws"], ws_bytes, None)

    _run(vk, "vk_boundary_loss", call, [
        (dict(n=0), "batch"), (dict(c=0), "classes"), (dict(c=17), "classes"), (dict(hw=0), "plane"), (dict(null="logits"), "null buffer"),
        (dict(null="phi"), "null buffer"), (dict(null="loss"), "null buffer"), (dict(null="ws"), "null buffer"),
        (dict(off=("logits", 2)), "misaligned"), (dict(off=("phi", 1)), "misaligned"), (dict(off=("grad", 2)), "misaligned"),
        (dict(off=("loss", 2)), "misaligned"), (dict(off=("ws", 4)), "misaligned"), (dict(ws_bytes=W - 1), "workspace")])


def test_python_entry_points_refuse_wrong_arguments(vk):
    import torch
    B = vk.boundary
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sites"):
        B.edt_sq(m, sites="outline")
    with pytest.raises(ValueError, match="rows"):
        B.edt_sq(m, rows="fast")
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        B.edt_sq(m)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        B.signed_distance(m)
    with pytest.raises(ValueError, match="differ in shape"):
        B.surface_stats(m, torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at most 8"):
        B.surface_stats(m, m, tolerances=range(9))
    with pytest.raises(ValueError, match="radius"):
        B.surface_stats(m, m, tolerances=(-1,))
    with pytest.raises(ValueError, match="radius"):
        vk.BoundaryMetrics(band=float("nan"))
    with pytest.raises(ValueError, match="before any update"):
        vk.BoundaryMetrics().compute()
    loss = vk.BoundaryLoss()
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError, match="either target or dist"):
        loss(x)
    with pytest.raises(ValueError, match="either target or dist"):
        loss(x, x, x)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        loss(x, x)
    with pytest.raises(ValueError, match="N, C, H, W"):
        loss(torch.zeros(4, 4), x)
    assert not hasattr(loss, "_as_sum") and not isinstance(loss, vk.seglosses._Algebra)       # no member of the LossSum algebra


def test_metrics_from_records_follow_the_restatement(vk):
    B = vk.boundary
    cases = BC.pair_cases()
    recs = np.zeros(len(cases), B.RECORD_DTYPE)
    for i, (_, p, g) in enumerate(cases):
        r = R.stats(p, g, tol2=BC.TOL2, band2=BC.BAND2)
        for k, v in r.items():
            recs[i][k] = v
    scale = np.linspace(1.0, 3.0, len(cases))
    out = B.metrics_from_records(recs, BC.TOLERANCES, scale)
    for i, (name, p, g) in enumerate(cases):
        want = R.metrics(R.stats(p, g, tol2=BC.TOL2, band2=BC.BAND2), 3, scale[i])
        for key in ("hd", "hd95", "assd", "boundary_iou"):
            assert out[key][i] == want[key] or abs(out[key][i] - want[key]) <= 1e-12 * abs(want[key]), (name, key)
        assert [out["nsd"][t][i] for t in BC.TOLERANCES] == want["nsd"], name
    assert out["n_images"] == len(cases) and out["mean"]["hd"] == float("inf")
    assert out["mean"]["boundary_iou"] == float(np.mean(out["boundary_iou"]))
