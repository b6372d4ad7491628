"""Host side of vk.subpix (no GPU): the restatement (tests/subpix_ref.py) against analytic truth, which is what makes the feature
worth having, its pieces against brute force and numpy.linalg, its behaviour on the reference's own label masks, and the argument
checks of vk_subpix_refine through the loaded library and of the Python entry points.

Measured when this file was written (32 draws per sigma, start vertices rint(truth + U(-1.5, 1.5)), error of d_mean in pixels):
  sigma 0: start worst 2.26, corner worst 0.42 (mean -0.20), lines worst 0.15 (mean -0.01)
  sigma 1: start worst 2.19, corner worst 0.52 (mean -0.45), lines worst 0.05 (mean +0.01)"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import geom_cases as GC
import instances_cases as IC
import subpix_cases as SC
import subpix_ref as R
from conftest import GOLDEN

CORNER_BOUND, LINES_BOUND = 0.8, 0.4          # pixels, on every draw


# ------------------------------------------------------------------------------------------------ against analytic truth
@pytest.fixture(scope="module")
def errors():
    out = {}
    for sigma in (0.0, 1.0):
        draws = SC.square_draws(sigma)
        assert len(draws) >= 30
        for name, p in (("corner", R.corner_params(win=5, zero_zone=-1)), ("lines", R.lines_params())):
            res = [R.refine_one(d.prob, [int(c) for c in d.box], p) for d in draws]
            out[(name, sigma)] = (np.array([r[6] - d.d_true for r, d in zip(res, draws)]), [r[2] for r in res])
        out[("start", sigma)] = (np.array([d.d_start - d.d_true for d in draws]), None)
    return out


@pytest.mark.parametrize("sigma", [0.0, 1.0])
@pytest.mark.parametrize("name,bound", [("corner", CORNER_BOUND), ("lines", LINES_BOUND)])
def test_diagonal_against_truth(errors, name, bound, sigma):
    err, flags = errors[(name, sigma)]
    print(name, sigma, "worst |error| %.3f px, mean %+.3f px" % (np.abs(err).max(), err.mean()))
    assert all(f == [0, 0, 0, 0] for f in flags)
    assert (np.abs(err) <= bound).all(), (name, sigma, np.abs(err).max())


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_the_start_vertices_are_worse_than_a_pixel(errors, sigma):
    start = np.abs(errors[("start", sigma)][0])
    print("start", sigma, "worst |error| %.3f px" % start.max())
    assert (start > 1.0).any()
    for name in ("corner", "lines"):
        assert np.abs(errors[(name, sigma)][0]).max() < start.max()


def test_vertices_against_truth():
    """The vertices themselves, not only the diagonal they give."""
    for sigma in (0.0, 1.0):
        for d in SC.square_draws(sigma)[:8]:
            v = np.array(R.refine_one(d.prob, [int(c) for c in d.box], R.lines_params())[0]).reshape(4, 2)
            assert np.abs(v - d.truth).max() <= 0.4, (sigma, np.abs(v - d.truth).max())


# ------------------------------------------------------------------------------------------------ pieces against brute force
def test_sample_is_bilinear_and_clamped():
    rng = np.random.default_rng(1)
    m = rng.random((5, 7)).astype(np.float32)
    for y in range(5):
        for x in range(7):
            assert R.sample(m, float(x), float(y)) == float(m[y, x])
    assert R.sample(m, 2.5, 1.0) == float(m[1, 2]) * 0.5 + float(m[1, 3]) * 0.5
    assert R.sample(m, -3.0, -9.0) == float(m[0, 0]) and R.sample(m, 99.0, 99.0) == float(m[4, 6])
    assert R.sample(m, float("nan"), float("inf")) == float(m[4, 0]) and R.sample(m, 6.0, 4.0) == float(m[4, 6])
    one = np.array([[0.25]], np.float32)
    assert R.sample(one, 3.0, -2.0) == 0.25
    row = np.array([[0.0, 1.0, 0.5]], np.float32)
    assert R.sample(row, 0.25, 7.0) == 0.25 and R.sample(row, 1.5, 0.0) == 0.75


def test_crossing_rule_against_brute_force():
    rng = np.random.default_rng(2)
    seen_tie = seen_none = 0
    for trial in range(400):
        reach = int(rng.integers(1, 6))
        g = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0, float("nan"), float("inf")], size=2 * reach + 1).tolist()
        level = float(rng.choice([0.45, 0.5]))
        if trial % 7 == 0 and reach >= 2:                        # crossings at -1.5 and +1.5: the same distance
            g = [0.0] * (2 * reach + 1)
            g[reach - 2], g[reach + 1], level = 1.0, 1.0, 0.5
        cand = []
        for t in range(-reach, reach):
            g0, g1 = g[t + reach], g[t + reach + 1]
            if g0 >= level > g1:
                pos = t + (g0 - level) / (g0 - g1)
                if not math.isnan(pos):
                    cand.append((abs(pos), t, pos))
        pos, found = R.crossing(g, level, reach)
        assert found == bool(cand)
        if cand:
            best = min(cand)                                     # least |pos|, then the smaller t
            assert pos == best[2]
            seen_tie += sum(1 for c in cand if c[0] == best[0]) > 1
        else:
            seen_none += 1
    assert seen_tie > 5 and seen_none > 5
    assert R.crossing([1.0, 0.0, 0.0, 1.0, 0.0], 0.5, 2) == (-1.5, True)        # |-1.5| == |+1.5|: the smaller t
    assert R.crossing([float("nan")] * 5, 0.5, 2) == (0.0, False)
    assert R.crossing([float("inf"), 0.0, 0.0], 0.5, 1) == (0.0, False)         # (inf - level) / inf is NaN: never wins


def test_line_fit_against_numpy_linalg():
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.integers(3, 33))
        ang = rng.uniform(0, np.pi)
        if trial < 4:
            ang = [0.0, np.pi / 2, np.pi / 4, 3 * np.pi / 4][trial]
        t = rng.uniform(-30, 30, n)
        pts = np.stack([40 + t * np.cos(ang), 50 + t * np.sin(ang)], axis=1) + rng.normal(0, 0.05, (n, 2))
        cx, cy, vx, vy = R.tls_line(pts[:, 0].tolist(), pts[:, 1].tolist())
        assert abs(cx - pts[:, 0].mean()) < 1e-9 and abs(cy - pts[:, 1].mean()) < 1e-9
        ev, evec = np.linalg.eigh(np.cov((pts - pts.mean(axis=0)).T, bias=True))
        major = evec[:, 1]
        nrm = math.hypot(vx, vy)
        assert nrm > 0 and abs(abs((vx * major[0] + vy * major[1]) / nrm) - 1.0) < 1e-9
    assert R.tls_line([1.0, 1.0, 1.0], [2.0, 2.0, 2.0])[2:] == (0.0, 0.0)         # coincident points: no direction


def test_diagonal_rule_is_the_records_rule():
    rng = np.random.default_rng(4)
    for _ in range(50):
        box = rng.integers(-5, 60, 8)
        d = [math.dist(box[2 * a:2 * a + 2], box[2 * c:2 * c + 2]) for a, c in itertools.combinations(range(4), 2)]
        pairs = list(itertools.combinations(range(4), 2))
        k = int(np.argmax(d))                                      # the first longest
        rest = [q for q in range(4) if q not in pairs[k]]
        d1, d2, dm = R.diagonals([float(c) for c in box], 1.0)
        assert d1 == max(d) and abs(d2 - math.dist(box[2 * rest[0]:2 * rest[0] + 2], box[2 * rest[1]:2 * rest[1] + 2])) < 1e-12
        assert dm == 0.5 * (d1 + d2)


def test_inv_scale_scales_the_diagonals_and_offsets_cancel():
    d = SC.square_draws(1.0)[0]
    box = [int(c) for c in d.box]
    for p in (R.corner_params(), R.lines_params()):
        base = R.refine_one(d.prob, box, p)
        for aff in ((0.0, 0.0, 6.0), (17.0, -3.5, 6.0), (0.25, 100.0, 1.0 / 3.0)):
            r = R.refine_one(d.prob, box, p, aff)
            assert r[0] == base[0] and r[2] == base[2]
            v = base[0]
            dmax = max(math.sqrt((v[2 * a] - v[2 * c]) ** 2 + (v[2 * a + 1] - v[2 * c + 1]) ** 2) for a, c in itertools.combinations(range(4), 2))
            assert r[4] == dmax * aff[2] and r[6] == 0.5 * (r[4] + r[5])
            assert r[1][0] == (v[0] - aff[0]) * aff[2] and r[1][7] == (v[7] - aff[1]) * aff[2]
        a, b = R.refine_one(d.prob, box, p, (0.0, 0.0, 4.0)), R.refine_one(d.prob, box, p, (9.0, 9.0, 4.0))
        assert a[4:] == b[4:] and a[4] == base[4] * 4.0 and a[5] == base[5] * 4.0          # a power of two: exact


# ------------------------------------------------------------------------------------------------ the built cases say what they claim
_CASES = SC.gpu_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_built_cases(case):
    recs = SC.records(case.kind, case.boxes, case.valid)
    sent = np.full(recs.shape + (R.QUAD_DT.itemsize,), 0xA5, np.uint8).reshape(-1).view(R.QUAD_DT).reshape(recs.shape)
    out = R.refine_ref(case.prob, recs, case.counts, case.params, case.affine, out=sent)
    again = R.refine_ref(case.prob, recs, case.counts, case.params, case.affine, out=sent)
    assert out.tobytes() == again.tobytes()
    B, M = recs.shape
    seen = 0
    for b in range(B):
        used = min(max(int(case.counts[b]), 0), M)
        assert out[b, used:].tobytes() == sent[b, used:].tobytes()
        for s in range(used):
            o = out[b, s]
            assert o["label"] == recs[b, s]["label"] and o["area"] == recs[b, s]["area"] and o["reserved"] == 0
            if not o["valid"]:
                assert o.tobytes()[12:] == bytes(R.QUAD_DT.itemsize - 12)
                continue
            seen |= int(np.bitwise_or.reduce(o["flags"]))
            start = recs[b, s]["box"].astype(np.float64)
            lim = float(case.params["win"]) if case.params["method"] == R.CORNER else case.params["max_shift"]
            moved = np.abs(o["v"] - start)
            for i in range(4):
                keeps = o["flags"][i] & (R.RESTORED | R.SHORT_SIDE | R.NO_EDGE | R.PARALLEL)
                assert (moved[2 * i:2 * i + 2] == 0).all() if keeps else (moved[2 * i:2 * i + 2] <= lim).all()
            assert np.isfinite(o["v"]).all() and np.isfinite(o["d_mean"])
    assert seen & case.expect_flags == case.expect_flags, (case.name, seen)


def test_built_cases_cover_every_flag_and_parameter():
    flags = 0
    seen = {k: set() for k in ("win", "zero_zone", "max_iter", "reach", "n_stations", "level")}
    sizes, batches = set(), set()
    for c in _CASES:
        out = R.refine_ref(c.prob, SC.records(c.kind, c.boxes, c.valid), c.counts, c.params, c.affine)
        flags |= int(np.bitwise_or.reduce(out["flags"].reshape(-1)))
        for k in seen:
            if k in c.params:
                seen[k].add(c.params[k])
        sizes.add(c.prob.shape[1:])
        batches.add(c.prob.shape[0])
    assert flags == 127, flags
    assert seen["win"] >= {2, 5, 15} and seen["zero_zone"] >= {-1, 0, 2} and seen["max_iter"] >= {1, 40}
    assert seen["reach"] >= {1, 15} and seen["n_stations"] >= {3, 32} and seen["level"] >= {0.45, 0.5}
    assert sizes >= {(1, 1), (4, 4), (32, 32), (40, 56), (96, 160)} and batches >= {1, 3}


# ------------------------------------------------------------------------------------------------ the reference's own label masks
@pytest.fixture(scope="module")
def real_records():
    out = []
    for idx in range(8):
        m = IC.real_mask(GOLDEN, idx)
        sy, sx = max(1, m.shape[0] // 256), max(1, m.shape[1] // 256)
        m = np.ascontiguousarray(m[::sy, ::sx]).astype(np.float32)
        cfg = GC.Cfg(thresh=0.5, k=1, min_area=30, cap=16, outset=2)
        _, _, recs = GC.MapRef(m, cfg).expected("quad", cfg)
        out.append((m, recs))
    return out


@pytest.mark.parametrize("method", ["corner", "lines"])
def test_real_masks_through_the_quad_fit(real_records, method):
    p = R.corner_params() if method == "corner" else R.lines_params()
    lim = 5.0 if method == "corner" else 6.0
    n_valid = 0
    for m, recs in real_records:
        r = recs[None]
        out = R.refine_ref(m[None], r, [len(recs)], p)
        assert out.tobytes() == R.refine_ref(m[None], r, [len(recs)], p).tobytes()              # deterministic
        for s in range(len(recs)):
            o = out[0, s]
            assert o["valid"] == int(recs[s]["valid"] != 0)
            if not o["valid"]:
                continue
            n_valid += 1
            moved = np.abs(o["v"] - recs[s]["box"].astype(np.float64)).reshape(4, 2).max(axis=1)
            for i in range(4):
                assert moved[i] <= lim or o["flags"][i] != 0
                if o["flags"][i] & (R.RESTORED | R.SHORT_SIDE | R.NO_EDGE | R.PARALLEL):
                    assert moved[i] == 0.0
    assert n_valid >= 8


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def _call(vk, null=None, off=None, **kw):
    L = vk._lib
    lib = L.lib()
    method = kw.pop("method", "corner")
    a = dict(batch=1, h=8, w=8, stride=96, box_off=8, valid_off=-1, cap=2)
    pkw = {k: kw.pop(k) for k in list(kw) if k not in a and k != "wt"}
    wt = kw.pop("wt", None)
    a.update(kw)
    p = vk.subpix.params(method, **pkw)
    if wt is not None:
        p.wt[wt[0]] = wt[1]
    bufs = dict(prob=np.full(64, 7, np.float32), records=np.full(96, 7, np.int32), counts=np.full(4, 7, np.int32),
                affine=np.full(8, 7.0), out=np.full(128, 7.0))

    def ptr(name):
        if null == name:
            return None
        return bufs[name].ctypes.data + (off[1] if off and off[0] == name else 0)

    rc = lib.vk_subpix_refine(None if null == "params" else C.byref(p), a["batch"], a["h"], a["w"], ptr("prob"), ptr("records"), a["stride"],
                              a["box_off"], a["valid_off"], ptr("counts"), a["cap"], ptr("affine"), ptr("out"), None)
    for name, b in bufs.items():
        assert (b == 7).all(), name
    return rc, lib.vk_last_error_string().decode()


def test_library_and_python_exports(vk):
    L = vk.lib()
    assert hasattr(L, "vk_subpix_refine") and "vk_subpix_refine" in vk._lib.SIGNATURES
    assert "subpix" in vk.__all__ and "RefinedDetections" in vk.__all__
    S = vk.subpix
    assert S.RECORD_DTYPE == R.QUAD_DT and C.sizeof(vk._lib.vk_subpix_quad) == 200 and vk._lib.vk_subpix_quad.d_mean.offset == 192
    assert S.FLAGS == dict(singular=R.SINGULAR, left_map=R.LEFT_MAP, not_converged=R.NOT_CONVERGED, restored=R.RESTORED,
                           short_side=R.SHORT_SIDE, no_edge=R.NO_EDGE, parallel=R.PARALLEL)
    for win in (2, 5, 15):
        assert S.corner_weights(win) == R.weight_table(win)
        p = S.params("corner", win=win)
        assert list(p.wt)[:2 * win + 1] == R.weight_table(win)
    p = S.params("lines")
    assert (p.lo, p.hi, p.n_stations, p.reach, p.level, p.max_shift) == (0.1, 0.5, 12, 6, 0.5, 6.0)
    p = S.params("corner")
    assert (p.win, p.zero_zone, p.max_iter, p.eps) == (5, -1, 40, 1e-3)
    assert issubclass(S.RefinedDetections, vk.instances.Detections)


def test_refine_refuses_bad_arguments(vk):
    for kw, word in ((dict(win=1), "win = 1"), (dict(win=16), "win = 16"), (dict(zero_zone=-2), "zero_zone"), (dict(zero_zone=5), "zero_zone"),
                     (dict(max_iter=0), "max_iter = 0"), (dict(max_iter=101), "max_iter = 101"), (dict(eps=0.0), "eps"),
                     (dict(eps=float("nan")), "eps"), (dict(wt=(3, float("inf"))), "weight 3"),
                     (dict(method="lines", n_stations=2), "n_stations = 2"), (dict(method="lines", n_stations=33), "n_stations = 33"),
                     (dict(method="lines", reach=0), "reach = 0"), (dict(method="lines", reach=16), "reach = 16"),
                     (dict(method="lines", lo=0.5, hi=0.5), "lo"), (dict(method="lines", lo=-0.1), "lo"), (dict(method="lines", hi=1.5), "hi"),
                     (dict(method="lines", lo=float("nan")), "lo"), (dict(method="lines", level=float("nan")), "level"),
                     (dict(method="lines", max_shift=0.0), "max_shift"), (dict(method="lines", max_shift=float("inf")), "max_shift"),
                     (dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=-1), "map size"),
                     (dict(h=1 << 15, w=1 << 15), "2^30"), (dict(cap=0), "max_components = 0"), (dict(cap=4097), "max_components = 4097"),
                     (dict(stride=38), "record stride"), (dict(stride=36), "record stride"), (dict(box_off=6), "record stride"),
                     (dict(box_off=4), "record stride"), (dict(box_off=68), "record stride"), (dict(valid_off=-2), "valid offset"),
                     (dict(valid_off=94), "valid offset"), (dict(valid_off=96), "valid offset"), (dict(valid_off=4), "valid offset"),
                     (dict(off=("prob", 2)), "misaligned"), (dict(off=("records", 2)), "misaligned"), (dict(off=("counts", 1)), "misaligned"),
                     (dict(off=("out", 4)), "misaligned"), (dict(off=("affine", 4)), "misaligned")):
        rc, err = _call(vk, **kw)
        assert rc == -1 and word in err, (kw, err)
    for name in ("params", "prob", "records", "counts", "out"):
        rc, err = _call(vk, null=name)
        assert rc == -1 and "null" in err, name
    p = vk.subpix.params("corner")
    p.method = 2
    rc = vk.lib().vk_subpix_refine(C.byref(p), 1, 8, 8, None, None, 96, 8, -1, None, 2, None, None, None)
    assert rc == -1 and "method 2" in vk.lib().vk_last_error_string().decode()


def test_python_entry_points_refuse_wrong_arguments(vk):
    S, I = vk.subpix, vk.instances
    prob = torch.rand(2, 8, 8)
    z8, z32 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.int32)
    dets = I.Detections("rect", z8, torch.zeros(2, 4, 96, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), z32, 4)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        S.refine(dets, prob)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        S.postprocess(prob)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.object_metrics(prob, torch.zeros(2, 8, 8), refine=dict(method="lines"))
    with pytest.raises(ValueError):
        S.refine(None, prob)
    with pytest.raises(ValueError):
        S.refine(dets, prob[0])
    with pytest.raises(ValueError):
        S.params("circle")
    with pytest.raises(ValueError):
        S.params("corner", reach=3)
    with pytest.raises(ValueError):
        S.params("lines", win=3)
    with pytest.raises(ValueError):
        vk.ObjectMetrics(refine="lines")
    assert vk.ObjectMetrics().refine is None and vk.ObjectMetrics(refine=dict(method="lines")).refine == dict(method="lines")


def test_letterbox_affine(vk):
    S = vk.subpix
    a = S.letterbox_affine(2048, 3072, 512, "centered")
    scale, nh, nw, top, left = vk.prepost.letterbox_geometry(2048, 3072, 512, "centered")
    assert a.dtype == np.float64 and a.tolist() == [float(left), float(top), 1.0 / scale] and a[2] == 6.0 and a[1] == 85.0
    assert S.letterbox_affine(2048, 3072, 512, (scale, nh, nw, top, left)).tolist() == a.tolist()
    assert S.letterbox_affine(100, 100, 512, "centered").tolist() == [206.0, 206.0, 1.0]
