"""Host side of the geometry front end (no GPU): the record layouts the package derives from its ctypes structures against the tests'
hand-written dtypes, the one record-to-dict path on records filled through ctypes (values, key order and Python types written out
here, not produced by the package), and the refusal of slot-less Detections by everything that needs the slot map."""
import ctypes as C

import numpy as np
import pytest
import torch

import geom_cases as GC
import instances_ref as IR
import subpix_ref as SR


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ layouts
def test_record_layouts_are_the_ctypes_structures(vk):
    L, Gm, I, S = vk._lib, vk.geometry, vk.instances, vk.subpix
    for ct, ref, size in ((L.vk_geom_det, GC.DET_DT, 96), (L.vk_geom_quad, GC.QUAD_DT, 104), (L.vk_subpix_quad, SR.QUAD_DT, 200),
                          (L.vk_inst_stats, IR.STATS_DT, 136)):
        dt = np.dtype(ct)
        assert dt == ref and dt.names == ref.names and dt.itemsize == ref.itemsize == C.sizeof(ct) == size
        for name in ref.names:
            assert dt.fields[name][1] == ref.fields[name][1] == getattr(ct, name).offset, name
            assert dt.fields[name][0] == ref.fields[name][0], name
    assert I.STATS_DTYPE == IR.STATS_DT and S.RECORD_DTYPE == SR.QUAD_DT
    assert I.Detections is Gm.Detections and I.detect is Gm.detect and vk.Detections is Gm.Detections
    z = torch.zeros(1, 2, 2, dtype=torch.uint8)
    for fit, ref in (("rect", GC.DET_DT), ("quad", GC.QUAD_DT)):
        d = Gm.Detections(fit, z, torch.zeros(1, 1, ref.itemsize, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), None, 1)
        assert d.record_dtype == ref and d.record_bytes == ref.itemsize
        assert d.diag_offset == ref.fields["d_mean"][1] and d.box_offset == ref.fields["box"][1] == 8
        assert d.valid_offset == (ref.fields["valid"][1] if fit == "quad" else -1)
    assert GC.QUAD_DT.fields["valid"][1] == 48


# ------------------------------------------------------------------------------------------------ records -> dicts
CAP = 3


def _detections(vk, fit, ct, recs, counts):
    """Detections on CPU tensors whose raw bytes are `recs` (one list of field dicts per map, padded to CAP with 0xA5 slots)."""
    arr = (ct * (len(recs) * CAP))()
    C.memset(arr, 0xA5, C.sizeof(arr))
    for b, rows in enumerate(recs):
        for s, fields in enumerate(rows):
            r = arr[b * CAP + s]
            C.memset(C.byref(r), 0, C.sizeof(r))
            for k, v in fields.items():
                if k == "box":
                    r.box[:] = v
                else:
                    setattr(r, k, v)
    raw = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).reshape(len(recs), CAP, C.sizeof(ct))
    z = torch.zeros(len(recs), 4, 4, dtype=torch.uint8)
    return vk.geometry.Detections(fit, z, raw, torch.tensor(counts, dtype=torch.int32), None, CAP)


def _same(got, exp, path="."):
    """Equal values, key order, container types and the type of every scalar."""
    assert type(got) is type(exp), (path, type(got), type(exp))
    if isinstance(exp, dict):
        assert list(got) == list(exp), (path, list(got), list(exp))
        for k in exp:
            _same(got[k], exp[k], f"{path}/{k}")
    elif isinstance(exp, (list, tuple)):
        assert len(got) == len(exp), (path, len(got), len(exp))
        for i, (g, e) in enumerate(zip(got, exp)):
            _same(g, e, f"{path}[{i}]")
    elif isinstance(exp, np.ndarray):
        assert got.dtype == exp.dtype == np.int32 and got.shape == exp.shape == (4, 2) and np.array_equal(got, exp), (path, got, exp)
        assert got.flags.owndata and got.flags.c_contiguous and got.flags.writeable, path
    else:
        assert got == exp, (path, got, exp)


def _box(*c):
    return np.array(c, np.int32).reshape(4, 2)


def test_float32_fields_widen_exactly():
    assert f32(0.1) == 0.10000000149011612 != 0.1 and f32(-1e-7) == -1.0000000116860974e-07 != -1e-7


def test_rect_records_to_dicts(vk):
    b0 = [-3, -2, 10, -2, 10, 9, -3, 9]
    b1 = [0, 0, 5, 0, 5, 5, 0, 5]
    b2 = [100, 200, 300, 200, 300, 400, 100, 400]
    common = dict(cx=0.1, cy=-1e-7, rw=13.3, rh=11.7, ux=0.6, uy=-0.8, d1=17.029386365926403, d2=0.1, d_mean=8.564693182963202)
    recs = [[dict(label=1, area=50, box=b0, hull_n=4, **common),
             dict(label=2, area=70, box=b1, hull_n=5, **common),
             dict(label=3, area=70, box=b2, hull_n=6, **common)],                 # equal areas: 2 stays before 3
            [dict(label=4, area=1, box=b1, hull_n=1, **common),
             dict(label=7, area=2 ** 31 - 1, box=b0, hull_n=2, **common),
             dict(label=9, area=3, box=b2, hull_n=3, **common)],                  # count 5 > CAP: the three listed ones
            []]                                                                    # count 0: the 0xA5 slots are not read
    dets = _detections(vk, "rect", vk._lib.vk_geom_det, recs, [3, 5, 0])

    def exp(label, area, box, hull_n):
        return {"label": label, "area": area, "box": _box(*box), "center": (f32(0.1), f32(-1e-7)), "d1": 17.029386365926403, "d2": 0.1,
                "d_mean": 8.564693182963202, "size": (f32(13.3), f32(11.7)), "direction": (f32(0.6), f32(-0.8)), "hull_vertices": hull_n}

    want = [[exp(2, 70, b1, 5), exp(3, 70, b2, 6), exp(1, 50, b0, 4)],
            [exp(7, 2 ** 31 - 1, b0, 2), exp(9, 3, b2, 3), exp(4, 1, b1, 1)],
            []]
    rows = dets.records()
    assert [len(r) for r in rows] == [3, 3, 0] and all(r.dtype == GC.DET_DT for r in rows)
    got = [vk.geometry._records(r) for r in rows]
    _same(got, want)
    assert not np.shares_memory(got[0][0]["box"], rows[0])
    again = dets.records(np.array([3, 5, 0], np.int32))                           # host counts handed over: the same rows
    assert [a.tobytes() for a in again] == [r.tobytes() for r in rows]


def test_quad_records_to_dicts(vk):
    b0 = [-7, 1, 4, -6, 12, 3, 1, 11]
    b1 = [0, 0, 9, 0, 9, 9, 0, 9]
    common = dict(cx=0.1, cy=-1e-7, quality=0.1, d1=12.5, d2=-1e-7, d_mean=6.25)
    recs = [[dict(label=1, area=40, box=b0, valid=1, branch=1, n_candidates=2, contour_n=33, hull_n=8, flags=0, **common),
             dict(label=2, area=90, box=b1, valid=0, branch=0, n_candidates=0, contour_n=4, hull_n=4, flags=1, **common),   # dropped
             dict(label=3, area=40, box=b1, valid=1, branch=2, n_candidates=12, contour_n=35, hull_n=9, flags=0, **common)],
            [dict(label=5, area=10, box=b1, valid=1, branch=3, n_candidates=1, contour_n=20, hull_n=5, flags=0, **common),
             dict(label=6, area=30, box=b0, valid=1, branch=7, n_candidates=1, contour_n=21, hull_n=6, flags=1, **common),  # unknown
             dict(label=8, area=20, box=b0, valid=2, branch=0, n_candidates=3, contour_n=22, hull_n=7, flags=0, **common)],
            []]
    dets = _detections(vk, "quad", vk._lib.vk_geom_quad, recs, [3, 4, 0])

    def exp(label, area, box, branch, n_candidates, contour_n, hull_n, flags):
        return {"label": label, "area": area, "box": _box(*box), "center": (f32(0.1), f32(-1e-7)), "d1": 12.5, "d2": -1e-7, "d_mean": 6.25,
                "quality": 0.1, "branch": branch, "n_candidates": n_candidates, "contour_points": contour_n, "hull_vertices": hull_n,
                "flags": flags}

    want = [[exp(1, 40, b0, "bisection", 2, 33, 8, 0), exp(3, 40, b1, "subsample", 12, 35, 9, 0)],
            [exp(6, 30, b0, "?", 1, 21, 6, 1), exp(8, 20, b0, "none", 3, 22, 7, 0), exp(5, 10, b1, "extremes", 1, 20, 5, 0)],
            []]
    rows = dets.records()
    assert [len(r) for r in rows] == [3, 3, 0] and all(r.dtype == GC.QUAD_DT for r in rows)
    assert rows[0]["valid"].tolist() == [1, 0, 1]                                # the invalid record is in records(), not in the list
    _same([vk.geometry._quad_records(r) for r in rows], want)


# ------------------------------------------------------------------------------------------------ slot-less Detections
def test_slotless_detections_are_refused(vk):
    I, S = vk.instances, vk.subpix
    z8, z32 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.int32)
    raw, counts = torch.zeros(2, 4, 96, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    bare, full = I.Detections("rect", z8, raw, counts, None, 4), I.Detections("rect", z8, raw, counts, z32, 4)
    for pair in ((bare, full), (full, bare), (bare, bare)):
        with pytest.raises(ValueError, match="slots=False"):
            I.contingency(*pair)
        with pytest.raises(ValueError, match="slots=False"):
            I.match(*pair)
    with pytest.raises(ValueError, match="slots=False"):
        S.refine(bare, torch.rand(2, 8, 8))
    assert [len(r) for r in bare.records()] == [0, 0]                            # the records need no slot map
