"""The geometry kernels of csrc/geometry.hip on the built cases of tests/geom_cases.py (-m gpu): vk_geom_minarearect and
vk_geom_quadrilateral through the C ABI with a free min_area and max_components, into sentinel-filled buffers, against references
composed from the oracle's stages.  Every comparison is equality (floats by bit pattern); tests/test_geom_cases_cpu.py proves on the
references alone that each case is what it claims to be.  DESIGN.md section 23."""
import numpy as np
import pytest

import geom_cases as GC

pytestmark = pytest.mark.gpu

CASES = [c for c in GC.all_cases() if c.family != "batch"]
PARAMS = [(c, kind) for c in CASES for kind in c.paths]


def _named(case, kind, res):
    """What the case was built to show, asserted by name on the device's own records (on top of equality with the reference)."""
    exp, rec0 = case.expect, res.recs[0, 0]
    if "ncomp" in exp:
        assert int(res.counts[0]) == exp["ncomp"]
    if case.family == "topology" and exp.get("single"):
        assert rec0["label"] == 1 and rec0["area"] == int((case.probs()[0] > 0).sum())
    if case.family == "hull":
        assert rec0["hull_n"] == (exp["chord"][1] + 1 if "chord" in exp else len(GC.lattice_polygon(exp["K"])))
    if case.family == "compaction" and case.name.startswith("dots_130x130"):
        nl = min(4225, case.cfg.cap)
        assert int(res.counts[0]) == 4225 and res.recs[0, :nl]["label"].tolist() == list(range(1, nl + 1))
        assert int((res.clean[0] > 0).sum()) == 4225                  # 4225 - cap components kept in `clean` but not listed
    if case.family == "morphology":
        assert bool((res.clean[1] == 255).all())                      # foreground up to the border stays: outside pixels never win
    if kind == "quad" and "quad" in exp:
        for key, v in exp["quad"].items():
            assert rec0[key] == (GC.BRANCH[v] if key == "branch" else v), (case.name, key, rec0)
    if kind == "quad" and case.family == "capacity":
        assert rec0["contour_n"] == exp["contour_n"] and (rec0["flags"] & 1) == exp["flags"] and rec0["flags"] & ~1 == 0
    if kind == "rect" and case.family == "degenerate" and case.name.endswith("-plain"):
        assert rec0["hull_n"] == (1 if case.name.startswith("pixel") else 4 if case.name.startswith("square2") else 2)


@pytest.mark.parametrize("case,kind", PARAMS, ids=[f"{c.family}-{c.name}-{k}" for c, k in PARAMS])
def test_case_equals_reference(case, kind):
    res = GC.run_device(kind, case.probs(), case.cfg)
    GC.check_call(kind, case, res)
    _named(case, kind, res)


@pytest.mark.parametrize("kind", ["rect", "quad"])
def test_batch_isolation_and_determinism(kind):
    """Five maps of 37 x 131 (all foreground, empty, serpentine, dots, noise) in one call: every per-image result equals the call on
    that image alone, and a second call returns the same bytes."""
    import torch

    case = GC.batch_case()
    probs = case.probs()
    res = GC.run_device(kind, probs, case.cfg)
    GC.check_call(kind, case, res)
    assert res.counts.tolist()[:2] == [1, 0] and res.counts[2] == 1 and res.counts[3] == 19 * 66
    for b in range(len(probs)):
        one = GC.run_device(kind, probs[b:b + 1], case.cfg)
        assert one.guards_ok and one.counts[0] == res.counts[b]
        assert np.array_equal(one.clean[0], res.clean[b]) and one.raw[0].tobytes() == res.raw[b].tobytes(), b
    again = GC.run_device(kind, probs, case.cfg)
    assert torch.equal(torch.from_numpy(again.clean), torch.from_numpy(res.clean))
    assert again.raw.tobytes() == res.raw.tobytes() and again.counts.tolist() == res.counts.tolist()


def test_public_api_reaches_the_two_vertex_hull():
    """A one-pixel line of 250 px passes the wrappers' floor of 200 px once the opening is off (morph_kernel = 1 or open_iter = 0): the
    m == 2 branch of k_geom_rect and the valid = 0 path of k_geom_quad through geometry.py, against the oracle's own entry points."""
    import importlib

    import torch

    from oracle import geometry_oracle as G
    from oracle import quad_oracle as Q

    vk = importlib.import_module("vickers-hardness-unet_amd")
    for kind in ("horizontal", "antidiagonal"):
        prob = GC._line(kind, 250).astype(np.float32)
        t = torch.from_numpy(prob[None]).to("cuda:0")
        for kw in (dict(morph_kernel=1), dict(open_iter=0)):
            clean, dets = vk.postprocess_minarearect_batch(t, **kw)
            clean_o, dets_o = G.postprocess_minarearect_multi(prob, **kw)
            assert np.array_equal(clean[0].cpu().numpy(), clean_o) and len(dets[0]) == len(dets_o) == 1
            dg, do = dets[0][0], dets_o[0]
            assert dg["area"] == do["area"] == 250 and dg["hull_vertices"] == len(do["hull"]) == 2
            assert np.array_equal(dg["box"], do["box"]) and (dg["d1"], dg["d2"], dg["d_mean"]) == (do["d1"], do["d2"], do["d_mean"])
            assert dg["center"] == do["center"] and dg["size"] == tuple(float(v) for v in do["rect"]["size"])
            assert dg["direction"] == tuple(float(v) for v in do["rect"]["u"])
        cq, dq = vk.postprocess_quadrilateral_batch(t, morph_kernel=1, fit_outset_px=0)
        cq_o, dq_o = Q.postprocess_quadrilateral_multi(prob, morph_kernel=1, fit_outset_px=0)
        assert np.array_equal(cq[0].cpu().numpy(), cq_o) and dq[0] == [] and dq_o == []      # kept in `clean`, dropped from the list
