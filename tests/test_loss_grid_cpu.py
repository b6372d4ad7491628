"""The cases of tests/loss_grid_cases.py, the parts that need no GPU: every case takes the route it is listed under (from the nbx rules
restated there, which are also held against the workspace sizes the built library reports); zeroing any one workgroup's share, or
exchanging the shares of two classes, moves a reported component of the float64 reference by ten times the bar the GPU test applies
(so a wrong row index or a dropped share cannot pass); every active term's value lies in [0.05, 20], where the relative bar decides."""
import importlib

import numpy as np
import pytest
import torch

import keypoints_loss_cases as KC
import keypoints_loss_ref as KR
import loss_grid_cases as G
import lovasz_cases as LK
import multiclass_ref as MR
import seglosses_cases as K
import seglosses_ref as SR

vk = importlib.import_module("vickers-hardness-unet_amd")
Ls = vk.seglosses
FACTOR = 10.0


# ------------------------------------------------------------------------------------------------ routes
def test_rules_on_known_shapes():
    assert G.seg_nbx(False, 32, 1, 512 * 512) == 64 and G.seg_nbx(True, 32, 3, 512 * 512) == 32      # the training shape
    assert G.seg_nbx(True, 64, 3, 512 * 512) == 16 and G.kp_nbx(32, 2, 512 * 512) == 32
    assert G.multi_nbx(512 * 512) == 64 and G.multi_nbx(4095) == 1 and G.multi_nbx(128 * 128) == 4
    assert G.seg_nbx(True, 2, 3, 128 * 128) == 8                                                       # the fused-step test
    assert G.kp_workspace_bytes(1, 1, 1) == 16 * 8 + 16 and G.kp_workspace_bytes(2, 2, 4096) == 16 * 8 + 2 * 2 * 2 * 16
    assert G.kp_workspace_bytes(32, 2, 512 * 512) == 16 * 8 + 32 * 2 * 32 * 16                         # tests/test_keypoints_loss_cpu.py
    for HW in (4099, 4100, 6147, 6148, 131075):
        for fam in ("seg_sig", "kp", "ml"):
            r = G.route(fam, 2, 4, HW)
            got = np.concatenate([G.share(fam, 2, 4, HW, bx) for bx in range(r["nbx"])])
            assert np.array_equal(np.sort(got), np.arange(HW)) and r["V"] == (4 if HW % 4 == 0 and fam != "ml" else 1)


def test_workspace_rules_equal_the_library():
    L = vk.lib()
    for c in G.CASES:
        N, C, HW = c["N"], c["C"], c["HW"]
        if c["family"] in ("seg_sig", "seg_mc"):
            assert L.vk_seg_loss_workspace_bytes(N, C, HW) == G.seg_workspace_bytes(N, C, HW), c["id"]
        elif c["family"] == "kp":
            assert L.vk_kp_loss_workspace_bytes(N, C, HW) == G.kp_workspace_bytes(N, C, HW), c["id"]
        else:
            assert L.vk_multi_loss_workspace_bytes(N, C, HW) == G.multi_workspace_bytes(N, C, HW), c["id"]


@pytest.mark.parametrize("case", G.CASES, ids=G.ident)
def test_case_takes_its_route(case):
    fam, cls, N, C, HW = case["family"], case["cls"], case["N"], case["C"], case["HW"]
    r = G.route(fam, N, C, HW)
    wg = G.MULTI_WG_PIXELS if fam in ("ml", "mc") else G.SEG_WG_PIXELS
    lanes = G.MULTI_FINALIZE_THREADS if fam in ("ml", "mc") else G.SEG_FINALIZE_LANES
    assert r["rows"] == N * r["nbx"] and r["trips"] == -(-r["rows"] // lanes) and r["sweeps"] >= 2
    if cls == "two":
        assert r["nbx"] == 2 and r["ragged"] and HW < 2 * wg + 8 and r["trips"] == 1
    elif cls == "three":
        assert r["nbx"] == 3 and r["ragged"] and 3 * wg <= HW < 4 * wg and r["trips"] == 1
    elif cls == "cap":
        assert r["trips"] >= 2 and r["ragged"] and (r["nbx"] == G.NBX_CAP or (fam in ("ml", "mc") and r["rows"] == 260))
    elif cls == "odd":
        assert r["rows"] % lanes != 0 and r["trips"] >= 2 and 3 < r["nbx"] < G.NBX_CAP and r["ragged"]
    elif cls == "want2":
        assert r["nbx"] == 2 and HW // wg >= 3 and r["ragged"]
    elif cls == "nbx1":
        assert r["nbx"] == 1 and HW >= 2 * wg
    else:
        raise AssertionError(cls)


@pytest.mark.parametrize("fam", ["seg_sig", "seg_mc", "kp", "ml", "mc"])
def test_family_covers_every_route(fam):
    rs = [(c, G.route(fam, c["N"], c["C"], c["HW"])) for c in G.cases(fam)]
    nbxs = {r["nbx"] for _, r in rs}
    trips = {min(r["trips"], 4) for _, r in rs} | {min(r.get("trips_all", 1), 4) for _, r in rs}
    assert {2, 3, 64} <= nbxs and trips == {1, 2, 3, 4}
    assert any(r["rows"] % (G.MULTI_FINALIZE_THREADS if fam in ("ml", "mc") else 64) != 0 and r["trips"] >= 2 for _, r in rs)
    for cls in ("two", "three", "cap") + (("odd", "want2") if fam in ("seg_sig", "seg_mc", "kp") else ()):
        vs = {c["HW"] % 4 == 0 for c, _ in rs if c["cls"] == cls}
        assert vs == {True, False}, cls                                  # 16-byte and scalar kinds of HW
    idle = {r["idle_last"] for c, r in rs if c["cls"] == "three"}
    assert 2 in idle and (0 in idle or 1 in idle)      # the last workgroup with nothing on the last sweep, and a fuller last sweep
    if fam in ("seg_sig", "seg_mc", "kp"):
        assert {1, 42 if fam != "seg_mc" else 21} <= nbxs and {c["cls"] for c, _ in rs} >= {"odd", "want2", "nbx1"}
    if fam == "seg_sig":
        assert {c["C"] for c, _ in rs} == {1, 4, 16}
    if fam == "seg_mc":
        assert {c["C"] for c, r in rs if r["nbx"] >= 2} == {2, 5, 16}
        for C in (2, 5, 16):                            # the three CM widths on the multi-workgroup route, and past one finalize trip
            assert any(c["C"] == C and r["trips"] >= 2 for c, r in rs)
    names = {n for _, n in G.single_term_cases(fam)} if fam.startswith("seg") else set()
    assert names == (set(G.SINGLE_NAMES) if fam.startswith("seg") else set())


# ------------------------------------------------------------------------------------------------ sensitivity and term size
def _moved(ref, new, bars):
    bars = np.asarray(bars)
    return bool(((np.abs(np.asarray(new) - np.asarray(ref)) >= FACTOR * bars) & (bars > 0)).any())     # an absent term has bar 0 and value 0


def _project_bars(ref):
    return 1e-5 * np.abs(np.asarray(ref)) + 1e-6


def _exchange_pairs(case):
    """(n, bx) of the shares whose two classes are exchanged"""
    return sorted({(n, bx) for n, _, bx in G.sample_shares(case)})


def _seg_eval(x, t, spec):
    rf = SR.evaluate(torch.from_numpy(x), torch.from_numpy(t), spec)
    return SR.components(rf).numpy(), rf["dlogits"].numpy()


def _grad_moved(g_ref, g_new, n, idx, gbar):
    """whether an element outside the altered pixels of image n moved by FACTOR times its bar (a dropped row changes a denominator, and
    with it every element; the altered pixels themselves are the restatement's device, not what a kernel would write there)"""
    d = np.abs(g_new - g_ref)
    d[n][:, idx] = 0.0
    return bool(((d >= FACTOR * gbar) & (np.asarray(gbar) > 0)).any())      # a plane without a rule has bound 0 and gradient 0


def test_an_unchanged_result_has_not_moved():
    """the two helpers on identical values and gradients, with bars that are 0 somewhere (the planes of vk_kp_loss without a rule)"""
    g = np.random.default_rng(0).standard_normal((2, 3, 8))
    g[:, 1] = 0.0
    gbar = np.full_like(g, 1e-6)
    gbar[:, 1] = 0.0
    idx = np.array([0, 3])
    assert not _grad_moved(g, g.copy(), 0, idx, gbar) and not _grad_moved(g, g.copy(), 0, idx, 1e-6)
    assert not _moved([1.0, 0.0], [1.0, 0.0], [1e-5, 1e-6]) and not _moved([1.0, 0.0], [1.0, 0.0], [1e-5, 0.0])
    g2 = g.copy()
    g2[0, 0, 0] += 1.0                      # inside the altered pixels: not counted
    assert not _grad_moved(g, g2, 0, idx, gbar)
    g2[1, 2, 5] += 1e-4                     # outside them, 100 bars
    assert _grad_moved(g, g2, 0, idx, gbar) and _moved([1.0, 0.0], [1.0, 2e-5], [1e-5, 1e-6])


def _planes_read(spec, mode, C):
    """the class planes whose sums can change the configuration's value: all of them under a pixel-wise term; under region terms alone
    the named classes that are present (the absent class is masked out of every region term, whatever its P)"""
    terms = spec["terms"]
    if mode == "multiclass":
        return [0]                                          # a multiclass workgroup owns every class of its pixels
    if "pix" in terms or "focal" in terms:
        return list(range(C))
    named = set()
    for k in ("dice", "jaccard", "tversky"):
        if k in terms:
            named |= set(range(C)) if terms[k]["classes"] is None else set(terms[k]["classes"])
    return sorted(named - ({1} if C > 1 else set()))


def _class_dependent(spec, mode):
    """whether exchanging two classes can change anything: a region term, or a BCE term with per-class pos_weight; cross-entropy and
    the focal term are symmetric in the classes"""
    terms = spec["terms"]
    return any(k in terms for k in ("dice", "jaccard", "tversky")) or (mode != "multiclass" and "pix" in terms
                                                                      and terms["pix"]["pos_weight"] is not None)


def _check_seg(case, name):
    fam, N, C, HW = case["family"], case["N"], case["C"], case["HW"]
    mode = G.seg_mode(case)
    x, t = G.inputs(case, True)
    S = K.build(Ls, name, mode, C, True)._as_sum()
    spec = S.spec(C)
    ref, g_ref = _seg_eval(x, t, spec)
    bars, gbar = _project_bars(ref), 1e-4 * np.abs(g_ref).max()
    active = [i for i, k in enumerate(SR.KINDS) if k in spec["terms"] and spec["terms"][k]["w"] != 0]
    for i in active:
        assert 0.05 <= ref[1 + i] <= 20.0, (case["id"], name, SR.KINDS[i], ref[1 + i])
    read = _planes_read(spec, mode, C)
    for n, c, bx in G.sample_shares(case):
        if c not in read:
            continue
        idx = G.share(fam, N, C, HW, bx)
        t2 = t.copy()
        if mode == "multiclass":
            t2[n, idx] = G.IGN
        else:
            t2[n, c, idx] = float(G.IGN)
        new, g_new = _seg_eval(x, t2, spec)
        assert _moved(ref, new, bars) or _grad_moved(g_ref, g_new, n, idx, gbar), (case["id"], name, "share", n, c, bx)
    a, b = 0, C - 1
    if C > 1 and _class_dependent(spec, mode):
        for n, bx in _exchange_pairs(case):
            idx = G.share(fam, N, C, HW, bx)
            x2, t2 = x.copy(), t.copy()
            x2[n, a, idx], x2[n, b, idx] = x[n, b, idx], x[n, a, idx]
            if mode == "multiclass":
                old = t[n, idx]
                t2[n, idx] = np.where(old == a, b, np.where(old == b, a, old))
            else:
                t2[n, a, idx], t2[n, b, idx] = t[n, b, idx], t[n, a, idx]
            new, g_new = _seg_eval(x2, t2, spec)
            assert _moved(ref, new, bars) or _grad_moved(g_ref, g_new, n, idx, gbar), (case["id"], name, "exchange", n, bx)


@pytest.mark.parametrize("case", G.cases("seg_sig") + G.cases("seg_mc"), ids=G.ident)
def test_seg_sum5_is_sensitive_and_sized(case):
    _check_seg(case, "sum5")


@pytest.mark.parametrize("case,name", G.single_term_cases("seg_sig") + G.single_term_cases("seg_mc"),
                         ids=lambda v: v if isinstance(v, str) else G.ident(v))
def test_seg_single_term_is_sensitive_and_sized(case, name):
    _check_seg(case, name)


def _ml_components(x, y):
    tot, b, d, _ = MR.multilabel(torch.from_numpy(x), torch.from_numpy(y))
    return np.array([tot.item(), b.item(), d.item()])


@pytest.mark.parametrize("case", G.cases("ml"), ids=G.ident)
def test_multilabel_is_sensitive_and_sized(case):
    N, C, HW = case["N"], case["C"], case["HW"]
    x, y = G.inputs(case)
    ref = _ml_components(x, y)
    bars = _project_bars(ref)
    assert all(0.05 <= v <= 20.0 for v in ref[1:]), ref
    for n, c, bx in G.sample_shares(case):
        idx = G.share("ml", N, C, HW, bx)
        x2, y2 = x.copy(), y.copy()
        x2[n, c, idx], y2[n, c, idx] = -100.0, 0.0           # BCE 4e-44, p 4e-44, y 0: the share adds nothing to any of the four sums
        assert _moved(ref, _ml_components(x2, y2), bars), (case["id"], "share", n, c, bx)
    if C > 1:
        a, b = 0, C - 1
        for n, bx in _exchange_pairs(case):
            idx = G.share("ml", N, C, HW, bx)
            x2, y2 = x.copy(), y.copy()
            x2[n, a, idx], x2[n, b, idx], y2[n, a, idx], y2[n, b, idx] = x[n, b, idx], x[n, a, idx], y[n, b, idx], y[n, a, idx]
            assert _moved(ref, _ml_components(x2, y2), bars), (case["id"], "exchange", n, bx)


def _mc_components(x, t, keep=None):
    """CE + Dice of MR.multiclass; keep: the batch as one image of the kept pixels, the cross-entropy sum still divided by all N HW
    pixels (what a dropped row of partials gives: the Dice sums lose the share, the count does not)"""
    N, C, HW = x.shape
    if keep is None:
        tot, ce, d, _ = MR.multiclass(torch.from_numpy(x), torch.from_numpy(t))
        return np.array([tot.item(), ce.item(), d.item()])
    xf = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(1, C, N * HW)[:, :, keep])
    _, ce, d, _ = MR.multiclass(torch.from_numpy(xf), torch.from_numpy(t.reshape(1, N * HW)[:, keep]))
    ce = ce.item() * keep.sum() / (N * HW)
    return np.array([ce + d.item(), ce, d.item()])


@pytest.mark.parametrize("case", G.cases("mc"), ids=G.ident)
def test_multiclass_is_sensitive_and_sized(case):
    N, C, HW = case["N"], case["C"], case["HW"]
    x, t = G.inputs(case)
    ref = _mc_components(x, t)
    assert np.abs(_mc_components(x, t, np.ones(N * HW, bool)) - ref).max() <= 1e-12        # the flattened form is the same loss
    bars = _project_bars(ref)
    assert all(0.05 <= v <= 20.0 for v in ref[1:]), ref
    present = {int(v) for v in np.unique(t)}
    assert present == set(range(C)) - ({1} if C > 2 else set())
    for n, _, bx in G.sample_shares(case):
        keep = np.ones(N * HW, bool)
        keep[n * HW + G.share("mc", N, C, HW, bx)] = False
        assert _moved(ref, _mc_components(x, t, keep), bars), (case["id"], "share", n, bx)
    a, b = 0, C - 1
    for n, bx in _exchange_pairs(case):
        idx = G.share("mc", N, C, HW, bx)
        x2, t2 = x.copy(), t.copy()
        x2[n, a, idx], x2[n, b, idx] = x[n, b, idx], x[n, a, idx]
        old = t[n, idx]
        t2[n, idx] = np.where(old == a, b, np.where(old == b, a, old))
        assert _moved(ref, _mc_components(x2, t2), bars), (case["id"], "exchange", n, bx)


def _kp_eval(x, y, c):
    r = KR.evaluate(x, y, c)
    return np.array([r["total"], r["heat"], r["bce"]]), r["grad"]


@pytest.mark.parametrize("case", G.cases("kp"), ids=G.ident)
def test_keypoint_loss_is_sensitive_and_sized(case):
    N, C, HW = case["N"], case["C"], case["HW"]
    x, y = G.inputs(case)
    c = G.kp_ref_cfg(case)
    rf, bnd = KC.bounds(x, y, c)
    ref = np.array([rf["total"], rf["heat"], rf["bce"]])
    bars = np.array([bnd["total"], bnd["heat"], bnd["bce"]])
    assert 0.05 <= ref[1] <= 20.0 and (not c["bce"] or 0.05 <= ref[2] <= 20.0), ref
    assert all(0 < rf["positives"][q] < N * HW for q in c["heat"])
    ruled = sorted(c["heat"] + c["bce"])
    for n, q, bx in G.sample_shares(case):
        q = ruled[q % len(ruled)]                           # a plane without a rule is not read
        idx = G.share("kp", N, C, HW, bx)
        x2, y2 = x.copy(), y.copy()
        x2[n, q, idx], y2[n, q, idx] = -100.0, 0.0          # a negative of value below 4e-44 under either rule
        new, g_new = _kp_eval(x2, y2, c)
        assert _moved(ref, new, bars) or _grad_moved(rf["grad"], g_new, n, idx, bnd["grad"]), (case["id"], "share", n, q, bx)
    if c["heat"] and c["bce"]:
        a, b = c["heat"][0], c["bce"][0]
        for n, bx in _exchange_pairs(case):
            idx = G.share("kp", N, C, HW, bx)
            x2, y2 = x.copy(), y.copy()
            x2[n, a, idx], x2[n, b, idx], y2[n, a, idx], y2[n, b, idx] = x[n, b, idx], x[n, a, idx], y[n, b, idx], y[n, a, idx]
            new, g_new = _kp_eval(x2, y2, c)
            assert _moved(ref, new, bars) or _grad_moved(rf["grad"], g_new, n, idx, bnd["grad"]), (case["id"], "exchange", n, bx)


# ------------------------------------------------------------------------------------------------ the Lovasz launch caps
@pytest.mark.parametrize("name", [c[0] for c in G.LOVASZ])
def test_lovasz_cap_cases(name):
    _, N, C, HW, second = next(c for c in G.LOVASZ if c[0] == name)
    assert C == 2 and second < N * HW <= second + 64                   # just above the cap: the second trip is a handful of pixels
    x, t = G.lovasz_inputs(name)
    assert {int(v) for v in t.unique()} == {0, 1, G.IGN}
    d0 = LK.softmax_d0(x, t, False, G.IGN)
    print("%s: d0 %.3e (recorded %.3e)" % (name, d0, G.LOVASZ_D0[name]))
    assert abs(d0 - G.LOVASZ_D0[name]) <= 1e-3 * G.LOVASZ_D0[name] + 1e-12
