"""Host side of vk.sweep (no GPU): the numpy restatement (tests/sweep_ref.py) against direct evaluation, against the oracle's
dice_coef / iou_coef and the reference's recorded outputs; its conventions; and the argument checks of vk_sweep_hist /
vk_sweep_curves through the loaded library and of the Python entry points."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import multiclass_eval_ref as MR
import sweep_cases as SC
import sweep_ref as R
from conftest import GOLDEN

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ restatement vs direct evaluation
@pytest.mark.parametrize("case", SC.HIST_CASES, ids=SC.HIST_IDS)
def test_suffix_sums_equal_direct_counts(case):
    """For every threshold the histogram's suffix sums are the directly evaluated counts ((pv > thr[k]) & valid)."""
    thr, pred, tgt = SC.build_hist_case(case)
    hist, bad = R.hist_ref(pred, tgt, thr, ignore_index=case.ignore)
    assert hist.dtype == np.int32 and hist.shape == (case.n, case.c, 2, case.K + 1) and (hist >= 0).all()
    Ik, Pk, T, valid = R.suffix_counts(hist)
    ks = range(case.K) if case.plane <= 96 * 160 or case.K <= 99 else (0, case.K // 2, case.K - 1)
    for k in ks:
        i, p, t, v = R.direct_counts(pred, tgt, thr[k], ignore_index=case.ignore)
        assert (Ik[k] == i).all() and (Pk[k] == p).all() and (T == t).all() and (valid == v).all(), k
    tf = tgt.astype(F32)
    skipped = ~((tf == 0) | (tf == 1))
    if case.ignore is not None:
        assert bad == int((skipped & (tf != case.ignore)).sum())
    else:
        assert bad == int(skipped.sum())
    assert int(valid.sum()) + int(skipped.sum()) == tgt.size
    if case.values == "saturated":
        assert (hist[..., 1:case.K] == 0).all()
    if case.values == "one_bin":
        b = max(1, case.K // 2)
        assert (np.delete(hist, b, axis=-1) == 0).all()


def test_bin_conventions():
    thr = np.array([0.25, 0.5, 0.75], F32)
    up, down = np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0))
    pv = np.array([np.nan, -np.inf, np.inf, 0.25, 0.5, up, down, 0.75, 1.0, -0.0], F32)
    assert R.bins(pv, thr).tolist() == [0, 0, 3, 0, 1, 2, 1, 2, 3, 0]
    assert (R.bins(pv, thr) == [(v > thr).sum() for v in pv]).all()            # the definition, NaN included


def test_zero_denominators_and_ties():
    # one image, one class, K = 3; nothing valid at all: every ratio has a zero denominator
    empty = R.curves_ref(np.zeros((1, 1, 2, 4), np.int32))
    for name in ("precision", "recall", "f1", "micro_iou"):
        assert (empty[name] == 1.0).all(), name
    assert (empty["fpr"] == 0.0).all()
    assert (empty["per_image"] == 1.0).all()                                   # (0 + eps) / (0 + eps)
    assert empty["best_dice"].tolist() == [0] and empty["best_f1"].tolist() == [0] and empty["best_mean"].tolist() == [0, 0]
    assert empty["ap"][0] == 1.0                                                # recall 1 down to recall_K = 0 at precision 1
    assert empty["auc"][0] == 1.0                                               # (1, 1) -> (0, 1): the one step that has a width
    # a perfect map: positives in bin K, negatives in bin 0; every threshold separates them
    h = np.zeros((1, 1, 2, 4), np.int32)
    h[0, 0, 0, 0], h[0, 0, 1, 3] = 90, 10
    c = R.curves_ref(h)
    assert (c["precision"] == 1).all() and (c["recall"] == 1).all() and (c["fpr"] == 0).all()
    assert c["ap"][0] == 1.0 and c["auc"][0] == 1.0
    assert c["best_dice"].tolist() == [0] and c["best_iou"].tolist() == [0] and c["best_f1"].tolist() == [0]     # all tie: the lowest k
    # the best is in the middle, twice: the lower one wins
    v = np.array([[0.1], [0.7], [0.7], [0.2]], F32)
    assert R.first_best(v).tolist() == [1]


def test_stats_partition_the_valid_elements():
    case = next(c for c in SC.HIST_CASES if c.name == "target_ignore_f32")
    thr, pred, tgt = SC.build_hist_case(case)
    out, hist, bad = R.sweep_ref(pred, tgt, thr, ignore_index=case.ignore)
    st = out["stats"]
    assert (st >= 0).all() and (st.sum(axis=1) == hist.astype(np.int64).sum(axis=(2, 3))[None]).all()
    assert (np.diff(st[:, 0], axis=0) <= 0).all() and (np.diff(st[:, 3], axis=0) >= 0).all()    # tp falls and tn rises with the threshold
    assert bad > 0


# ------------------------------------------------------------------------------------------------ restatement vs the oracle
@pytest.mark.parametrize("shape", [(1, 1, 7, 5), (3, 1, 37, 53), (70, 1, 16, 16)])
def test_per_image_scores_equal_the_oracle_composition(oracle, shape):
    """dice_coef / iou_coef (train.py:230-281) composed per image in torch fp32, as test_seg_metrics_shapes_vs_oracle spells them out,
    at several thresholds of the default grid: bit for bit.  The batch mean at 0.5 against the oracle's own functions."""
    g = torch.Generator().manual_seed(sum(shape))
    prob = torch.sigmoid(torch.randn(*shape, generator=g) * 3)
    tgt = (torch.rand(*shape, generator=g) > 0.7).float()
    tgt[0].zero_()
    if shape[0] > 1:
        prob[1].fill_(0.1)
    thr = R.default_thresholds()
    out, _, bad = R.sweep_ref(prob.numpy(), tgt.numpy(), thr)
    assert bad == 0
    T = tgt.sum(dim=(1, 2, 3))
    for k in (0, 24, 44, 49, 98):
        pred = (prob > float(thr[k])).float()
        I, P = (pred * tgt).sum(dim=(1, 2, 3)), pred.sum(dim=(1, 2, 3))
        assert np.array_equal(out["per_image"][k, :, 0, 0], ((2 * I + 1e-7) / (P + T + 1e-7)).numpy()), k
        assert np.array_equal(out["per_image"][k, :, 0, 1], ((I + 1e-7) / (P + T - I + 1e-7)).numpy()), k
    k = int(np.nonzero(thr == F32(0.5))[0][0])
    assert float(out["mean_dice"][k]) == pytest.approx(oracle.dice_coef(prob, tgt), abs=2e-7)
    assert float(out["mean_iou"][k]) == pytest.approx(oracle.iou_coef(prob, tgt), abs=2e-7)


def test_reference_golden_at_one_half():
    """tests/golden/metrics_ref.json holds outputs of the reference's own dice_coef / iou_coef; the row with thr[k] == 0.5 reproduces
    them to the bar the vk_seg_metrics test holds that fixture to."""
    thr = R.default_thresholds()
    k = int(np.nonzero(thr == F32(0.5))[0][0])
    for c in json.load(open(GOLDEN / "metrics_ref.json")):
        g = torch.Generator().manual_seed(c["seed"])
        prob = torch.rand(c["n"], 1, c["s"], c["s"], generator=g)
        tgt = (torch.rand(c["n"], 1, c["s"], c["s"], generator=g) > c["thr"]).float()
        if c["seed"] == 3:
            tgt.zero_()
            prob.mul_(0.4)
        out, _, _ = R.sweep_ref(prob.numpy(), tgt.numpy(), thr)
        assert float(out["mean_dice"][k]) == pytest.approx(c["dice"], abs=1.5e-7), c
        assert float(out["mean_iou"][k]) == pytest.approx(c["iou"], abs=1.5e-7), c
        assert float(out["dice"][k, 0]) == float(out["mean_dice"][k])           # one class: the class mean is the score


# ------------------------------------------------------------------------------------------------ groups and the epoch mean
@pytest.mark.parametrize("case", [c for c in SC.CURVE_CASES if c.groups], ids=[c.name for c in SC.CURVE_CASES if c.groups])
def test_groups_equal_a_per_batch_loop(case):
    """Every group's row equals the sweep of that batch alone (its images in ascending index), and the epoch score is the sequential
    float64 mean of those."""
    hist, groups, G = SC.build_curve_case(case)
    out = R.curves_ref(hist, groups, G)
    per_batch = []
    for g in range(G):
        sub = R.curves_ref(hist[groups == g])
        per_batch.append(sub)
        for name in ("dice", "iou", "mean_dice", "mean_iou"):
            assert np.array_equal(out["group_" + name][g], sub[name]), (g, name)
        for k in (0, case.K // 2, case.K - 1):                                  # and the scalar loop of tests/multiclass_eval_ref.py
            for c in range(case.c):
                assert out["group_dice"][g, k, c] == MR._mean_f64(sub["per_image"][k, :, c, 0])
                assert out["group_iou"][g, k, c] == MR._mean_f64(sub["per_image"][k, :, c, 1])
    for name in ("dice", "iou", "mean_dice", "mean_iou"):
        s = np.zeros(per_batch[0][name].shape, F64)
        for sub in per_batch:
            s = s + sub[name].astype(F64)
        assert np.array_equal(out["epoch_" + name], s / G)
        # np.mean sums pairwise.  Every score is in [0, 1], so every partial sum is at most G and each of the G - 1 additions of the
        # sequential sum rounds by at most G u (u = 2^-53, the float64 unit round-off); a pairwise sum has ceil(log2 G) levels with an
        # error of at most G u each.  The two sums differ by at most (G - 1 + ceil(log2 G)) G u; divided by G, plus one rounding of each
        # quotient (at most u each, the quotients being at most 1):
        ref = np.mean(np.stack([sub[name].astype(F64) for sub in per_batch]), axis=0)
        assert np.abs(out["epoch_" + name] - ref).max() <= (G - 1 + int(np.ceil(np.log2(G))) + 2) * 2.0 ** -53


def test_one_group_of_everything_is_the_batch_mean():
    case = next(c for c in SC.CURVE_CASES if c.name == "N70_C1_K99_onegroup")
    hist, groups, G = SC.build_curve_case(case)
    out = R.curves_ref(hist, groups, G)
    assert np.array_equal(out["group_dice"][0], out["dice"]) and np.array_equal(out["group_mean_iou"][0], out["mean_iou"])
    assert np.array_equal(out["epoch_dice"], out["dice"].astype(F64))


# ------------------------------------------------------------------------------------------------ argument checks of the library
def _hist_call(vk, n_planes=2, per_plane=8, stride=0, pred=True, target=True, K=3, thr=(0.25, 0.5, 0.75), thr_dev=True, hist=True, bad=True,
               hist_off=0):
    """vk_sweep_hist on host buffers: a failed check returns before anything is read or written (only failing calls may come here)."""
    L = vk.lib()
    p = np.full(64, 0.5, F32)
    t = np.full(64, 1.0, F32)
    th = np.asarray(thr, F32)
    td = th.copy()
    h = np.full(64, 7, np.int32)
    b = np.full(1, 7, np.int32)
    rc = L.vk_sweep_hist(n_planes, per_plane, stride, p.ctypes.data if pred else None, t.ctypes.data if target else None, 0, 0, 0, 0, K,
                         th.ctypes.data if thr is not None else None, td.ctypes.data if thr_dev else None, 0,
                         h.ctypes.data + hist_off if hist else None, b.ctypes.data if bad else None, None)
    assert (h == 7).all() and (b == 7).all()
    return rc, L.vk_last_error_string().decode()


def test_hist_refuses_null_and_sizes(vk):
    for kw in (dict(pred=False), dict(target=False), dict(thr=None), dict(thr_dev=False), dict(hist=False), dict(bad=False)):
        rc, err = _hist_call(vk, **kw)
        assert rc == -1 and "null" in err, kw
    for kw, word in ((dict(K=0), "K = 0"), (dict(K=1025, thr=np.arange(1025)), "K = 1025"), (dict(n_planes=0), "n_planes"),
                     (dict(n_planes=(1 << 20) + 1), "n_planes"), (dict(per_plane=0), "per_plane"), (dict(per_plane=2 ** 31), "per_plane"),
                     (dict(per_plane=8, stride=7), "plane_stride"), (dict(hist_off=2), "misaligned")):
        rc, err = _hist_call(vk, **kw)
        assert rc == -1 and word in err, (kw, err)


@pytest.mark.parametrize("thr,word", [((0.5, 0.5, 0.75), "ascending"), ((0.5, 0.25, 0.75), "ascending"), ((0.25, np.nan, 0.75), "finite"),
                                      ((0.25, 0.5, np.inf), "finite"), ((-np.inf, 0.5, 0.75), "finite")])
def test_hist_refuses_a_bad_threshold_list(vk, thr, word):
    rc, err = _hist_call(vk, thr=thr)
    assert rc == -1 and word in err


def _round8(b):
    return (b + 7) // 8 * 8


@pytest.mark.parametrize("n,c,k,g", [(1, 1, 1, 0), (2, 3, 99, 0), (70, 16, 1024, 0), (6, 1, 99, 3), (65535, 1, 1, 65535)])
def test_layout_has_the_documented_sizes(vk, n, c, k, g):
    L = vk.lib()
    lay = vk._lib.vk_sweep_layout()
    assert L.vk_sweep_curves_layout(n, c, k, g, C.byref(lay)) == 0
    want = [("stats", k * 4 * n * c * 8), ("per_image", k * n * c * 2 * 4), ("dice", k * c * 4), ("iou", k * c * 4), ("mean_dice", k * 4),
            ("mean_iou", k * 4), ("micro_stats", 4 * k * c * 8), ("micro", 5 * k * c * 8), ("ap", c * 8), ("auc", c * 8), ("best_dice", c * 4),
            ("best_iou", c * 4), ("best_f1", c * 4), ("best_mean", 8), ("group_dice", g * k * c * 4), ("group_iou", g * k * c * 4),
            ("group_mean_dice", g * k * 4), ("group_mean_iou", g * k * 4), ("epoch_dice", k * c * 8 if g else 0),
            ("epoch_iou", k * c * 8 if g else 0), ("epoch_mean_dice", k * 8 if g else 0), ("epoch_mean_iou", k * 8 if g else 0)]
    assert [f for f, _ in want] == list(vk._lib.SWEEP_FIELDS)
    off = 0
    for name, size in want:
        assert getattr(lay, name) == off and off % 8 == 0, name
        off += _round8(size)
    assert lay.total_bytes == off == L.vk_sweep_curves_out_bytes(n, c, k, g)
    assert lay.workspace_bytes == ((2 * n + 2 * g) * 4 if g else 0)


def test_curves_refuses_bad_arguments(vk):
    L = vk.lib()
    lay = vk._lib.vk_sweep_layout()
    for bad in ((0, 1, 3, 0), (65536, 1, 3, 0), (2, 0, 3, 0), (2, 17, 3, 0), (2, 1, 0, 0), (2, 1, 1025, 0), (2, 1, 3, -1), (2, 1, 3, 3)):
        assert L.vk_sweep_curves_out_bytes(*bad) == 0, bad
        assert L.vk_sweep_curves_layout(*bad, C.byref(lay)) == -1, bad
    assert L.vk_sweep_curves_layout(2, 1, 3, 0, None) == -1
    n, c, k = 2, 1, 3
    need = L.vk_sweep_curves_out_bytes(n, c, k, 0)
    need_g = L.vk_sweep_curves_out_bytes(n, c, k, 2)
    hist = np.full(n * c * 2 * (k + 1), 5, np.int32)
    grp = np.zeros(n, np.int32)
    out = np.full(need_g // 8 + 2, 7, np.int64)
    ws = np.full(16, 7, np.int64)

    def call(n=n, c=c, k=k, hist_p=hist.ctypes.data, grp_p=None, g=0, ws_p=None, ws_b=0, out_p=out.ctypes.data, out_b=need_g + 16):
        rc = L.vk_sweep_curves(n, c, k, hist_p, grp_p, g, 1e-7, ws_p, ws_b, out_p, out_b, None)
        assert (out == 7).all() and (ws == 7).all() and (hist == 5).all()
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(hist_p=None), "null"), (dict(out_p=None), "null"), (dict(n=0), "N = 0"), (dict(c=17), "C = 17"), (dict(k=1025), "K = 1025"),
                     (dict(out_b=need - 1), "out too small"), (dict(out_p=out.ctypes.data + 4), "misaligned"),
                     (dict(hist_p=hist.ctypes.data + 2), "misaligned"), (dict(g=2), "together"), (dict(grp_p=grp.ctypes.data), "together"),
                     (dict(grp_p=grp.ctypes.data, g=3), "G = 3"), (dict(grp_p=grp.ctypes.data, g=2), "workspace too small"),
                     (dict(grp_p=grp.ctypes.data, g=2, ws_p=ws.ctypes.data, ws_b=31), "workspace too small"),
                     (dict(grp_p=grp.ctypes.data, g=2, ws_p=ws.ctypes.data + 4, ws_b=64), "8-byte aligned")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


# ------------------------------------------------------------------------------------------------ Python entry points
def test_default_grid_holds_the_two_reference_thresholds(vk):
    thr = vk.sweep.DEFAULT_THRESHOLDS
    assert thr.dtype == F32 and thr.shape == (99,) and np.array_equal(thr, R.default_thresholds())
    assert F32(0.5) in thr and F32(0.45) in thr and thr[49] == F32(vk.geometry.BIN_THRESH) and thr[44] == F32(vk.geometry.BIN_THRESH_QUAD)


def test_python_entry_points_refuse_wrong_arguments(vk):
    p, t = torch.rand(2, 1, 8, 8), torch.zeros(2, 1, 8, 8)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.sweep_hist(p, t)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.threshold_sweep(p, t.to(torch.uint8))
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.sweep_curves(torch.zeros(2, 1, 2, 100, dtype=torch.int32))
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        vk.ThresholdSweep().update(p, t)
    for bad_p, bad_t in ((p, t[:1]), (p[0, 0, 0], t[0, 0, 0]), (torch.rand(1, 17, 4, 4), torch.zeros(1, 17, 4, 4)), (p, t.to(torch.int64)),
                         (p, t.to(torch.float64)), (p.to(torch.int32), t), (torch.rand(2, 1, 0, 8), torch.zeros(2, 1, 0, 8)),
                         (torch.rand(1, 1, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2))):
        with pytest.raises(ValueError):
            vk.sweep_hist(bad_p, bad_t)
    for thr in ([0.5, 0.25], [0.5, 0.5], [0.1, float("nan")], [float("inf")], [], np.zeros((2, 2)), np.arange(1025) / 1025.0):
        with pytest.raises(ValueError):
            vk.sweep_hist(p, t, thresholds=thr)
        with pytest.raises(ValueError):
            vk.ThresholdSweep(thresholds=thr)
    with pytest.raises(ValueError):
        vk.sweep_hist(p, t, ignore_index=0.5)
    with pytest.raises(ValueError):
        vk.sweep_curves(torch.zeros(2, 1, 2, 100))                                       # not int32
    with pytest.raises(ValueError):
        vk.sweep_curves(torch.zeros(2, 1, 2, 50, dtype=torch.int32))                     # 49 thresholds' bins against the default 99
    with pytest.raises(ValueError):
        vk.sweep_curves(torch.zeros(2, 1, 3, 100, dtype=torch.int32))
    with pytest.raises(ValueError):
        vk.ThresholdSweep().compute()
