"""vk.sweep on the MI355X: the histogram kernel against the numpy restatement bit for bit (probabilities and scores: nothing
transcendental between the input and the bins), the logits path against the single-threshold kernels of the same device at every
threshold, the curves pass alone on built histograms, ThresholdSweep over an epoch, the uint8 target path.  Equality everywhere:
integer counts and IEEE operations in a fixed order leave nothing to tolerate."""
import importlib

import numpy as np
import pytest
import torch

import sweep_cases as SC
import sweep_ref as R

pytestmark = pytest.mark.gpu

vk = importlib.import_module("vickers-hardness-unet_amd")
SW = vk.sweep
F32 = np.float32
CURVE_FIELDS = ("stats", "per_image", "dice", "iou", "mean_dice", "mean_iou", "micro_stats", "precision", "recall", "f1", "micro_iou", "fpr",
                "ap", "auc", "best_dice", "best_iou", "best_f1", "best_mean")
GROUP_FIELDS = ("group_dice", "group_iou", "group_mean_dice", "group_mean_iou", "epoch_dice", "epoch_iou", "epoch_mean_dice", "epoch_mean_iou")


def dev():
    return torch.device("cuda:0")


def D(a, offset=0):
    """numpy -> device tensor; offset > 0 places the data that many elements into a fresh allocation, so its base pointer is
    off the 16-byte boundary every allocation starts on."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(dev())
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=dev())
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return view


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,)))[:, :got.ndim]
        at = tuple(bad[0])
        raise AssertionError("%s differs in %d bytes, first at %s: got %r want %r" % (what, len(bad), at, got[at], want[at]))


def check_curves(res, want, groups):
    h = res.cpu()
    for name in CURVE_FIELDS + (GROUP_FIELDS if groups else ()):
        same_bits(getattr(h, name), want[name], name)


# ------------------------------------------------------------------------------------------------ histogram vs numpy
@pytest.mark.parametrize("case", SC.HIST_CASES, ids=SC.HIST_IDS)
def test_hist_equals_numpy(case):
    thr, pred, tgt = SC.build_hist_case(case)
    want, want_bad = R.hist_ref(pred, tgt, thr, ignore_index=case.ignore)
    p, t = D(pred, case.offset), D(tgt, case.offset)
    hist, bad = SW.sweep_hist(p, t, thr, from_logits=False, ignore_index=case.ignore)
    same_bits(hist, want, "hist")
    assert int(bad.item()) == want_bad
    assert int(want.astype(np.int64).sum()) + want_bad + (int((tgt.astype(F32) == case.ignore).sum()) if case.ignore is not None else 0) == tgt.size


@pytest.mark.parametrize("dt", ["f32", "u8"])
@pytest.mark.parametrize("plane,cut", [(4096, 2048), (4096, 1000), (12289, 4097), (96 * 160, 96 * 160 - 16)])
def test_accumulate_over_two_pieces_equals_one_call(plane, cut, dt):
    """A plane fed in two pieces (slices along the last axis: read in place through the plane stride) adds up to the single call."""
    case = SC.HCase("acc_%d_%d_%s" % (plane, cut, dt), 2, 3, plane, 99, "default", "mix", "bad", dt, None, 0)
    thr, pred, tgt = SC.build_hist_case(case)
    p, t = D(pred), D(tgt)
    whole, bad_whole = SW.sweep_hist(p, t, thr, from_logits=False)
    part = SW.sweep_hist(p[..., :cut], t[..., :cut], thr, from_logits=False)
    first = part[0].clone()
    both = SW.sweep_hist(p[..., cut:], t[..., cut:], thr, from_logits=False, out=part)
    assert both[0].data_ptr() == part[0].data_ptr()
    same_bits(both[0], whole.cpu().numpy(), "accumulated hist")
    assert int(both[1].item()) == int(bad_whole.item()) > 0
    same_bits(first, R.hist_ref(pred[..., :cut], tgt[..., :cut], thr)[0], "first piece")
    same_bits(whole, R.hist_ref(pred, tgt, thr)[0], "whole")


def test_hist_is_reproducible_and_takes_image_shapes():
    case = SC.HCase("shapes", 3, 2, 40 * 24, 99, "default", "mix", "random", "f32", None, 0)
    thr, pred, tgt = SC.build_hist_case(case)
    p4, t4 = D(pred.reshape(3, 2, 40, 24)), D(tgt.reshape(3, 2, 40, 24))
    a, _ = SW.sweep_hist(p4, t4, from_logits=False)                     # the default grid
    b, _ = SW.sweep_hist(D(pred), D(tgt), thr, from_logits=False)
    same_bits(a, R.hist_ref(pred, tgt, thr)[0], "hist")
    assert torch.equal(a, b)
    one, _ = SW.sweep_hist(p4[1, 1], t4[1, 1], from_logits=False)       # [H, W]
    assert one.shape == (1, 1, 2, 100) and torch.equal(one[0, 0], a[1, 1])


# ------------------------------------------------------------------------------------------------ logits vs the single-threshold kernels
@pytest.mark.parametrize("c,K", [(1, 99), (3, 99), (1, 1024), (3, 1024)])
def test_logits_rows_equal_the_single_threshold_kernels(c, K):
    """Same expression on the same device: row k of the sweep holds the bits of vk_seg_metrics (C = 1) and of vk_seg_metrics_multi
    (multilabel) at threshold thr[k], for every k of the default grid and for 16 ks (ends included) of a 1024-threshold grid."""
    x, t = SC.logits_case(3, c, 64, 48, seed=100 + c + K)
    thr = SC.grid("default" if K == 99 else "uniform", K)
    ks = range(K) if K == 99 else sorted(set(np.linspace(0, K - 1, 16).astype(int).tolist()))
    xd, td = D(x), D(t)
    res = SW.threshold_sweep(xd, td, thr, from_logits=True)
    assert int(res.bad.item()) == 0
    h = res.cpu()
    ME = vk.multiclass_eval
    for k in ks:
        th = float(thr[k])
        tp, fp, fn, tn = (s.cpu() for s in ME.seg_stats(xd, td, "multilabel", threshold=th))
        assert torch.equal(h.stats[k], torch.stack([tp, fp, fn, tn])), k
        out = ME.seg_metrics_device(xd, td, "multilabel", threshold=th).cpu()
        assert out[0] == h.mean_dice[k] and out[1] == h.mean_iou[k], k
        assert torch.equal(out[2:2 + c], h.dice[k]) and torch.equal(out[2 + c:2 + 2 * c], h.iou[k]), k
        assert torch.equal(out[2 + 2 * c:].view(3, c, 2), h.per_image[k]), k
        if c == 1:
            one = vk.seg_metrics_device(xd, td, from_logits=True, threshold=th).cpu()
            assert one[0] == h.mean_dice[k] and one[1] == h.mean_iou[k], k
            assert torch.equal(one[2:].view(3, 2), h.per_image[k, :, 0]), k
    hist = SW.sweep_hist(xd, td, thr, from_logits=True)[0].cpu().numpy().astype(np.int64)
    assert hist.sum() == x.size and (hist[:, :, 1].sum(-1) == t.reshape(3, c, -1).sum(-1)).all()


def test_logits_uint8_target_and_ignore():
    x, t = SC.logits_case(2, 3, 32, 48, seed=7)
    t8 = t.astype(np.uint8)
    t8[:, :, :4] = SC.IGNORE
    tf = t8.astype(F32)
    a, bad_a = SW.sweep_hist(D(x), D(t8), ignore_index=SC.IGNORE)
    b, bad_b = SW.sweep_hist(D(x), D(tf), ignore_index=SC.IGNORE)
    assert torch.equal(a, b) and int(bad_a.item()) == int(bad_b.item()) == 0
    assert int(a.sum().item()) == x.size - int((t8 == SC.IGNORE).sum())
    c, bad_c = SW.sweep_hist(D(x), D(t8))                                 # without the ignore value the same elements are bad
    assert torch.equal(a, c) and int(bad_c.item()) == int((t8 == SC.IGNORE).sum())


# ------------------------------------------------------------------------------------------------ curves pass alone
@pytest.mark.parametrize("case", SC.CURVE_CASES, ids=SC.CURVE_IDS)
def test_curves_equal_numpy(case):
    hist, groups, G = SC.build_curve_case(case)
    want = R.curves_ref(hist, groups, G)
    thr = SC.grid("uniform", case.K)
    res = SW.sweep_curves(D(hist), thr, groups=None if groups is None else groups.tolist())
    assert res.n_groups == G
    check_curves(res, want, G > 0)
    if G:                                                                # the same from a device tensor of groups
        res2 = SW.sweep_curves(D(hist), thr, groups=D(groups), n_groups=G)
        check_curves(res2, want, True)


def test_curves_other_eps_and_groups_out_of_range():
    case = next(c for c in SC.CURVE_CASES if c.name == "N70_C3_K99_threegroups")
    hist, groups, G = SC.build_curve_case(case)
    thr = SC.grid("uniform", case.K)
    check_curves(SW.sweep_curves(D(hist), thr, groups=groups.tolist(), eps=1.0), R.curves_ref(hist, groups, G, eps=1.0), True)
    # images whose group is outside [0, G) belong to no batch: the other groups' rows are those of the listed images alone
    g2 = groups.copy()
    g2[[3, 17, 44]] = (-1, 3, 2 ** 30)
    res = SW.sweep_curves(D(hist), thr, groups=D(g2), n_groups=G)
    check_curves(res, R.curves_ref(hist, g2, G), True)


# ------------------------------------------------------------------------------------------------ ThresholdSweep
BATCHES = ((2, 32, 32), (3, 16, 48), (1, 40, 24))


def _epoch(seed, logits):
    rng = np.random.default_rng(seed)
    out = []
    for n, h, w in BATCHES:
        if logits:
            x, t = SC.logits_case(n, 1, h, w, seed=int(rng.integers(1 << 30)))
        else:
            x = rng.random((n, 1, h, w)).astype(F32)
            x.reshape(-1)[::7] = SW.DEFAULT_THRESHOLDS[rng.integers(0, 99, x.reshape(-1)[::7].size)]
            t = (rng.random((n, 1, h, w)) < 0.3).astype(F32)
        out.append((x, t))
    return out


def test_threshold_sweep_over_an_epoch_equals_numpy():
    """Three updates of different N and H x W: the result is the restatement over the concatenated per-image histograms, with the batch
    of every image as its group."""
    batches = _epoch(11, logits=False)
    sw = vk.ThresholdSweep(from_logits=False)
    for x, t in batches:
        sw.update(D(x), D(t))
    assert sw.n_images == 6 and sw.n_batches == 3
    thr = R.default_thresholds()
    hist = np.concatenate([R.hist_ref(x, t, thr)[0] for x, t in batches])
    groups = np.array([0, 0, 1, 1, 1, 2], np.int32)
    res = sw.compute(batch_mean=True)
    check_curves(res, R.curves_ref(hist, groups, 3), True)
    plain = sw.compute()
    assert plain.n_groups == 0 and plain.epoch_dice is None
    check_curves(plain, R.curves_ref(hist), False)
    # best(): the epoch curve when there are groups, the device's own index otherwise; ties to the lowest k
    want = R.curves_ref(hist, groups, 3)
    k = int(np.argmax(want["epoch_mean_dice"]))
    assert res.best("dice") == (float(thr[k]), float(want["epoch_mean_dice"][k]))
    k = int(want["best_mean"][1])
    assert plain.best("iou") == (float(thr[k]), float(want["mean_iou"][k]))
    k = int(want["best_f1"][0])
    assert plain.best("f1") == (float(thr[k]), float(want["f1"][k, 0]))
    # a second run gives identical bits
    sw2 = vk.ThresholdSweep(from_logits=False)
    for x, t in batches:
        sw2.update(D(x), D(t))
    again = sw2.compute(batch_mean=True).cpu()
    first = res.cpu()
    for name in CURVE_FIELDS + GROUP_FIELDS:
        assert getattr(again, name).numpy().tobytes() == getattr(first, name).numpy().tobytes(), name
    sw.reset()
    assert sw.n_images == 0 and sw.n_batches == 0
    with pytest.raises(ValueError):
        sw.compute()
    sw.update(D(batches[2][0]), D(batches[2][1]))
    check_curves(sw.compute(), R.curves_ref(hist[5:]), False)


def test_batch_mean_at_one_half_equals_the_mean_of_seg_metrics_calls():
    """The reference's validate (train.py:518-529): per-batch means, then the mean of those, in float64."""
    batches = _epoch(12, logits=True)
    sw = vk.ThresholdSweep()                                             # logits in, the default grid
    per_batch = []
    for x, t in batches:
        sw.update(D(x), D(t))
        per_batch.append(vk.seg_metrics_device(D(x), D(t), from_logits=True, threshold=0.5)[:2].cpu().numpy())
    res = sw.compute(batch_mean=True).cpu()
    k = int(np.nonzero(sw.thresholds == F32(0.5))[0][0])
    d = u = 0.0
    for m in per_batch:
        d += float(m[0])
        u += float(m[1])
    assert float(res.epoch_dice[k, 0]) == d / 3 and float(res.epoch_iou[k, 0]) == u / 3
    assert float(res.epoch_mean_dice[k]) == d / 3 and float(res.epoch_mean_iou[k]) == u / 3
    for g, m in enumerate(per_batch):
        assert float(res.group_dice[g, k, 0]) == float(m[0]) and float(res.group_iou[g, k, 0]) == float(m[1])


def test_best_raises_on_bad_targets():
    x = np.random.default_rng(3).random((2, 1, 16, 16)).astype(F32)
    t = np.zeros((2, 1, 16, 16), F32)
    t[0, 0, 0, :3] = 2.0
    res = vk.threshold_sweep(D(x), D(t), from_logits=False)
    assert int(res.bad.item()) == 3
    with pytest.raises(vk.VkError, match="3 value"):
        res.best()


# ------------------------------------------------------------------------------------------------ uint8 masks as PatchDataset keeps them
@pytest.mark.parametrize("shape", [(4, 1, 64, 64), (3, 1, 37, 53), (2, 2, 96, 160)])
def test_uint8_masks_give_the_float_copy_histogram(shape):
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 4).astype(F32)
    m8 = torch.from_numpy((rng.random(shape) < 0.04).astype(np.uint8)).to(dev())     # 0/1 masks, 1 byte per pixel, kept on the device
    xd = D(x)
    a, bad_a = SW.sweep_hist(xd, m8)
    b, bad_b = SW.sweep_hist(xd, m8.float())
    assert torch.equal(a, b) and int(bad_a.item()) == int(bad_b.item()) == 0
    assert int(a[:, :, 1].sum().item()) == int(m8.sum().item())
