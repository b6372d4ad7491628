"""vk.multiclass validation metrics and post-processing, the parts that need no GPU: the numpy restatement (tests/multiclass_eval_ref.py)
against independent formulations, the C ABI's argument checks (all on the host, nothing is launched) and the Python wrappers'
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_eval_ref as R
from oracle import prepost_oracle as P


def _onehot_counts(x, t, mode, thr=0.5, from_logits=True):
    """tp, fp, fn, tn as one-hot products and sums in torch float64 (bad labels are not used here)."""
    x = torch.as_tensor(x, dtype=torch.float64)
    N, Cc = x.shape[:2]
    if mode == "multilabel":
        p = torch.sigmoid(x) if from_logits else x
        pred = (p > thr).double()
        tgt = torch.as_tensor(t, dtype=torch.float64)
    else:
        pred = F.one_hot(x.argmax(dim=1), Cc).movedim(-1, 1).double()
        tgt = F.one_hot(torch.as_tensor(t), Cc).movedim(-1, 1).double()
    dims = tuple(range(2, x.dim()))
    tp = (pred * tgt).sum(dims)
    fp = (pred * (1 - tgt)).sum(dims)
    fn = ((1 - pred) * tgt).sum(dims)
    tn = ((1 - pred) * (1 - tgt)).sum(dims)
    return [v.long().numpy() for v in (tp, fp, fn, tn)]


def _logits(rng, shape):
    x = (rng.normal(size=shape) * 3).round(2).astype(np.float32)      # away from the threshold by at least 0.01 ...
    x.reshape(-1)[::13] = 0.0                                          # ... except exact zeros: sigmoid(0) = 0.5, not > 0.5
    return x


@pytest.mark.parametrize("C", [1, 2, 3, 7, 16])
def test_multilabel_counts_match_onehot_products(C):
    rng = np.random.default_rng(C)
    x = _logits(rng, (3, C, 9, 11))
    t = (rng.random((3, C, 9, 11)) < 0.3).astype(np.float32)
    (tp, fp, fn, tn), bad = R.counts(x, t, "multilabel")
    want = _onehot_counts(x, t, "multilabel")
    assert bad == 0
    for got, w in zip((tp, fp, fn, tn), want):
        assert np.array_equal(got, w)
    assert (tp + fp + fn + tn == 99).all()
    # probabilities in, compared directly; values exactly at the threshold are not foreground
    p = rng.random((3, C, 9, 11)).astype(np.float32)
    p.reshape(-1)[::7] = 0.5
    (tp, fp, fn, tn), _ = R.counts(p, t, "multilabel", 0.5, from_logits=False)
    for got, w in zip((tp, fp, fn, tn), _onehot_counts(p, t, "multilabel", 0.5, False)):
        assert np.array_equal(got, w)


@pytest.mark.parametrize("C", [2, 3, 7, 16])
def test_multiclass_counts_match_onehot_products_with_ties(C):
    rng = np.random.default_rng(10 + C)
    x = _logits(rng, (4, C, 8, 13))
    x[:, :, ::3, ::2] = 1.5                            # every class ties: argmax is class 0
    x[:, C - 1, 1::4, :] = x[:, 0, 1::4, :]            # last and first class tie
    t = rng.integers(0, C, (4, 8, 13))
    (tp, fp, fn, tn), bad = R.counts(x, t, "multiclass")
    assert bad == 0
    for got, w in zip((tp, fp, fn, tn), _onehot_counts(x, t, "multiclass")):
        assert np.array_equal(got, w)
    assert np.array_equal(np.argmax(x, axis=1), torch.as_tensor(x).argmax(dim=1).numpy())     # ties: torch's first maximum
    assert ((tp + fn).sum(1) == 104).all() and ((tp + fp).sum(1) == 104).all()


def test_bad_labels_are_skipped_and_counted():
    rng = np.random.default_rng(5)
    x = _logits(rng, (2, 3, 6, 6))
    t = rng.integers(0, 3, (2, 6, 6))
    t[0, 0, :3] = [-1, 3, 255]
    (tp, fp, fn, tn), bad = R.counts(x, t, "multiclass")
    assert bad == 3
    assert (tp + fp + fn + tn)[0].tolist() == [33] * 3 and (tp + fp + fn + tn)[1].tolist() == [36] * 3
    tl = (rng.random((2, 3, 6, 6)) < 0.5).astype(np.float32)
    tl[1, 2, 0, 0] = 0.5
    (tp, fp, fn, tn), bad = R.counts(x, tl, "multilabel")
    assert bad == 1 and (tp + fp + fn + tn)[1, 2] == 35 and (tp + fp + fn + tn)[1, 1] == 36


def test_scores_with_one_class_equal_the_reference_formulas():
    """train.py:230-281 restated in torch fp32 (dice_coef / iou_coef per image), against the restatement's per-image scores (exact)
    and batch means (fp64 here, fp32 .mean() there: within 1e-6)."""
    rng = np.random.default_rng(3)
    prob = torch.from_numpy(rng.random((70, 1, 16, 16)).astype(np.float32))
    target = torch.from_numpy((rng.random((70, 1, 16, 16)) < 0.2).astype(np.float32))
    target[5] = 0
    prob[5] = 0.1                                      # empty prediction and target: scores 1
    pred = (prob > 0.5).float()
    inter = (pred * target).sum(dim=(1, 2, 3))
    union = pred.sum(dim=(1, 2, 3)) + target.sum(dim=(1, 2, 3))
    eps = 1e-7
    dice_ref = (2 * inter + eps) / (union + eps)
    iou_ref = (inter + eps) / (union - inter + eps)
    (tp, fp, fn, _), _ = R.counts(prob.numpy(), target.numpy(), "multilabel", 0.5, from_logits=False)
    out = R.scores(tp, fp, fn)
    per = out[4:].reshape(70, 1, 2)
    assert np.array_equal(per[:, 0, 0], dice_ref.numpy()) and np.array_equal(per[:, 0, 1], iou_ref.numpy())
    assert per[5, 0, 0] == 1.0 and per[5, 0, 1] == 1.0
    assert abs(out[0] - dice_ref.mean().item()) < 1e-6 and abs(out[1] - iou_ref.mean().item()) < 1e-6
    assert out[0] == out[2] and out[1] == out[3]


@pytest.mark.parametrize("conv", ["pad_br", "centered", "train"])
@pytest.mark.parametrize("h,w", [(300, 400), (512, 512), (37, 700), (1001, 333)])
def test_postprocess_restatement_with_one_class_is_the_oracle(h, w, conv):
    rng = np.random.default_rng(h + w)
    lg = (rng.normal(size=(1, 64, 64)) * 3).astype(np.float32)
    geo = P.GEOMETRY[conv](h, w, 64)
    assert np.array_equal(R.postprocess_masks(lg, *geo[1:], (h, w))[0], P.postprocess_mask(lg[0], *geo[1:], (h, w)))
    assert np.array_equal(R.postprocess_probs(lg, *geo[1:], (h, w), "multilabel")[0], P.postprocess_prob(lg[0], *geo[1:], (h, w)))
    lg3 = (rng.normal(size=(3, 64, 64)) * 3).astype(np.float32)
    lab = R.postprocess_labels(lg3, *geo[1:], (h, w))
    assert lab.shape == (h, w) and lab.dtype == np.uint8 and lab.max() <= 2
    pr = R.postprocess_probs(lg3, *geo[1:], (h, w), "multiclass")
    assert pr.shape == (3, h, w) and np.abs(pr.sum(0) - 1).max() < 1e-5


def test_c_abi_argument_errors(vk):
    """Every refusal happens on the host before anything is launched (no GPU here: a launch would fail differently)."""
    L = vk.lib()
    ML, MC = vk._lib.VK_LOSS_MULTILABEL, vk._lib.VK_LOSS_MULTICLASS
    fake = C.c_void_p(1 << 20)                         # never dereferenced: the checks reject the call first
    ws = L.vk_seg_metrics_multi_workspace_bytes(2, 3)
    assert ws == 2 * 3 * 4 * 8 and L.vk_seg_metrics_multi_workspace_bytes(0, 3) == 0

    def metrics(mode=ML, n=2, c=3, per=64, logits=fake, target=fake, wsb=ws, out=fake, bad=fake, wsp=fake):
        return L.vk_seg_metrics_multi(mode, n, c, per, logits, target, 1, 0.5, 1e-7, wsp, wsb, None, out, bad, None)

    cases = [(dict(c=0), b"outside [1, 16]"), (dict(c=17), b"outside [1, 16]"), (dict(mode=MC, c=1), b"multiclass needs C >= 2"),
             (dict(mode=0), b"neither multilabel"), (dict(n=0), b"n_images"), (dict(per=0), b"per_image"),
             (dict(logits=None), b"null buffer"), (dict(target=None), b"null buffer"), (dict(out=None), b"null buffer"),
             (dict(bad=None), b"null buffer"), (dict(wsp=None), b"null buffer"), (dict(wsb=ws - 1), b"workspace too small")]
    for kw, msg in cases:
        assert metrics(**kw) < 0, kw
        assert msg in L.vk_last_error_string(), (kw, L.vk_last_error_string())
    lb = vk._lib.vk_letterbox_desc
    ok, bad_fit = lb(10, 10, 0, 64, 10, 10, 0, 0, 0), lb(10, 10, 0, 64, 10, 10, 60, 0, 0)     # top + nh > S
    for fn, extra in ((L.vk_letterbox_postprocess_labels, ()), (L.vk_letterbox_postprocess_mask_multi, (0.5,))):
        args = lambda d, c, lg, o: (C.byref(d), c, lg) + extra + (o, None)        # noqa: E731
        assert fn(*args(bad_fit, 3, fake, fake)) < 0 and b"does not fit" in L.vk_last_error_string()
        assert fn(*args(ok, 0, fake, fake)) < 0 and b"outside [1, 16]" in L.vk_last_error_string()
        assert fn(*args(ok, 17, fake, fake)) < 0
        assert fn(*args(ok, 3, None, fake)) < 0 and b"null buffer" in L.vk_last_error_string()
        assert fn(*args(ok, 3, fake, None)) < 0
        assert fn(None, 3, fake, *extra, fake, None) < 0
    pm = L.vk_letterbox_postprocess_prob_multi
    assert pm(C.byref(bad_fit), 3, ML, fake, fake, None) < 0 and b"does not fit" in L.vk_last_error_string()
    assert pm(C.byref(ok), 1, MC, fake, fake, None) < 0 and b"multiclass needs C >= 2" in L.vk_last_error_string()
    assert pm(C.byref(ok), 3, 0, fake, fake, None) < 0
    assert pm(C.byref(ok), 17, ML, fake, fake, None) < 0
    assert pm(C.byref(ok), 3, ML, None, fake, None) < 0 and b"null buffer" in L.vk_last_error_string()


def test_python_refuses_cpu_tensors_and_bad_shapes(vk):
    M = vk.multiclass
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(vk.VkError, match="CUDA"):
        M.seg_metrics(x, torch.zeros(2, 8, 8, dtype=torch.long), "multiclass")
    with pytest.raises(vk.VkError, match="CUDA"):
        M.seg_stats(x, torch.zeros_like(x), "multilabel")
    with pytest.raises(vk.VkError, match="CUDA"):
        M.postprocess_probs(x[0], (1.0, (1.0, 8, 8, 0, 0), (8, 8)), "multiclass")
    # shapes and modes are checked first, on any device
    xd = x
    d = x.device
    with pytest.raises(ValueError, match="mode"):
        M.seg_metrics(xd, torch.zeros_like(xd), "binary")
    with pytest.raises(ValueError, match="C >= 2"):
        M.seg_metrics(xd[:, :1], torch.zeros(2, 8, 8, dtype=torch.long, device=d), "multiclass")
    with pytest.raises(ValueError, match="N, H, W"):
        M.seg_metrics(xd, torch.zeros(2, 1, 8, 8, dtype=torch.long, device=d), "multiclass")
    with pytest.raises(ValueError, match="integer"):
        M.seg_metrics(xd, torch.zeros(2, 8, 8, device=d), "multiclass")
    with pytest.raises(ValueError, match="shape"):
        M.seg_metrics(xd, torch.zeros(2, 3, 8, 7, device=d), "multilabel")
    with pytest.raises(ValueError, match="C <= 16"):
        M.seg_metrics(torch.zeros(1, 17, 4, 4, device=d), torch.zeros(1, 17, 4, 4, device=d), "multilabel")
    with pytest.raises(ValueError, match="square"):
        M.postprocess_labels(torch.zeros(3, 8, 9, device=d), (1.0, (1.0, 8, 8, 0, 0), (8, 8)))
