"""Unet(classes=C), the parts that need no GPU: the engine's tensor table and buckets on host-only handles, the refusal of classes
outside 1..16, the default initialisation against OracleUnet(classes=C), and the float64 loss restatement the GPU tests use against
torch autograd of the smp formulas."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as R


def _handle(vk, classes, training=1, dtype=None):
    L = vk.lib()
    cfg = vk._lib.vk_unet_config(2, 64, vk._lib.VK_BF16 if dtype is None else dtype, training)
    h = C.c_void_p()
    rc = L.vk_unet_create_ex(C.byref(cfg), classes, C.byref(h))
    return L, h, rc


def _table(vk, L, h):
    out = []
    for i in range(L.vk_unet_num_tensors(h)):
        ti = vk._lib.vk_tensor_info()
        vk._lib.check(L.vk_unet_tensor_info(h, i, C.byref(ti)))
        out.append((ti.name.decode(), ti.kind, [ti.dims[j] for j in range(ti.ndim)], ti.offset, ti.numel))
    return out


@pytest.mark.parametrize("classes", [2, 3, 16])
def test_tensor_table_and_buckets(vk, classes):
    L, h1, rc = _handle(vk, 1)
    assert rc == 0
    L, hc, rc = _handle(vk, classes)
    assert rc == 0
    try:
        assert L.vk_unet_num_classes(hc) == classes and L.vk_unet_num_classes(h1) == 1
        t1, tc = _table(vk, L, h1), _table(vk, L, hc)
        assert sum(1 for t in tc if t[1] in (0, 1)) == 140
        assert [t[0] for t in t1] == [t[0] for t in tc]
        for a, b in zip(t1, tc):                   # everything before the head keeps its place
            if not a[0].startswith("segmentation_head."):
                assert a == b
        w = next(t for t in tc if t[0] == "segmentation_head.0.weight")
        b = next(t for t in tc if t[0] == "segmentation_head.0.bias")
        w1 = next(t for t in t1 if t[0] == "segmentation_head.0.weight")
        assert w[2] == [classes, 16, 3, 3] and w[4] == 144 * classes and w[3] == w1[3]
        assert b[2] == [classes] and b[4] == classes and b[3] == w[3] + 144 * classes
        P = L.vk_unet_param_numel(hc)
        assert b[3] + classes <= P and max(t[3] + t[4] for t in tc if t[1] in (0, 1)) == b[3] + classes
        # gradient buckets: contiguous, cover [0, P), the head in bucket 0
        rng = []
        for i in range(L.vk_unet_num_buckets(hc)):
            b0, b1 = C.c_int64(), C.c_int64()
            vk._lib.check(L.vk_unet_bucket_range(hc, i, C.byref(b0), C.byref(b1)))
            rng.append((b0.value, b1.value))
        assert rng[0][1] == P and rng[0][0] <= w[3]
        s = sorted(rng)
        assert s[0][0] == 0 and s[-1][1] == P and all(s[i][1] == s[i + 1][0] for i in range(len(s) - 1))
        assert L.vk_unet_workspace_bytes(hc) > L.vk_unet_workspace_bytes(h1)
    finally:
        L.vk_unet_destroy(h1)
        L.vk_unet_destroy(hc)


def test_classes_one_is_the_binary_plan(vk):
    L = vk.lib()
    for training in (0, 1):
        cfg = vk._lib.vk_unet_config(2, 64, vk._lib.VK_BF16, training)
        a, b = C.c_void_p(), C.c_void_p()
        vk._lib.check(L.vk_unet_create(C.byref(cfg), C.byref(a)))
        vk._lib.check(L.vk_unet_create_ex(C.byref(cfg), 1, C.byref(b)))
        try:
            assert _table(vk, L, a) == _table(vk, L, b)
            assert L.vk_unet_workspace_bytes(a) == L.vk_unet_workspace_bytes(b)
            assert L.vk_unet_param_numel(a) == L.vk_unet_param_numel(b)
        finally:
            L.vk_unet_destroy(a)
            L.vk_unet_destroy(b)


@pytest.mark.parametrize("classes", [0, 17, -1])
def test_classes_out_of_range_refused(vk, classes):
    L, h, rc = _handle(vk, classes)
    assert rc == -1 and not h.value
    assert b"classes" in L.vk_last_error_string()
    with pytest.raises(NotImplementedError, match="classes"):
        vk.multiclass.Unet(encoder_weights=None, classes=classes)


@pytest.mark.parametrize("classes", [2, 3, 16])
def test_default_init_reproduces_oracle(vk, oracle, classes):
    oracle.set_seed(42)
    ref = oracle.OracleUnet(classes=classes)
    oracle.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=classes)
    so, sg = ref.state_dict(), m.state_dict()
    assert list(so.keys()) == list(sg.keys())
    for k in so:
        assert so[k].shape == sg[k].shape, k
        assert torch.equal(so[k], sg[k]), k
    assert sg["segmentation_head.0.weight"].shape == (classes, 16, 3, 3)
    assert len(list(m.parameters())) == 140


def test_constructor_rejects_what_is_not_implemented(vk):
    with pytest.raises(vk.VkError):
        vk.Unet(encoder_weights="imagenet")          # needs a download
    with pytest.raises(NotImplementedError):
        vk.Unet(encoder_name="resnet50", encoder_weights=None)
    with pytest.raises(NotImplementedError):
        vk.multiclass.Unet(encoder_weights=None, classes=17)
    with pytest.raises(NotImplementedError):
        vk.Unet(encoder_weights=None, in_channels=1)
    with pytest.raises(NotImplementedError):
        vk.multiclass.DiceLoss(mode="multiclass", ignore_index=255)


def test_top_level_names_stay_binary(vk):
    """vk.Unet / vk.DiceLoss / vk.BCEDiceLoss are the reference's binary drop-ins; the wider contract is vk.multiclass."""
    with pytest.raises(NotImplementedError, match="vk.multiclass.Unet"):
        vk.Unet(encoder_weights=None, classes=3)
    for mode in ("multilabel", "multiclass"):
        with pytest.raises(NotImplementedError, match="vk.multiclass.DiceLoss"):
            vk.DiceLoss(mode=mode)
    with pytest.raises(NotImplementedError):
        vk.BCEDiceLoss(mode="multilabel")
    assert issubclass(vk.multiclass.Unet, vk.Unet) and issubclass(vk.multiclass.DiceLoss, vk.DiceLoss)
    assert vk.multiclass.Unet(encoder_weights=None).classes == 1


def test_multi_loss_modes_accepted_and_others_refused(vk):
    for mode in ("binary", "multilabel", "multiclass"):
        assert vk.multiclass.DiceLoss(mode=mode).mode == mode
    vk.multiclass.CEDiceLoss()
    vk.multiclass.BCEDiceLoss(mode="multilabel")
    for kw in (dict(mode="multiclass", classes=[0]), dict(mode="multiclass", ignore_index=0), dict(mode="multilabel", log_loss=True),
               dict(mode="multilabel", smooth=1.0), dict(mode="other")):
        with pytest.raises(NotImplementedError):
            vk.multiclass.DiceLoss(**kw)


# ---- the float64 restatement against torch autograd of the smp formulas
def _smp_dice(p, onehot):
    N, Cc = p.shape[:2]
    p, onehot = p.reshape(N, Cc, -1), onehot.reshape(N, Cc, -1)
    inter = (p * onehot).sum(dim=(0, 2))
    card = (p + onehot).sum(dim=(0, 2))
    score = (2.0 * inter) / card.clamp_min(1e-7)
    loss = (1.0 - score) * (onehot.sum(dim=(0, 2)) > 0).to(p.dtype)
    return loss.mean()


def _batch(Cc, seed, empty_class=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, Cc, 8, 12, generator=g, dtype=torch.float64) * 2
    y = (torch.rand(2, Cc, 8, 12, generator=g) > 0.6).double()
    t = torch.randint(0, Cc, (2, 8, 12), generator=g)
    if empty_class:
        y[:, -1] = 0
        t[t == Cc - 1] = 0
    return x, y, t


@pytest.mark.parametrize("Cc", [2, 3, 5])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.5, 2.0)])
def test_multilabel_restatement_matches_autograd(Cc, weights):
    x, y, _ = _batch(Cc, 7 + Cc)
    xr = x.clone().requires_grad_(True)
    bce = F.binary_cross_entropy_with_logits(xr, y)
    dice = _smp_dice(F.logsigmoid(xr).exp(), y)
    loss = weights[0] * bce + weights[1] * dice
    loss.backward()
    tot, b, d, dl = R.multilabel(x, y, *weights)
    assert torch.allclose(tot, loss.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(b, bce.detach(), rtol=1e-12) and torch.allclose(d, dice.detach(), rtol=1e-12)
    assert torch.allclose(dl, xr.grad, rtol=1e-10, atol=1e-15)


@pytest.mark.parametrize("Cc", [2, 3, 5])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.5, 2.0)])
def test_multiclass_restatement_matches_autograd(Cc, weights):
    x, _, t = _batch(Cc, 11 + Cc)
    xr = x.clone().requires_grad_(True)
    ce = F.cross_entropy(xr, t)
    onehot = F.one_hot(t, Cc).permute(0, 3, 1, 2).double()
    dice = _smp_dice(xr.log_softmax(dim=1).exp(), onehot)
    loss = weights[0] * ce + weights[1] * dice
    loss.backward()
    tot, c, d, dl = R.multiclass(x, t, *weights)
    assert torch.allclose(tot, loss.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(c, ce.detach(), rtol=1e-12) and torch.allclose(d, dice.detach(), rtol=1e-12)
    assert torch.allclose(dl, xr.grad, rtol=1e-10, atol=1e-15)


def test_one_class_multilabel_is_binary(oracle):
    x, y, _ = _batch(1, 3, empty_class=False)
    tot, _, _, dl = R.multilabel(x, y)
    xr = x.clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(xr, y) + oracle.DiceLoss(mode="binary")(xr, y)
    loss.backward()
    assert torch.allclose(tot, loss.detach(), rtol=1e-12)
    assert torch.allclose(dl, xr.grad, rtol=1e-10, atol=1e-15)
