"""Instance copy-paste augmentation on the device (Ghiasi et al., CVPR 2021): a compose step between the uint8 store of
``DeviceDataset`` and ``vk_augment_batch``.

Everything downstream of the model measures several indentations per micrograph; nine training images in ten hold one.  ``CopyPaste``
pastes indentations of other items into the base image before the usual augmentation, so the network sees neighbours:

    DeviceDataset.batch(indices, sampler)           CopyPaste(dataset).batch(indices, sampler, cp_sampler=...)   -> x, y, names
    AugmentSampler                                  AugmentSampler + CopyPasteSampler

* ``InstanceBank``: once per dataset — ``vk.instances.detect_gt`` over the masks, ``vk_cp_boxes`` (box and area of every component),
  ``vk_cp_alpha`` (a kept map and a feathered alpha map, resident as uint8), one read-back of the boxes; then the host records and the
  donor rule.
* ``CopyPasteSampler``: the draws, on the host, in a fixed order, as ``AugmentSampler`` makes them.
* ``CopyPaste``: ``vk_cp_paste`` into two uint8 scratch buffers, which ``vk_augment_batch`` reads with index 0..n-1 — the hand-off
  ``PatchDataset.batch`` uses.  ``PatchDataset`` itself (ragged native-resolution stores) is out of scope: this stage composes the
  letterboxed S x S items only.

What copy-paste is worth on the object metrics (``vk.ObjectMetrics``) with a trained model is unmeasured.  No CPU fallback: without
libvkunet.so and an MI355X the device entry points raise; the sampler and the donor rule are host code."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .augment import IDENTITY, PHOTO_CLAHE, AugmentSampler, DeviceDataset, _params_array

MAX_PASTES = L.VK_CP_MAX_PASTES
MAX_SLOTS = L.VK_CP_MAX_SLOTS
MAX_SIDE = L.VK_CP_MAX_SIDE
REC_FIELDS = L.CP_REC_FIELDS
RECORD_DTYPE = np.dtype([(f, "<i4") for f in ("item", "slot", "x0", "y0", "x1", "y1", "area", "donor")])
CHUNK = 64                                   # items per detect_gt call of the bank build


def default_min_area(S: int) -> int:
    """The area filter of the geometry post-processing (``vk.geometry.detect``): max(200, int(0.0008 S S))."""
    return max(200, int(0.0008 * S * S))


def bank_records(boxes: np.ndarray, counts: np.ndarray, content: np.ndarray, S: int, max_components: int = 16, margin: int = 4,
                 min_area: Optional[int] = None) -> np.ndarray:
    """The host half of the bank: ``boxes`` int32 [n, M, 5] (``vk_cp_boxes``), ``counts`` [n] and ``content`` [n, 4] = (top, left, nh,
    nw) -> ``RECORD_DTYPE`` rows, one per component, item then slot ascending.  The box of a row is the component's box grown by
    ``margin`` and clipped to the item's content rectangle.  A row is a donor iff its item holds at most ``max_components`` components,
    its area is at least ``min_area`` and its grown box meets no other grown box of the item — so every kept pixel inside a donor box
    belongs to that instance, and (``margin`` >= 3) so does every non-zero alpha."""
    boxes = np.asarray(boxes, np.int64)
    if boxes.ndim != 3 or boxes.shape[2] != 5 or len(counts) != boxes.shape[0] or np.shape(content) != (boxes.shape[0], 4):
        raise ValueError("expected boxes [n, M, 5], counts [n] and content [n, 4]")
    if margin < 0 or max_components < 1:
        raise ValueError("margin must be >= 0 and max_components >= 1")
    if min_area is None:
        min_area = default_min_area(S)
    rows = []
    for i in range(boxes.shape[0]):
        used = min(max(int(counts[i]), 0), boxes.shape[1])
        if not used:
            continue
        top, left, nh, nw = (int(v) for v in content[i])
        b = boxes[i, :used]
        x0, y0 = np.maximum(b[:, 0] - margin, left), np.maximum(b[:, 1] - margin, top)
        x1, y1 = np.minimum(b[:, 2] + margin, left + nw - 1), np.minimum(b[:, 3] + margin, top + nh - 1)
        meet = (x0[:, None] <= x1[None, :]) & (x0[None, :] <= x1[:, None]) & (y0[:, None] <= y1[None, :]) & (y0[None, :] <= y1[:, None])
        np.fill_diagonal(meet, False)
        donor = (int(counts[i]) <= max_components) & (b[:, 4] >= min_area) & ~meet.any(axis=1)
        part = np.zeros(used, RECORD_DTYPE)
        part["item"], part["slot"] = i, np.arange(used)
        part["x0"], part["y0"], part["x1"], part["y1"], part["area"], part["donor"] = x0, y0, x1, y1, b[:, 4], donor
        rows.append(part)
    return np.concatenate(rows) if rows else np.zeros(0, RECORD_DTYPE)


class InstanceBank:
    """The instances of a ``DeviceDataset`` that can be pasted.  ``kept`` and ``alpha``: uint8 [n, S, S] on the device; ``boxes`` int32
    [n, 256, 5] and ``counts`` [n] on the host; ``records`` (``RECORD_DTYPE``); ``content`` int32 [n, 4]; ``donors``: the rows of
    ``records`` with ``donor`` set.  ``from_host`` builds the host half alone (no device): what the sampler needs."""

    def __init__(self, dataset: DeviceDataset, max_components: int = 16, margin: int = 4, min_area: Optional[int] = None):
        from . import instances
        if not isinstance(dataset, DeviceDataset):
            raise ValueError("InstanceBank takes a DeviceDataset (PatchDataset is out of scope)")
        n, S = len(dataset), dataset.S
        if not 1 <= S <= MAX_SIDE:
            raise ValueError(f"img_size {S} outside 1..{MAX_SIDE}")
        dev = dataset.device
        self.kept = torch.empty(n, S, S, dtype=torch.uint8, device=dev)
        self.alpha = torch.empty(n, S, S, dtype=torch.uint8, device=dev)
        boxes = torch.empty(n, MAX_SLOTS, 5, dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        lib, st = L.lib(), L.current_stream()
        for a in range(0, n, CHUNK):
            b = min(a + CHUNK, n)
            dets = instances.detect_gt(dataset.masks[a:b], max_components=MAX_SLOTS)
            L.check(lib.vk_cp_boxes(b - a, S, S, dets.slots.data_ptr(), MAX_SLOTS, boxes[a:b].data_ptr(), st), "vk_cp_boxes")
            L.check(lib.vk_cp_alpha(b - a, S, S, dets.slots.data_ptr(), self.kept[a:b].data_ptr(), self.alpha[a:b].data_ptr(), st), "vk_cp_alpha")
            counts[a:b] = dets.counts
        self._host(S, boxes.cpu().numpy(), counts.cpu().numpy(), dataset.content, max_components, margin, min_area)     # the one read-back

    def _host(self, S, boxes, counts, content, max_components, margin, min_area):
        self.S, self.boxes, self.counts = int(S), boxes, np.asarray(counts, np.int32)
        self.content = np.ascontiguousarray(content, dtype=np.int32)
        self.max_components, self.margin = int(max_components), int(margin)
        self.min_area = default_min_area(self.S) if min_area is None else int(min_area)
        self.records = bank_records(boxes, self.counts, self.content, self.S, self.max_components, self.margin, self.min_area)
        self.donors = self.records[self.records["donor"] != 0]
        self._by_item = {int(i): self.records[self.records["item"] == i] for i in np.unique(self.records["item"])}

    @classmethod
    def from_host(cls, S: int, boxes: np.ndarray, counts, content, max_components: int = 16, margin: int = 4,
                  min_area: Optional[int] = None) -> "InstanceBank":
        bank = cls.__new__(cls)
        bank.kept = bank.alpha = None
        bank._host(S, np.asarray(boxes, np.int32), counts, content, max_components, margin, min_area)
        return bank

    def __len__(self) -> int:
        return int(self.content.shape[0])

    def boxes_of(self, item: int) -> np.ndarray:
        """The records of one item's components."""
        return self._by_item.get(int(item), self.records[:0])


def _meets(a, b, gap: int) -> bool:
    """Box ``a`` grown by ``gap`` shares a pixel with box ``b`` (inclusive x0, y0, x1, y1)."""
    return a[0] - gap <= b[2] and b[0] <= a[2] + gap and a[1] - gap <= b[3] and b[1] <= a[3] + gap


class CopyPasteSampler:
    """The draws of copy-paste, made on the host in a fixed order: with probability ``p`` a number of pastes uniform in
    1..``max_pastes``; per paste a donor uniform over the bank's donors, ``d4`` uniform in 0..7, a scale log-uniform in ``scale``, then
    an origin uniform over the places where the box lies inside the base item's content rectangle (none: the paste is dropped),
    redrawn at most ``tries`` times while the box grown by ``gap`` meets a box of the base item or an accepted paste (then dropped).
    ``p``, ``max_pastes``, ``scale``, ``gap`` and ``tries`` are parameters, not measurements."""

    def __init__(self, bank: InstanceBank, seed: Optional[int] = None, p: float = 0.5, max_pastes: int = 3,
                 scale: Tuple[float, float] = (0.5, 1.25), gap: int = 2, tries: int = 10):
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must be in [0, 1]")
        if not 1 <= int(max_pastes) <= MAX_PASTES:
            raise ValueError(f"max_pastes must be in 1..{MAX_PASTES}")
        lo, hi = float(scale[0]), float(scale[1])
        if not 0.0 < lo <= hi <= 2.0:
            raise ValueError("scale range must satisfy 0 < lo <= hi <= 2")
        if gap < 0 or tries < 1:
            raise ValueError("gap must be >= 0 and tries >= 1")
        self.bank, self.p, self.max_pastes, self.scale, self.gap, self.tries = bank, float(p), int(max_pastes), (lo, hi), int(gap), int(tries)
        self.rng = np.random.default_rng(None if seed is None else [int(seed), 0x6370])       # a stream of its own, beside AugmentSampler's

    def sample(self, base_item: int) -> List[dict]:
        """The record dicts (keys of ``vk_cp_rec``) of one sample whose base is ``base_item``."""
        r, bank = self.rng, self.bank
        if not 0 <= int(base_item) < len(bank):
            raise ValueError(f"base item {base_item} outside 0..{len(bank) - 1}")
        if not r.random() < self.p or not len(bank.donors):
            return []
        k = int(r.integers(1, self.max_pastes + 1))
        top, left, nh, nw = (int(v) for v in bank.content[int(base_item)])
        taken = [(int(b["x0"]), int(b["y0"]), int(b["x1"]), int(b["y1"])) for b in bank.boxes_of(base_item)]
        lo, hi = self.scale
        out = []
        for _ in range(k):
            d = bank.donors[int(r.integers(len(bank.donors)))]
            d4 = int(r.integers(8))
            s = min(max(math.exp(float(r.uniform(math.log(lo), math.log(hi)))), lo), hi)
            sw, sh = int(d["x1"]) - int(d["x0"]) + 1, int(d["y1"]) - int(d["y0"]) + 1
            tw, th = (sh, sw) if d4 & 1 else (sw, sh)
            dw, dh = max(1, int(math.floor(tw * s + 0.5))), max(1, int(math.floor(th * s + 0.5)))
            if dw > nw or dh > nh or dw > 2 * bank.S or dh > 2 * bank.S:
                continue
            for _ in range(self.tries):
                x, y = left + int(r.integers(nw - dw + 1)), top + int(r.integers(nh - dh + 1))
                box = (x, y, x + dw - 1, y + dh - 1)
                if not any(_meets(box, t, self.gap) for t in taken):
                    taken.append(box)
                    out.append(dict(donor=int(d["item"]), sx0=int(d["x0"]), sy0=int(d["y0"]), sw=sw, sh=sh, d4=d4, dx0=x, dy0=y, dw=dw, dh=dh))
                    break
        return out


def _recs_array(pastes: Sequence[Sequence[dict]]):
    n = len(pastes)
    counts = (C.c_int32 * n)()
    recs = (L.vk_cp_rec * (n * MAX_PASTES))()
    for k, lst in enumerate(pastes):
        if len(lst) > MAX_PASTES:
            raise ValueError(f"sample {k}: {len(lst)} pastes, at most {MAX_PASTES}")
        counts[k] = len(lst)
        for j, d in enumerate(lst):
            recs[k * MAX_PASTES + j] = L.vk_cp_rec(*(int(d[f]) for f in REC_FIELDS))
    return counts, recs


class CopyPaste:
    """``DeviceDataset`` with the compose step in front of ``vk_augment_batch``.  The composed buffers, the parameter scratch and the
    CLAHE workspace are reused by every call: one stream at a time, as ``DeviceDataset.batch`` documents."""

    def __init__(self, dataset: DeviceDataset, bank: Optional[InstanceBank] = None):
        if not isinstance(dataset, DeviceDataset):
            raise ValueError("CopyPaste takes a DeviceDataset (PatchDataset is out of scope)")
        self.dataset, self.bank = dataset, bank if bank is not None else InstanceBank(dataset)
        if self.bank.kept is None or tuple(self.bank.kept.shape) != tuple(dataset.masks.shape):
            raise ValueError("the bank was not built on this dataset's device store")
        self.device, self.S, self.names = dataset.device, dataset.S, dataset.names
        self._cap = 0
        self._clahe_ws = None

    def __len__(self) -> int:
        return len(self.dataset)

    def _reserve(self, n: int) -> None:
        if n <= self._cap:
            return
        cap, S = max(n, 32), self.S
        self._rgb = torch.empty(cap, S, S, 3, dtype=torch.uint8, device=self.device)
        self._msk = torch.empty(cap, S, S, dtype=torch.uint8, device=self.device)
        self._recs_dev = torch.empty(L.vk_cp_recs_dev_bytes(cap) // 4, dtype=torch.int32, device=self.device)
        self._ap_dev = torch.empty(cap * C.sizeof(L.vk_aug_params), dtype=torch.uint8, device=self.device)
        self._arange = torch.arange(cap, dtype=torch.int32, device=self.device)
        self._cap = cap

    def compose(self, indices: Sequence[int], pastes: Sequence[Sequence[dict]]) -> Tuple[torch.Tensor, torch.Tensor]:
        """``vk_cp_paste`` alone: (uint8 RGB [n,S,S,3], mask {0,1} [n,S,S]) — views of buffers this object owns and reuses with the next
        call.  ``pastes[k]``: the record dicts of sample k, applied in list order; an empty list copies the base.  No host
        synchronisation."""
        idx = [int(i) for i in indices]
        n, ds = len(idx), self.dataset
        if n < 1 or len(pastes) != n:
            raise ValueError("need at least one index and one list of pastes per index")
        for i in idx:
            if not 0 <= i < len(ds):
                raise ValueError(f"index {i} outside 0..{len(ds) - 1}")
        counts, recs = _recs_array(pastes)
        self._reserve(n)
        base = torch.tensor(idx, dtype=torch.int32, device=self.device)
        L.check(L.lib().vk_cp_paste(n, self.S, len(ds), ds.images.data_ptr(), ds.masks.data_ptr(), self.bank.kept.data_ptr(),
                                    self.bank.alpha.data_ptr(), base.data_ptr(), counts, recs, self._recs_dev.data_ptr(),
                                    self._rgb.data_ptr(), self._msk.data_ptr(), L.current_stream()),
                "vk_cp_paste")
        return self._rgb[:n], self._msk[:n]

    def batch(self, indices: Sequence[int], sampler: Optional[AugmentSampler] = None, draws: Optional[Sequence[dict]] = None,
              cp_sampler: Optional[CopyPasteSampler] = None, pastes: Optional[Sequence[Sequence[dict]]] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
        """``(x float32 [n,3,S,S], y float32 [n,1,S,S], names)``: ``compose`` followed by ``vk_augment_batch`` over the composed buffers.
        ``sampler`` / ``draws`` as ``DeviceDataset.batch`` takes them; ``cp_sampler`` draws the pastes, ``pastes`` gives them (tests);
        neither: no pastes, the batch ``DeviceDataset.batch`` returns.  One stream at a time."""
        idx = [int(i) for i in indices]
        n, S = len(idx), self.S
        if pastes is None:
            pastes = [cp_sampler.sample(i) if cp_sampler is not None else [] for i in idx]
        if draws is None:
            draws = [sampler.sample() if sampler is not None else IDENTITY for _ in idx]
        if len(draws) != n:
            raise ValueError("one set of draws per index")
        rgb, msk = self.compose(idx, pastes)
        x = torch.empty(n, 3, S, S, dtype=torch.float32, device=self.device)
        y = torch.empty(n, 1, S, S, dtype=torch.float32, device=self.device)
        ws_ptr, ws_bytes = None, 0
        if any(int(d["photo"]) == PHOTO_CLAHE for d in draws):
            ws_bytes = int(L.lib().vk_augment_workspace_bytes(n, S))
            if self._clahe_ws is None or self._clahe_ws.numel() < ws_bytes:
                self._clahe_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            ws_ptr = self._clahe_ws.data_ptr()
        L.check(L.lib().vk_augment_batch(n, S, n, rgb.data_ptr(), msk.data_ptr(), self._arange.data_ptr(), _params_array(draws, S),
                                         self._ap_dev.data_ptr(), self.dataset._tables.data_ptr(), ws_ptr, ws_bytes, x.data_ptr(),
                                         y.data_ptr(), L.current_stream()),
                "vk_augment_batch")
        return x, y, [self.names[i] for i in idx]

    def loader(self, batch_size: int, shuffle: bool = True, sampler: Optional[AugmentSampler] = None,
               cp_sampler: Optional[CopyPasteSampler] = None, seed: Optional[int] = None):
        """Iterate ``(x, y, names)`` over one epoch, as ``DeviceDataset.loader`` does."""
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        order = np.arange(len(self))
        if shuffle:
            np.random.default_rng(seed).shuffle(order)
        for b in range(0, len(order), batch_size):
            yield self.batch(order[b:b + batch_size].tolist(), sampler, cp_sampler=cp_sampler)
