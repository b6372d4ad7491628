"""Native-resolution patch training on the device: the training-side half of ``vk.tiling``.

``Segmenter.infer_tiled`` runs the model on 512 x 512 windows of a micrograph at its own resolution; ``DeviceDataset`` letterboxes every
image to 512 x 512 first, so a model trained on it has seen a 3072 x 2048 micrograph six times smaller than tiled inference shows it.
``PatchDataset`` keeps the images on the device at their own size and cuts random S x S patches out of them every step:

    DeviceDataset.batch(indices, sampler)          PatchDataset.batch(indices, sampler)     -> x [n,3,S,S], y [n,1,S,S], names
    AugmentSampler                                  PatchSampler (wraps an AugmentSampler)

* foreground-aware: with probability ``p_fg`` the window is placed so that a uniformly chosen foreground pixel of the item lands at a
  uniformly chosen place in it (mean foreground is 4.4 % of an image: a uniformly placed window is usually empty);
* rotated and zoomed in the SOURCE image: the reference's ``Rotate(limit=180, p=0.6)`` fires with its own probability, but where real
  pixels exist around the window, so the corners of the patch are not blanked;
* no CPU in the loop: ``vk_patch_batch`` (origins kernel + crop kernel) fills the uint8 patch buffers, ``vk_augment_batch`` reads them
  as its dataset (D4, photometric transforms, noise, Normalize) — the draws are made on the host, exactly as ``AugmentSampler`` makes them.

No CPU fallback: without libvkunet.so and an MI355X these raise."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .augment import IDENTITY, PHOTO_CLAHE, AugmentSampler, _params_array, color_tables

MAX_SIDE = 16384
ZOOM_MIN, ZOOM_MAX = 0.25, 4.0
PATCH_IDENTITY = dict(item=0, k=-1, oy=0, ox=0, zoom=1.0, cos_a=1.0, sin_a=0.0)


class PatchSampler:
    """The per-sample draws of patch training, made on the host.  ``p_fg`` and the ``zoom`` range (source pixels per output pixel,
    log-uniform) are parameters, not measurements.  ``aug``: the ``AugmentSampler`` whose draws are used; its rotation is moved into
    the patch draw (applied in the source image), everything else stays with ``vk_augment_batch``."""

    def __init__(self, seed: Optional[int] = None, p_fg: float = 0.7, zoom: Tuple[float, float] = (0.8, 1.25),
                 aug: Optional[AugmentSampler] = None):
        if not 0.0 <= p_fg <= 1.0:
            raise ValueError("p_fg must be in [0, 1]")
        lo, hi = float(zoom[0]), float(zoom[1])
        if not ZOOM_MIN <= lo <= hi <= ZOOM_MAX:
            raise ValueError(f"zoom range must satisfy {ZOOM_MIN} <= lo <= hi <= {ZOOM_MAX}")
        self.p_fg, self.zoom = float(p_fg), (lo, hi)
        self.aug = aug if aug is not None else AugmentSampler(seed)
        self.rng = np.random.default_rng(None if seed is None else [int(seed), 0x7061])      # a stream of its own, beside aug's

    def sample(self, item: int, h: int, w: int, fg_count: int, S: int) -> Tuple[dict, dict]:
        """(patch, aug): ``patch`` has the keys of ``vk_patch_params``, ``aug`` those of ``vk_aug_params`` with ``rotate = 0``."""
        r = self.rng
        aug = self.aug.sample()
        patch = dict(PATCH_IDENTITY, item=int(item))
        if aug["rotate"]:
            patch["cos_a"], patch["sin_a"] = aug["cos_a"], aug["sin_a"]
            aug["rotate"], aug["cos_a"], aug["sin_a"] = 0, 1.0, 0.0
        if r.random() < self.p_fg and fg_count > 0:
            patch["k"] = int(r.integers(fg_count))
            patch["oy"], patch["ox"] = int(r.integers(S)), int(r.integers(S))
        else:
            patch["oy"], patch["ox"] = int(r.integers(max(h - S, 0) + 1)), int(r.integers(max(w - S, 0) + 1))
        lo, hi = self.zoom
        patch["zoom"] = min(max(math.exp(float(r.uniform(math.log(lo), math.log(hi)))), lo), hi)
        return patch, aug


def _patch_array(draws: Sequence[dict]):
    arr = (L.vk_patch_params * len(draws))()
    for i, d in enumerate(draws):
        arr[i] = L.vk_patch_params(int(d["item"]), int(d["k"]), int(d["oy"]), int(d["ox"]), float(d["zoom"]), float(d["cos_a"]),
                                   float(d["sin_a"]), 0)
    return arr


class PatchDataset:
    """All (image, mask) pairs resident on the device at their own size: uint8 BGR in one ragged store (every item starts on a
    multiple of 4 bytes), masks binarised ``(m > 0)`` in a second one, an item table and the foreground row index beside them."""

    def __init__(self, images_bgr: Sequence[np.ndarray], masks: Sequence[np.ndarray], patch_size: int = 512, device=None,
                 names: Optional[Sequence[str]] = None):
        if len(images_bgr) != len(masks) or not len(images_bgr):
            raise ValueError("need one mask per image")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise L.VkError("PatchDataset lives on the MI355X; there is no CPU path")
        self.S = int(patch_size)
        if not 1 <= self.S <= MAX_SIDE:
            raise ValueError(f"patch_size must be in 1..{MAX_SIDE}")
        self.names = list(names) if names is not None else [str(i) for i in range(len(images_bgr))]
        pairs = []
        self.items = (L.vk_patch_item * len(images_bgr))()
        io = mo = ro = 0
        for i, (im, mk) in enumerate(zip(images_bgr, masks)):
            im = np.ascontiguousarray(im)
            mk = np.ascontiguousarray(mk[:, :, 0] if mk.ndim == 3 else mk)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or mk.dtype != np.uint8 or mk.shape != im.shape[:2]:
                raise ValueError(f"item {i}: expected uint8 BGR [h, w, 3] and uint8 mask [h, w]")
            h, w = im.shape[:2]
            if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
                raise ValueError(f"item {i}: sides must be in 1..{MAX_SIDE}, got {h} x {w}")
            self.items[i] = L.vk_patch_item(io, mo, h, w, ro)
            pairs.append((im, mk))
            io += (h * w * 3 + 3) & ~3
            mo += (h * w + 3) & ~3
            ro += h
        self.shapes = [(int(it.h), int(it.w)) for it in self.items]
        self.images = torch.empty(io, dtype=torch.uint8, device=self.device)
        self.masks = torch.empty(mo, dtype=torch.uint8, device=self.device)
        self.rowcum = torch.empty(ro, dtype=torch.int32, device=self.device)
        self._items_dev = torch.empty(len(pairs) * C.sizeof(L.vk_patch_item), dtype=torch.uint8, device=self.device)
        for it, (im, mk) in zip(self.items, pairs):
            h, w = it.h, it.w
            self.images[it.img_off:it.img_off + h * w * 3].copy_(torch.from_numpy(im).view(-1))
            self.masks[it.msk_off:it.msk_off + h * w].copy_(torch.from_numpy((mk > 0).astype(np.uint8)).view(-1))
        L.check(L.lib().vk_patch_index(len(pairs), self.items, self._items_dev.data_ptr(), self.images.numel(), self.masks.data_ptr(),
                                       self.masks.numel(), self.rowcum.data_ptr(), self.rowcum.numel(), L.current_stream()),
                "vk_patch_index")
        last = torch.tensor([it.row_off + it.h - 1 for it in self.items], dtype=torch.int64, device=self.device)
        self.fg_counts = [int(v) for v in self.rowcum[last].cpu().tolist()]       # the one synchronisation, at construction
        self.last_origins = None
        self._cap = 0
        self._tables = torch.from_numpy(color_tables()).to(self.device)
        self._clahe_ws = None

    def __len__(self) -> int:
        return len(self.items)

    def image(self, i: int) -> torch.Tensor:
        """Item ``i`` as a device view of the store, uint8 BGR [h, w, 3] (no copy): what ``Segmenter.infer_tiled`` / ``run_tiled`` take."""
        it = self.items[i]
        return self.images[it.img_off:it.img_off + it.h * it.w * 3].view(it.h, it.w, 3)

    def mask(self, i: int) -> torch.Tensor:
        """The mask of item ``i`` as float32 [1, 1, h, w] on the device: the target ``vk.seg_metrics`` takes."""
        it = self.items[i]
        return self.masks[it.msk_off:it.msk_off + it.h * it.w].view(1, 1, it.h, it.w).float()

    def rowcum_of(self, i: int) -> torch.Tensor:
        it = self.items[i]
        return self.rowcum[it.row_off:it.row_off + it.h]

    def centred(self, item: int) -> dict:
        """The draw of the validation pipeline: one window centred on the item, no transform."""
        h, w = self.shapes[item]
        return dict(PATCH_IDENTITY, item=int(item), oy=max((h - self.S) // 2, 0), ox=max((w - self.S) // 2, 0))

    def _reserve(self, n: int) -> None:
        if n <= self._cap:
            return
        cap, S = max(n, 32), self.S
        self._rgb = torch.empty(cap, S, S, 3, dtype=torch.uint8, device=self.device)
        self._msk = torch.empty(cap, S, S, dtype=torch.uint8, device=self.device)
        self._origins = torch.empty(cap, 2, dtype=torch.int32, device=self.device)
        self._pp_dev = torch.empty(cap * C.sizeof(L.vk_patch_params), dtype=torch.uint8, device=self.device)
        self._ap_dev = torch.empty(cap * C.sizeof(L.vk_aug_params), dtype=torch.uint8, device=self.device)
        self._arange = torch.arange(cap, dtype=torch.int32, device=self.device)
        self._cap = cap

    def crop(self, patch_draws: Sequence[dict], force_general: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``vk_patch_batch`` alone: (uint8 RGB [n,S,S,3], mask {0,1} [n,S,S], origins int32 [n,2]) — views of buffers the dataset owns
        and reuses with the next call."""
        n = len(patch_draws)
        if n < 1:
            raise ValueError("need at least one draw")
        for d in patch_draws:
            if not 0 <= int(d["item"]) < len(self):
                raise ValueError(f"item {d['item']} outside 0..{len(self) - 1}")
        self._reserve(n)
        L.check(L.lib().vk_patch_batch(n, self.S, len(self), self._items_dev.data_ptr(), self.images.data_ptr(), self.masks.data_ptr(),
                                       self.rowcum.data_ptr(), _patch_array(patch_draws), self._pp_dev.data_ptr(),
                                       L.VK_PATCH_FORCE_GENERAL if force_general else 0, self._origins.data_ptr(), self._rgb.data_ptr(),
                                       self._msk.data_ptr(), L.current_stream()),
                "vk_patch_batch")
        self.last_origins = self._origins[:n]
        return self._rgb[:n], self._msk[:n], self.last_origins

    def batch(self, indices: Sequence[int], sampler: Optional[PatchSampler] = None,
              draws: Optional[Sequence[Tuple[dict, dict]]] = None) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
        """One stream at a time: the patch buffers, the parameter scratch and the CLAHE workspace of the dataset are reused by every
        call, so batches requested on different streams must be ordered by the caller (consecutive calls on one stream are).

        ``(x float32 [n,3,S,S], y float32 [n,1,S,S], names)``, one patch per index.  ``sampler=None`` and ``draws=None``: one centred
        window per item, no transform.  ``draws``: explicit ``(patch, aug)`` dict pairs (tests); the patch dict's item is set from
        ``indices``.  The origins of the call stay in ``last_origins`` (a device tensor).  No host synchronisation."""
        idx = [int(i) for i in indices]
        n, S = len(idx), self.S
        for i in idx:
            if not 0 <= i < len(self):
                raise ValueError(f"index {i} outside 0..{len(self) - 1}")
        if draws is None:
            if sampler is not None:
                draws = [sampler.sample(i, *self.shapes[i], self.fg_counts[i], S) for i in idx]
            else:
                draws = [(self.centred(i), IDENTITY) for i in idx]
        if len(draws) != n:
            raise ValueError("one (patch, aug) pair of draws per index")
        rgb, msk, _ = self.crop([dict(p, item=i) for i, (p, _) in zip(idx, draws)])
        aug = [a for _, a in draws]
        x = torch.empty(n, 3, S, S, dtype=torch.float32, device=self.device)
        y = torch.empty(n, 1, S, S, dtype=torch.float32, device=self.device)
        ws_ptr, ws_bytes = None, 0
        if any(int(d["photo"]) == PHOTO_CLAHE for d in aug):
            ws_bytes = int(L.lib().vk_augment_workspace_bytes(n, S))
            if self._clahe_ws is None or self._clahe_ws.numel() < ws_bytes:
                self._clahe_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            ws_ptr = self._clahe_ws.data_ptr()
        L.check(L.lib().vk_augment_batch(n, S, n, rgb.data_ptr(), msk.data_ptr(), self._arange.data_ptr(), _params_array(aug, S),
                                         self._ap_dev.data_ptr(), self._tables.data_ptr(), ws_ptr, ws_bytes, x.data_ptr(), y.data_ptr(),
                                         L.current_stream()),
                "vk_augment_batch")
        return x, y, [self.names[i] for i in idx]

    def loader(self, batch_size: int, patches_per_image: int = 1, shuffle: bool = True, sampler: Optional[PatchSampler] = None,
               seed: Optional[int] = None):
        """Iterate ``(x, y, names)``; one epoch is ``patches_per_image`` visits of every item."""
        if batch_size < 1 or patches_per_image < 1:
            raise ValueError("batch_size and patches_per_image must be positive")
        rng = np.random.default_rng(seed)
        visits = []
        for _ in range(patches_per_image):
            order = np.arange(len(self))
            if shuffle:
                rng.shuffle(order)
            visits.append(order)
        order = np.concatenate(visits)
        for b in range(0, len(order), batch_size):
            yield self.batch(order[b:b + batch_size].tolist(), sampler)
