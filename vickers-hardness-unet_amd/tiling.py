"""Sliding-window inference at the image's own resolution, with D4 test-time augmentation.

The letterbox entry points (``predict_mask``, ``Segmenter.infer``) shrink a micrograph into one img_size square; here the uint8 image
is cut into overlapping tiles on the device, every tile optionally in 2, 4 or 8 views (flips, transposition), the batches go through
the model, and the per-tile logits are blended back into one map of the original size::

    grid = vk.tiling.tile_grid(h, w, tile=512, overlap=64)
    x = vk.tiling.tile_preprocess(bgr, grid, "d4", device)              # [ntiles*8, 3, 512, 512]
    prob = vk.tiling.tile_blend(model(x), grid, "d4")                   # [C, h, w]
    prob = vk.Segmenter(model).infer_tiled(bgr, overlap=64, tta="d4")   # the same, in chunks of `batch` tiles

Two kernels (csrc/tiling.hip: vk_tile_preprocess, vk_tile_blend); no CPU fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib as L

TTA_VIEWS = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
BLEND_MODES = {"prob": L.VK_BLEND_PROB, "logit": L.VK_BLEND_LOGIT}


@dataclass(frozen=True)
class TileGrid:
    """Tiles of side ``tile`` over an h x w image: origins ``ys`` x ``xs``, tile index t = iy * nx + ix."""
    h: int
    w: int
    tile: int
    overlap: int
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]

    @property
    def ny(self) -> int:
        return len(self.ys)

    @property
    def nx(self) -> int:
        return len(self.xs)

    @property
    def ntiles(self) -> int:
        return len(self.ys) * len(self.xs)

    def origin(self, t: int) -> Tuple[int, int]:
        return self.ys[t // self.nx], self.xs[t % self.nx]


def axis_origins(length: int, tile: int, overlap: int) -> Tuple[int, ...]:
    """n = 1 if length <= tile else ceil((length - tile) / s) + 1 origins with s = tile - overlap, origin_i = min(i*s, max(length -
    tile, 0)): the last tile is pulled back flush with the edge, so padding exists only where length < tile."""
    s = tile - overlap
    n = 1 if length <= tile else -(-(length - tile) // s) + 1
    if n > L.VK_TILE_MAX_ORIGINS:
        raise ValueError("%d tile origins along an axis of %d pixels (tile %d, overlap %d): at most %d"
                         % (n, length, tile, overlap, L.VK_TILE_MAX_ORIGINS))
    last = max(length - tile, 0)
    return tuple(min(i * s, last) for i in range(n))


def tile_grid(h: int, w: int, tile: int = 512, overlap: int = 64) -> TileGrid:
    h, w, tile, overlap = int(h), int(w), int(tile), int(overlap)
    if h < 1 or w < 1:
        raise ValueError("image size %dx%d" % (h, w))
    if not 1 <= tile <= L.VK_TILE_MAX_SIDE:
        raise ValueError("tile %d outside 1..%d" % (tile, L.VK_TILE_MAX_SIDE))
    if not 0 <= 2 * overlap <= tile:
        raise ValueError("overlap %d outside 0..tile/2 (tile %d)" % (overlap, tile))
    return TileGrid(h, w, tile, overlap, axis_origins(h, tile, overlap), axis_origins(w, tile, overlap))


def view_map(v: int, T: int, i: int, j: int) -> Tuple[int, int]:
    """(i0, j0): the tile pixel that view v shows at (i, j)."""
    a, b = (j, i) if v & 4 else (i, j)
    return (T - 1 - a if v & 2 else a), (T - 1 - b if v & 1 else b)


def view_inverse(v: int, T: int, i0: int, j0: int) -> Tuple[int, int]:
    """(i, j): where view v shows the tile pixel (i0, j0)."""
    a = T - 1 - i0 if v & 2 else i0
    b = T - 1 - j0 if v & 1 else j0
    return (b, a) if v & 4 else (a, b)


def window_1d(T: int, overlap: int) -> torch.Tensor:
    """The blend ramp w1(t) = float(min(t+1, T-t, R)) / float(R) in fp32, R = overlap (1 when overlap is 0)."""
    R = overlap if overlap > 0 else 1
    t = torch.arange(T)
    return torch.minimum(torch.minimum(t + 1, T - t), torch.tensor(R)).float() / torch.tensor(float(R))


def _views(tta: str) -> Tuple[int, ...]:
    if tta not in TTA_VIEWS:
        raise ValueError("tta must be one of %s, got %r" % (sorted(TTA_VIEWS), tta))
    return TTA_VIEWS[tta]


def _desc(grid: TileGrid, tta: str, stride: int = 0, pad_value: int = 0, classes: int = 1) -> L.vk_tile_desc:
    d = L.vk_tile_desc()
    d.h, d.w, d.src_stride, d.T, d.overlap, d.ny, d.nx = grid.h, grid.w, stride, grid.tile, grid.overlap, grid.ny, grid.nx
    d.ys[:grid.ny] = grid.ys
    d.xs[:grid.nx] = grid.xs
    d.view_mask = sum(1 << v for v in _views(tta))
    d.pad_value, d.C = pad_value, classes
    return d


def tile_preprocess(img_bgr, grid: TileGrid, tta: str = "none", device=None, pad_value: int = 0) -> torch.Tensor:
    """uint8 BGR [h, w, 3] (numpy or tensor) -> float32 [ntiles*nviews, 3, T, T] on the device: tile major, view minor (ascending v),
    each normalised as ``preprocess`` does (the same bits); pixels outside the image are ``pad_value`` before the normalisation."""
    from .prepost import _as_device_u8
    device = torch.device(device if device is not None else "cuda")
    src = _as_device_u8(img_bgr, device)
    if (int(src.shape[0]), int(src.shape[1])) != (grid.h, grid.w):
        raise ValueError("image is %dx%d, the grid was made for %dx%d" % (src.shape[0], src.shape[1], grid.h, grid.w))
    nv = len(_views(tta))
    x = torch.empty(grid.ntiles * nv, 3, grid.tile, grid.tile, dtype=torch.float32, device=device)
    d = _desc(grid, tta, stride=3 * grid.w, pad_value=pad_value)
    L.check(L.lib().vk_tile_preprocess(C.byref(d), src.data_ptr(), x.data_ptr(), L.current_stream()), "vk_tile_preprocess")
    return x


def tile_blend(logits: torch.Tensor, grid: TileGrid, tta: str = "none", mode: str = "prob", thresh: Optional[float] = None, *,
               values: bool = True, out: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """logits [ntiles*nviews, C, T, T] (as ``tile_preprocess`` orders them) -> float32 [C, h, w] on the device: probabilities in [0, 1]
    (mode "prob": sigmoid per view, then the means) or blended raw logits (mode "logit": for multi-class models, whose softmax stays
    with the caller).  With ``thresh`` the uint8 {0,255} masks [C, h, w] come from the same pass: the return value is (map, masks), or
    the masks alone with ``values=False``.  ``out`` / ``mask``: contiguous tensors to write into."""
    if mode not in BLEND_MODES:
        raise ValueError("mode must be 'prob' or 'logit', got %r" % (mode,))
    nv = len(_views(tta))
    T = grid.tile
    if logits.dim() != 4 or logits.shape[0] != grid.ntiles * nv or tuple(logits.shape[2:]) != (T, T):
        raise ValueError("expected logits [%d, C, %d, %d], got %s" % (grid.ntiles * nv, T, T, tuple(logits.shape)))
    if not logits.is_cuda:
        raise L.VkError("logits are on %s: this package runs on an MI355X only and has no CPU fallback" % logits.device)
    lg = logits.detach().contiguous().float()
    nc = int(lg.shape[1])
    shape = (nc, grid.h, grid.w)
    if thresh is None and not values:
        raise ValueError("nothing to compute: values=False needs a thresh")
    if values and out is None:
        out = torch.empty(shape, dtype=torch.float32, device=lg.device)
    if thresh is not None and mask is None:
        mask = torch.empty(shape, dtype=torch.uint8, device=lg.device)
    for t, dt in ((out, torch.float32), (mask, torch.uint8)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != lg.device):
            raise ValueError("out / mask must be contiguous %s tensors on the logits' device" % (shape,))
    d = _desc(grid, tta, classes=nc)
    L.check(L.lib().vk_tile_blend(C.byref(d), BLEND_MODES[mode], lg.data_ptr(), float(thresh if thresh is not None else 0.5),
                                  L.ptr(out if values else None), L.ptr(mask if thresh is not None else None), L.current_stream()),
            "vk_tile_blend")
    if thresh is None:
        return out
    return (out, mask) if values else mask


def run_tiled(model, img_bgr, tile: int, overlap: int = 64, tta: str = "none", blend: str = "prob", batch: int = 16,
              thresh: Optional[float] = None, values: bool = True, device=None, pad_value: int = 0):
    """tile_preprocess -> model in chunks of ``batch`` -> tile_blend.  Every chunk has exactly ``batch`` tiles (the last one is filled
    with zero tiles whose logits are dropped), so the model builds one eval plan and no tile takes another route through the
    convolution kernels than its neighbours."""
    if batch < 1:
        raise ValueError("batch must be positive")
    device = torch.device(device if device is not None else "cuda")
    h, w = int(img_bgr.shape[0]), int(img_bgr.shape[1])
    grid = tile_grid(h, w, tile, overlap)
    with torch.no_grad():
        x = tile_preprocess(img_bgr, grid, tta, device, pad_value)
        n = int(x.shape[0])
        logits = None
        for i in range(0, n, batch):
            chunk = x[i:i + batch]
            k = int(chunk.shape[0])
            if k < batch:
                chunk = torch.cat([chunk, x.new_zeros(batch - k, *x.shape[1:])])
            lg = model(chunk)
            if logits is None:
                logits = torch.empty(n, lg.shape[1], tile, tile, dtype=torch.float32, device=device)
            logits[i:i + k] = lg[:k]
        return tile_blend(logits, grid, tta, blend, thresh, values=values)
