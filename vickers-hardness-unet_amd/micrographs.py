"""Synthetic indentation micrographs rendered on the device: images whose masks and diagonals are known exactly.

The package measures a diagonal through letterbox, U-Net, geometry, ``vk.subpix``, ``vk.zoom`` and ``vk.instances``, and no test can read
the dataset.  ``vk_mg_render`` draws a scene — a polished surface with scratches along one direction, a streaky texture, vignetting, dust,
and up to eight four-facet pyramids with ridge lines and a halo, blurred, with sensor noise and the camera's burnt-in overlays — into the
uint8 slot ``vk.copypaste`` composes into: pixels [n, S, S, 3] in the store's channel order and a {0, 1} mask [n, S, S], which
``vk_augment_batch`` reads.

    SceneSampler(seed).sample()            one scene record (``SCENE_DTYPE``, the layout of ``vk_mg_scene``), drawn on the host
    render(scenes, size)                   -> (rgb, mask) on the device
    truth(scene)                           -> the exact vertices, diagonals, area and box of every indentation
    MicrographDataset(length, size, seed)  item i is the scene of ``default_rng([seed, i])``; ``batch`` / ``loader`` as ``DeviceDataset``

All arithmetic of the renderer is integer (geometry in 1/16 pixel); tests/micrographs_ref.py restates it and the kernel gives its bytes.
Numbers measured on these scenes are numbers on synthetic scenes: nothing here says that training on them transfers to real micrographs.
No CPU fallback: without libvkunet.so and an MI355X ``render`` raises; the sampler and ``truth`` are host code."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .augment import IDENTITY, PHOTO_CLAHE, AugmentSampler, _params_array, color_tables

MAX_INDENTS, MAX_SCRATCHES, MAX_BLOBS, MAX_RECTS = L.VK_MG_MAX_INDENTS, L.VK_MG_MAX_SCRATCHES, L.VK_MG_MAX_BLOBS, L.VK_MG_MAX_RECTS
MIN_SIDE, MAX_SIDE, COORD_MARGIN = L.VK_MG_MIN_SIDE, L.VK_MG_MAX_SIDE, L.VK_MG_COORD_MARGIN
SCENE_DTYPE = np.dtype(L.vk_mg_scene)
INDENT_DTYPE, SCRATCH_DTYPE, BLOB_DTYPE, RECT_DTYPE = (np.dtype(t) for t in (L.vk_mg_indent, L.vk_mg_scratch, L.vk_mg_blob, L.vk_mg_rect))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
assert SCENE_DTYPE.itemsize == C.sizeof(L.vk_mg_scene) == 3200


def blank_scene(base: int = 128, tint: Sequence[int] = (256, 256, 256)) -> np.ndarray:
    """A scene without records, gradient, vignette, texture, blur or noise: the constant ``(base tint + 128) >> 8``."""
    s = np.zeros((), SCENE_DTYPE)
    s["base"], s["tint"], s["tex_cos"] = base, tint, 16384
    return s


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def quad_ok(vx: Sequence[int], vy: Sequence[int], ax: int, ay: int) -> bool:
    """Convex and clockwise (x to the right, y down), with the apex strictly inside: what ``vk_mg_render`` admits."""
    vx, vy = [int(v) for v in vx], [int(v) for v in vy]
    for i in range(4):
        j, k = (i + 1) & 3, (i + 2) & 3
        if _cross(vx[j] - vx[i], vy[j] - vy[i], vx[k] - vx[j], vy[k] - vy[j]) <= 0:
            return False
        if _cross(vx[j] - vx[i], vy[j] - vy[i], int(ax) - vx[i], int(ay) - vy[i]) <= 0:
            return False
    return True


def _fx(v: float) -> int:
    return int(math.floor(16.0 * v + 0.5))


class SceneSampler:
    """The host draws of one scene, in a fixed order (every draw is made whether or not its value ends up used):

    1. ``random()`` < ``p_empty``: no indentation; then ``integers(1, max_indents + 1)``: their number.
    2. Per indentation, at most ``tries`` times, one ``random(15)``: centre (2), half diagonal, asymmetry of the second one
       (``+-asym``), rotation in [0, pi / 2), vertex jitter (8, ``+-jitter`` of the half diagonal), apex offset (2, ``+-apex``).  Redrawn
       until the quadrilateral is convex, its vertices lie ``margin`` pixels inside the frame and its box grown by ``gap`` pixels meets
       no box before it; dropped after ``tries``.
    3. Per scene, one ``random(16)``: light direction, shade level, contrast, specular, background level, tint (3), gradient (2),
       vignette (3), scratch direction, texture amplitude, blur; then ``integers(2 ** 32, size=2)``: texture and noise seeds;
       ``integers(3, 10)``: noise amplitude; per indentation one ``random(8)``: facet slopes (4), ridge level and half width, halo radius
       and depth.
    4. ``integers(scratches[0], scratches[1] + 1)`` scratches, one ``random(8)`` each: point (2), deviation from the scratch direction,
       stray, half width, depth, finite, length.  ``integers(0, max_blobs + 1)`` blobs, one ``random(4)`` each.  One ``random(6)`` for the
       overlays: a red outline rectangle and a scale-bar box, each with probability ``p_overlay``.
    The ranges are parameters, not measurements."""

    def __init__(self, seed: Optional[int] = None, size: int = 512, max_indents: int = 3, p_empty: float = 0.0,
                 half_diag: Tuple[float, float] = (0.04, 0.14), asym: float = 0.04, jitter: float = 0.02, apex: float = 0.08,
                 margin: int = 6, gap: int = 6, tries: int = 20, scratches: Tuple[int, int] = (8, 40), max_blobs: int = 4,
                 p_specular: float = 0.15, p_overlay: float = 0.15):
        if not MIN_SIDE <= int(size) <= MAX_SIDE:
            raise ValueError(f"size {size} outside {MIN_SIDE}..{MAX_SIDE}")
        if not 1 <= int(max_indents) <= MAX_INDENTS:
            raise ValueError(f"max_indents must be in 1..{MAX_INDENTS}")
        if not 0.0 <= p_empty <= 1.0 or not 0.0 <= p_specular <= 1.0 or not 0.0 <= p_overlay <= 1.0:
            raise ValueError("probabilities must be in [0, 1]")
        lo, hi = float(half_diag[0]), float(half_diag[1])
        if not 0.0 < lo <= hi <= 0.35:
            raise ValueError("half_diag must satisfy 0 < lo <= hi <= 0.35 (fractions of the side)")
        if not 0 <= int(scratches[0]) <= int(scratches[1]) <= MAX_SCRATCHES:
            raise ValueError(f"scratches must satisfy 0 <= lo <= hi <= {MAX_SCRATCHES}")
        if not 0 <= int(max_blobs) <= MAX_BLOBS:
            raise ValueError(f"max_blobs must be in 0..{MAX_BLOBS}")
        if margin < 0 or gap < 0 or tries < 1 or not 0.0 <= asym < 0.5 or not 0.0 <= jitter < 0.2 or not 0.0 <= apex < 0.3:
            raise ValueError("margin, gap >= 0, tries >= 1, asym < 0.5, jitter < 0.2, apex < 0.3")
        self.S, self.max_indents, self.p_empty, self.half_diag = int(size), int(max_indents), float(p_empty), (lo, hi)
        self.asym, self.jitter, self.apex, self.margin, self.gap, self.tries = float(asym), float(jitter), float(apex), int(margin), int(gap), int(tries)
        self.scratches, self.max_blobs, self.p_specular, self.p_overlay = (int(scratches[0]), int(scratches[1])), int(max_blobs), float(p_specular), float(p_overlay)
        self.rng = np.random.default_rng(None if seed is None else [int(seed), 0x6D67])

    def _indent(self, u: np.ndarray, boxes: List[tuple]):
        S, (lo, hi) = self.S, self.half_diag
        h1 = (lo + (hi - lo) * u[2]) * S
        h2 = h1 * (1.0 + self.asym * (2.0 * u[3] - 1.0))
        reach = max(h1, h2) * (1.0 + self.jitter) + self.margin + 1
        if 2 * reach >= S - 1:
            return None
        cx, cy = reach + (S - 1 - 2 * reach) * u[0], reach + (S - 1 - 2 * reach) * u[1]
        a = 0.5 * math.pi * u[4]
        c, s = math.cos(a), math.sin(a)
        j = self.jitter * h1 * (2.0 * u[5:13] - 1.0)
        pts = [(cx + h1 * c, cy + h1 * s), (cx - h2 * s, cy + h2 * c), (cx - h1 * c, cy - h1 * s), (cx + h2 * s, cy - h2 * c)]
        vx = [_fx(p[0] + j[2 * i]) for i, p in enumerate(pts)]
        vy = [_fx(p[1] + j[2 * i + 1]) for i, p in enumerate(pts)]
        ax, ay = _fx(cx + self.apex * h1 * (2.0 * u[13] - 1.0)), _fx(cy + self.apex * h1 * (2.0 * u[14] - 1.0))
        if not quad_ok(vx, vy, ax, ay):
            return None
        m = 16 * self.margin
        if min(vx) < m or min(vy) < m or max(vx) > 16 * (S - 1) - m or max(vy) > 16 * (S - 1) - m:
            return None
        box = (min(vx), min(vy), max(vx), max(vy))
        g = 16 * self.gap
        for b in boxes:
            if box[0] - g <= b[2] and b[0] <= box[2] + g and box[1] - g <= b[3] and b[1] <= box[3] + g:
                return None
        return vx, vy, ax, ay, box, h1

    def sample(self, rng: Optional[np.random.Generator] = None) -> np.ndarray:
        """One scene (a 0-d ``SCENE_DTYPE`` array) from this sampler's generator, or from ``rng``."""
        r, S = self.rng if rng is None else rng, self.S
        sc = blank_scene()
        empty = r.random() < self.p_empty
        k = int(r.integers(1, self.max_indents + 1))
        boxes, halves = [], []
        for _ in range(0 if empty else k):
            for _ in range(self.tries):
                got = self._indent(r.random(15), boxes)
                if got is not None:
                    vx, vy, ax, ay, box, h1 = got
                    q = sc["indents"][len(boxes)]
                    q["vx"], q["vy"], q["ax"], q["ay"] = vx, vy, ax, ay
                    boxes.append(box)
                    halves.append(h1)
                    break
        sc["n_indents"] = len(boxes)
        u = r.random(16)
        light = 2.0 * math.pi * u[0]
        level, contrast = 70.0 + 40.0 * u[1], 30.0 + 30.0 * u[2]
        sc["base"] = int(140 + 50 * u[4])
        sc["tint"] = [int(256 + 32 * (u[5 + c] - 0.5)) for c in range(3)]
        sc["grad_x"], sc["grad_y"] = int(24 * (u[8] - 0.5)), int(24 * (u[9] - 0.5))
        sc["grad_cx"] = sc["grad_cy"] = S // 2
        sc["vig_cx"], sc["vig_cy"] = int(S * (0.4 + 0.2 * u[10])), int(S * (0.4 + 0.2 * u[11]))
        sc["vig"] = min(255, int((4 + 16 * u[12]) * (512.0 / S) ** 2))
        theta = math.pi * u[13]
        sc["tex_cos"], sc["tex_sin"] = int(round(16384 * math.cos(theta))), int(round(16384 * math.sin(theta)))
        sc["tex_amp"], sc["tex_lu"], sc["tex_lv"] = int(10 + 20 * u[14]), 5, 1
        sc["blur_r"] = min(3, 1 + int(3 * u[15]))
        seeds = r.integers(2 ** 32, size=2, dtype=np.uint64)
        sc["tex_seed"], sc["noise_seed"] = int(seeds[0]), int(seeds[1])
        sc["noise_amp"] = int(r.integers(3, 10))
        for i in range(len(boxes)):
            w = r.random(8)
            q = sc["indents"][i]
            vx, vy = q["vx"].astype(np.float64), q["vy"].astype(np.float64)
            lit = []
            for f in range(4):
                g = (f + 1) & 3
                nx, ny = 0.5 * (vx[f] + vx[g]) - float(q["ax"]), 0.5 * (vy[f] + vy[g]) - float(q["ay"])
                lit.append((nx * math.cos(light) + ny * math.sin(light)) / max(math.hypot(nx, ny), 1.0))
            shade = [int(level + contrast * v) for v in lit]
            if u[3] < self.p_specular:
                shade[int(np.argmax(lit))] = 320                                  # one facet mirrors the lamp: it saturates
            q["shade"] = shade
            q["slope"] = [int(-25 + 30 * w[f]) for f in range(4)]
            q["ridge"], q["ridge_hw"] = int(80 * (w[4] - 0.5)), int(6 + 8 * w[5])
            q["halo_r"], q["halo_depth"] = max(16, int(16 * halves[i] * (0.15 + 0.2 * w[6]))), int(5 + 15 * w[7])
        n_s = int(r.integers(self.scratches[0], self.scratches[1] + 1))
        for i in range(n_s):
            w = r.random(8)
            a = math.pi * w[3] * 2.0 if w[3] < 0.05 else theta + 0.1 * (w[2] - 0.5)      # one in twenty strays from the direction
            q = sc["scratches"][i]
            q["x"], q["y"] = _fx((S - 1) * w[0]), _fx((S - 1) * w[1])
            q["dx"], q["dy"] = int(round(16384 * math.cos(a))), int(round(16384 * math.sin(a)))
            q["hw"] = int(3 + 17 * w[4])
            d = int(-25 + 40 * w[5])
            q["depth"] = d if d != 0 else -1
            q["t0"], q["t1"] = I32_MIN, I32_MAX
            if w[6] < 0.3:
                half = int((0.05 + 0.3 * w[7]) * S * 16 * 16384)
                q["t0"], q["t1"] = -half, half
        sc["n_scratches"] = n_s
        n_b = int(r.integers(0, self.max_blobs + 1))
        for i in range(n_b):
            w = r.random(4)
            q = sc["blobs"][i]
            q["x"], q["y"], q["r"], q["dark"] = _fx((S - 1) * w[0]), _fx((S - 1) * w[1]), int(16 * (1.5 + 4.5 * w[2])), int(20 + 60 * w[3])
        sc["n_blobs"] = n_b
        w = r.random(6)
        rects = []
        if w[0] < self.p_overlay:                                                  # the camera's region marker: a red outline
            x0, y0 = int(S * 0.1 * w[1]), int(S * 0.1 * w[2])
            rects.append((x0, y0, x0 + int(S * 0.6), y0 + int(S * 0.45), max(1, S // 256), (0, 0, 255)))
        if w[3] < self.p_overlay:                                                  # the scale bar: a dark box with a white bar
            bw, bh = max(8, S // 5), max(4, S // 16)
            x0, y0 = S - bw - int(S * 0.03 * w[4]) - 1, S - bh - int(S * 0.03 * w[5]) - 1
            rects.append((x0, y0, x0 + bw - 1, y0 + bh - 1, 0, (16, 16, 16)))
            rects.append((x0 + bw // 8, y0 + bh // 2, x0 + bw - 1 - bw // 8, y0 + bh // 2 + max(0, S // 256), 0, (255, 255, 255)))
        for i, (x0, y0, x1, y1, th, col) in enumerate(rects):
            q = sc["rects"][i]
            q["x0"], q["y0"], q["x1"], q["y1"], q["thickness"], q["color"] = x0, y0, x1, y1, th, col
        sc["n_rects"] = len(rects)
        return sc


def truth(scene) -> List[dict]:
    """Per indentation of one scene: ``vertices`` float64 [4, 2] in pixels (x, y), ``d1`` (v0 to v2), ``d2`` (v1 to v3), ``d_mean``, the
    shoelace ``area`` and the inclusive ``box`` (x0, y0, x1, y1), computed in float64 from the fixed-point vertices: the coordinates are
    exact (rationals over 16)."""
    s = np.asarray(scene, SCENE_DTYPE).reshape(())
    out = []
    for k in range(int(s["n_indents"])):
        q = s["indents"][k]
        v = np.stack([q["vx"], q["vy"]], axis=1).astype(np.float64) / 16.0
        d1, d2 = float(np.hypot(*(v[2] - v[0]))), float(np.hypot(*(v[3] - v[1])))
        x, y = v[:, 0], v[:, 1]
        area = 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))
        out.append(dict(vertices=v, d1=d1, d2=d2, d_mean=0.5 * (d1 + d2), area=area, box=(float(x.min()), float(y.min()), float(x.max()), float(y.max()))))
    return out


def _scene_array(scenes) -> np.ndarray:
    if isinstance(scenes, np.ndarray) and scenes.dtype == SCENE_DTYPE:
        arr = scenes.reshape(-1)
    else:
        lst = list(scenes)
        if not lst:
            raise ValueError("need at least one scene")
        arr = np.stack([np.asarray(s, SCENE_DTYPE).reshape(()) for s in lst])
    if arr.shape[0] < 1:
        raise ValueError("need at least one scene")
    return np.ascontiguousarray(arr)


class _Buffers:
    def __init__(self):
        self.cap = 0


_buffers = {}


def render(scenes, size: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``vk_mg_render``: (uint8 [n, S, S, 3], uint8 {0, 1} [n, S, S]) on the device — views of buffers kept per (device, size) and reused
    by the next call with them.  ``scenes``: an array of ``SCENE_DTYPE`` or a sequence of such records.  No host synchronisation."""
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise L.VkError("vk.micrographs renders on the MI355X; there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    S = int(size)
    if not MIN_SIDE <= S <= MAX_SIDE:
        raise ValueError(f"size {S} outside {MIN_SIDE}..{MAX_SIDE}")
    arr = _scene_array(scenes)
    n = int(arr.shape[0])
    b = _buffers.setdefault((dev, S), _Buffers())
    if n > b.cap:
        cap = max(n, 32)
        b.rgb = torch.empty(cap, S, S, 3, dtype=torch.uint8, device=dev)
        b.mask = torch.empty(cap, S, S, dtype=torch.uint8, device=dev)
        b.scenes_dev = torch.empty(L.lib().vk_mg_scenes_dev_bytes(cap) // 4, dtype=torch.int32, device=dev)
        b.cap = cap
    with torch.cuda.device(dev):
        L.check(L.lib().vk_mg_render(n, S, arr.ctypes.data, b.scenes_dev.data_ptr(), b.scenes_dev.numel() * 4, b.rgb.data_ptr(), b.mask.data_ptr(),
                                     L.current_stream()), "vk_mg_render")
    return b.rgb[:n], b.mask[:n]


class MicrographDataset:
    """``length`` synthetic items; item i is always the scene ``SceneSampler(size=size, **sampler_kwargs)`` draws from
    ``np.random.default_rng([seed, i])``, so a validation split is stable and an item does not depend on the batch it is drawn in.
    Nothing is stored: every batch is rendered.  ``batch`` / ``loader`` return what ``DeviceDataset``'s return; the rendered buffers, the
    parameter scratch and the CLAHE workspace are reused by every call: one stream at a time."""

    def __init__(self, length: int, size: int = 512, seed: int = 0, device=None, sampler_kwargs: Optional[dict] = None):
        if int(length) < 1:
            raise ValueError("length must be positive")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise L.VkError("MicrographDataset lives on the MI355X; there is no CPU path")
        self.length, self.S, self.seed = int(length), int(size), int(seed)
        self.sampler = SceneSampler(seed=None, size=self.S, **(sampler_kwargs or {}))
        self.names = ["mg%06d" % i for i in range(self.length)]
        self._tables = None
        self._ap_dev = None
        self._arange = None
        self._clahe_ws = None

    def __len__(self) -> int:
        return self.length

    def _index(self, i) -> int:
        i = int(i)
        if not 0 <= i < self.length:
            raise ValueError(f"index {i} outside 0..{self.length - 1}")
        return i

    def scene(self, i: int) -> np.ndarray:
        return self.sampler.sample(np.random.default_rng([self.seed, self._index(i)]))

    def truth(self, i: int) -> List[dict]:
        return truth(self.scene(i))

    def _render(self, indices: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        idx = [self._index(i) for i in indices]
        if not idx:
            raise ValueError("need at least one index")
        return render([self.scene(i) for i in idx], self.S, self.device)

    def images(self, indices: Sequence[int]) -> torch.Tensor:
        """uint8 [n, S, S, 3] on the device: a view of the render buffers, valid until the next render of this size on this device."""
        return self._render(indices)[0]

    def masks(self, indices: Sequence[int]) -> torch.Tensor:
        """uint8 {0, 1} [n, S, S] on the device (for ``seg_metrics`` and ``detect_gt``): a view, as ``images``."""
        return self._render(indices)[1]

    def batch(self, indices: Sequence[int], sampler: Optional[AugmentSampler] = None, draws: Optional[Sequence[dict]] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
        """``(x float32 [n,3,S,S], y float32 [n,1,S,S], names)``: ``render`` followed by ``vk_augment_batch`` over the rendered buffers
        with index 0..n-1.  ``sampler`` / ``draws`` as ``DeviceDataset.batch`` takes them."""
        idx = [self._index(i) for i in indices]
        n, S = len(idx), self.S
        if draws is None:
            draws = [sampler.sample() if sampler is not None else IDENTITY for _ in idx]
        if len(draws) != n:
            raise ValueError("one set of draws per index")
        rgb, msk = self._render(idx)
        if self._tables is None:
            self._tables = torch.from_numpy(color_tables()).to(self.device)
        if self._arange is None or self._arange.numel() < n:
            self._arange = torch.arange(max(n, 32), dtype=torch.int32, device=self.device)
            self._ap_dev = torch.empty(max(n, 32) * C.sizeof(L.vk_aug_params), dtype=torch.uint8, device=self.device)
        x = torch.empty(n, 3, S, S, dtype=torch.float32, device=self.device)
        y = torch.empty(n, 1, S, S, dtype=torch.float32, device=self.device)
        ws_ptr, ws_bytes = None, 0
        if any(int(d["photo"]) == PHOTO_CLAHE for d in draws):
            ws_bytes = int(L.lib().vk_augment_workspace_bytes(n, S))
            if self._clahe_ws is None or self._clahe_ws.numel() < ws_bytes:
                self._clahe_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            ws_ptr = self._clahe_ws.data_ptr()
        L.check(L.lib().vk_augment_batch(n, S, n, rgb.data_ptr(), msk.data_ptr(), self._arange.data_ptr(), _params_array(draws, S),
                                         self._ap_dev.data_ptr(), self._tables.data_ptr(), ws_ptr, ws_bytes, x.data_ptr(), y.data_ptr(),
                                         L.current_stream()),
                "vk_augment_batch")
        return x, y, [self.names[i] for i in idx]

    def loader(self, batch_size: int, shuffle: bool = True, sampler: Optional[AugmentSampler] = None, seed: Optional[int] = None):
        """Iterate ``(x, y, names)`` over one epoch, as ``DeviceDataset.loader`` does."""
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        order = np.arange(len(self))
        if shuffle:
            np.random.default_rng(seed).shuffle(order)
        for b in range(0, len(order), batch_size):
            yield self.batch(order[b:b + batch_size].tolist(), sampler)
