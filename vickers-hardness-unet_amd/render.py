"""Validation panels and detection overlays on the device (csrc/render.hip).

The last stage of the reference's three programs is drawing what was computed: ``train.py``'s four-panel validation image
(``save_individual_visuals``), the GUIs' ``make_overlay`` / ``overlay`` / ``compose_canvas`` and their three annotated views
(``draw_detections_on_three``).  Here the pixels are made where the maps and the records already are::

    vk.render.save_individual_visuals(x, y, pr, names, out_dir)            # one launch, one read-back, then PIL per image
    vis = vk.render.overlay(img_bgr, prob)                                 # make_overlay / overlay
    row = vk.render.compose_canvas(img_bgr, mask)                          # [h, 3 w, 3]
    vis_o, vis_b, vis_v = vk.render.draw_detections_on_three(img_bgr, dets.clean[0], None, fine, reduce=4)
    rows, vis_o, vis_b, vis_v = vk.Segmenter(model).render(img_bgr)        # measure + the three views

Images are BGR as in the reference.  The blend is ``cv2.addWeighted``'s documented float32 rule; the thick lines, the 5 x 7 font and
the absence of antialiasing (the GUIs ask ``cv2.putText`` for ``LINE_AA``) are this package's own, not OpenCV's: the views show the
same geometry and the same numbers, not the same bytes as the GUIs'.  JPEG files are written by PIL, so their bytes are PIL's.  CUDA
tensors only; numpy images are uploaded."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from . import subpix as SP
from ._lib import VkError

__all__ = ["DIAG_COLOR", "IMAGENET_MEAN", "IMAGENET_STD", "PALETTE", "PRIM_DTYPE", "box_reduce", "compose_canvas", "draw", "draw_detections_on_three",
           "glyph", "overlay", "primitives", "render", "save_individual_visuals", "val_panels"]

PRIM_DTYPE = np.dtype(L.vk_render_prim)
IMAGENET_MEAN = (0.485, 0.456, 0.406)          # train.py:322
IMAGENET_STD = (0.229, 0.224, 0.225)
PALETTE = ((0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (0, 165, 255), (255, 255, 0), (147, 20, 255), (50, 205, 50))
DIAG_COLOR = (0, 0, 255)                       # ui_infer_rectangle.py:405-415
PANEL_COLOR = (0, 140, 255)                    # train.py:339, infer_pth_gui.py:55
_COORDS = {"box": L.VK_RENDER_COORD_BOX, "v": L.VK_RENDER_COORD_V, "vs": L.VK_RENDER_COORD_VS}


def glyph(ch: str) -> List[int]:
    """The seven rows of the 5 x 7 glyph of ``ch`` (top first, bit 4 = the left column), as the library draws it."""
    rows = (C.c_uint8 * 7)()
    L.check(L.lib().vk_render_glyph(ord(ch), rows), "vk_render_glyph")
    return list(rows)


def _blend(color, alpha: float, beta: float, gamma: float = 0.0) -> L.vk_render_blend:
    c = [int(v) for v in color]
    if len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise ValueError("a colour is three bytes (B, G, R), got %r" % (color,))
    return L.vk_render_blend((C.c_uint8 * 3)(*c), 0, float(alpha), float(beta), float(gamma))


def _device_of(*ts) -> torch.device:
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda")


def _image(img, device, what: str = "image") -> torch.Tensor:
    """uint8 [h, w, 3] on the device; a tensor that is there already is used where it is (its row stride is free)."""
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("%s: expected a uint8 BGR image [h, w, 3]" % what)
    if not t.is_cuda:
        t = t.to(device)
    if t.shape[0] > 1 and (t.stride(2) != 1 or t.stride(1) != 3):
        t = t.contiguous()
    return t


def _mask(m, device) -> torch.Tensor:
    """uint8 or float32 [h, w] on the device."""
    t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("mask: expected a uint8 or floating map [h, w]")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8:
        if not t.dtype.is_floating_point:
            raise ValueError("mask: expected a uint8 or floating map [h, w], got %s" % t.dtype)
        t = t.float()
    if not t.is_cuda:
        t = t.to(device)
    if t.shape[0] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t


def _row_stride(t: torch.Tensor) -> int:
    return int(t.stride(0)) * t.element_size() if t.shape[0] > 1 else int(t.shape[1]) * (3 if t.dim() == 3 else 1) * t.element_size()


# ------------------------------------------------------------------------------------------------ panels
def val_panels(x: torch.Tensor, y: torch.Tensor, prob: torch.Tensor, *, mean: Sequence[float] = IMAGENET_MEAN,
               std: Sequence[float] = IMAGENET_STD, order: str = "bgr", color=PANEL_COLOR, alpha: float = 1.0, beta: float = 0.35,
               gamma: float = 0.0) -> torch.Tensor:
    """train.py's [image | ground truth | prediction | overlay] rows: x float32 [N, 3, H, W] (normalised RGB planes), y and prob
    float32 [N, 1, H, W] -> uint8 [N, H, 4 W, 3] on the device.  ``order``: "bgr" (what the reference hands to ``cv2.imwrite``) or
    "rgb" (what PIL wants)."""
    if order not in ("bgr", "rgb"):
        raise ValueError("order must be 'bgr' or 'rgb'")
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[1] == 3):
        raise ValueError("x: expected float32 [N, 3, H, W]")
    N, _, H, W = (int(v) for v in x.shape)
    maps = []
    for name, t in (("y", y), ("prob", prob)):
        if not isinstance(t, torch.Tensor) or t.numel() != N * H * W or tuple(t.shape[-2:]) != (H, W):
            raise ValueError("%s: expected float32 [%d, 1, %d, %d]" % (name, N, H, W))
        maps.append(t)
    if not x.is_cuda:
        raise VkError("x is on %s: this package runs on an MI355X only and has no CPU fallback" % x.device)
    x, y, prob = (t.detach().to(x.device).float().contiguous() for t in (x, maps[0], maps[1]))
    out = torch.empty(N, H, 4 * W, 3, dtype=torch.uint8, device=x.device)
    bl = _blend(color, alpha, beta, gamma)
    L.check(L.lib().vk_render_val_panels(N, H, W, x.data_ptr(), y.data_ptr(), prob.data_ptr(), (C.c_double * 3)(*mean), (C.c_double * 3)(*std),
                                         C.byref(bl), L.VK_RENDER_RGB if order == "rgb" else 0, out.data_ptr(), 12 * W, L.current_stream()),
            "vk_render_val_panels")
    return out


def save_individual_visuals(x: torch.Tensor, y: torch.Tensor, pr: torch.Tensor, names: Sequence[str], out_dir, quality: int = 95) -> None:
    """train.py:285-350 with its signature: ``out_dir/<name>.jpg`` per image.  One launch and one read-back for the batch; the JPEG
    encoder is PIL's (the reference's is OpenCV's), so the files show the same canvas but are not the same bytes."""
    from PIL import Image
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    canvas = val_panels(x, y, pr, order="rgb").cpu().numpy()
    if len(names) != canvas.shape[0]:
        raise ValueError("%d names for %d images" % (len(names), canvas.shape[0]))
    for i, name in enumerate(names):
        Image.fromarray(canvas[i]).save(str(out_dir / ("%s.jpg" % name)), quality=int(quality))


# ------------------------------------------------------------------------------------------------ primitives
def _style(palette, diag_color, thickness: int, text_scale: int) -> L.vk_render_style:
    pal = [[int(v) for v in c] for c in palette]
    if len(pal) != 8 or any(len(c) != 3 for c in pal):
        raise ValueError("the palette is eight (B, G, R) colours")
    st = L.vk_render_style()
    for i, c in enumerate(pal):
        for j in range(3):
            st.palette[i][j] = c[j]
    for j in range(3):
        st.diag[j] = int(diag_color[j])
    st.thickness, st.text_scale = int(thickness), int(text_scale)
    return st


def _layout(dets: G.Detections, coords: Optional[str]) -> Tuple[int, int, int, int, int]:
    """(coordinate mode, box offset, valid offset, diag offset, center offset) of the records of ``dets``."""
    refined = isinstance(dets, SP.RefinedDetections)
    coords = ("vs" if refined else "box") if coords is None else coords
    if coords not in _COORDS or (coords != "box") != refined:
        raise ValueError("coords must be 'v' or 'vs' for refined detections and 'box' for geometry records, got %r" % (coords,))
    if refined:
        Q = L.vk_subpix_quad
        return _COORDS[coords], int(getattr(Q, coords).offset), int(Q.valid.offset), int(Q.d_mean.offset), -1
    rec = G._fit(dets.fit).record
    return _COORDS["box"], dets.box_offset, dets.valid_offset, dets.diag_offset, int(rec.cx.offset)


def primitives(dets: G.Detections, *, affine=None, coords: Optional[str] = None, thickness: int = 2, text_scale: int = 2,
               palette=PALETTE, diag_color=DIAG_COLOR) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The drawing list of every map of ``dets`` (a ``Detections``, ``RefinedDetections`` or ``ZoomedDetections``), built on the device
    from the records in place -> (records uint8 [B, max_components, 104] (``PRIM_DTYPE``, rank order), drawn int32 [B], skipped int32
    [B]).  ``coords``: "box" for geometry records, "vs" (default) or "v" for refined ones; ``affine``: (ox, oy, inv_scale) rows as in
    ``vk.subpix.refine``, applied to "box" and "v".  No host synchronisation."""
    if not isinstance(dets, G.Detections):
        raise ValueError("expected Detections")
    mode, box_off, valid_off, diag_off, center_off = _layout(dets, coords)
    if not dets.raw.is_cuda:
        raise VkError("the detections are on %s: this package runs on an MI355X only and has no CPU fallback" % dets.raw.device)
    dev = dets.raw.device
    B, M = int(dets.raw.shape[0]), dets.max_components
    st = _style(palette, diag_color, thickness, text_scale)
    aff = SP._affine_tensor(affine, B, dev)
    prims = G._record_buffer((B, M), PRIM_DTYPE.itemsize, dev, zero=True)
    drawn = torch.zeros(B, dtype=torch.int32, device=dev)
    skipped = torch.zeros(B, dtype=torch.int32, device=dev)
    L.check(L.lib().vk_render_primitives(B, dets.raw.data_ptr(), dets.record_bytes, box_off, valid_off, diag_off, center_off, mode,
                                         dets.counts.data_ptr(), M, L.ptr(aff), C.byref(st), prims.data_ptr(), drawn.data_ptr(),
                                         skipped.data_ptr(), L.current_stream()), "vk_render_primitives")
    return prims, drawn, skipped


def _pack_list(rows: Sequence[Dict], coords: Optional[str], device) -> G.Detections:
    """The GUIs' list of dicts as one map of records on the device, in list order: ``vk_subpix_quad``-shaped when the rows carry
    ``box_subpix`` (and ``coords`` is not "box"), else ``vk_geom_det``-shaped with ``det["box"].astype(np.int32)`` as the GUIs take it.
    The area field holds len - position, so that the list's order is the drawing order, as ``enumerate(detections, start=1)`` is."""
    n = len(rows)
    M = max(n, 1)
    refined = n > 0 and coords != "box" and all("box_subpix" in d for d in rows)
    if refined:
        recs = np.zeros(M, SP.RECORD_DTYPE)
        for i, d in enumerate(rows):
            recs[i]["label"], recs[i]["area"], recs[i]["valid"] = int(d.get("label", i + 1)), n - i, 1
            recs[i]["vs"] = np.asarray(d["box_subpix"], np.float64).reshape(8)
            recs[i]["v"] = np.asarray(d.get("box_subpix_map", d["box_subpix"]), np.float64).reshape(8)
            recs[i]["d_mean"] = float(d["d_mean"])
    else:
        recs = np.zeros(M, np.dtype(L.vk_geom_det))
        for i, d in enumerate(rows):
            recs[i]["label"], recs[i]["area"] = int(d.get("label", i + 1)), n - i
            recs[i]["box"] = np.asarray(d["box"]).astype(np.int32).reshape(8)
            recs[i]["cx"], recs[i]["cy"] = float(d["center"][0]), float(d["center"][1])
            recs[i]["d_mean"] = float(d["d_mean"])
    raw = G._record_buffer((1, M), recs.dtype.itemsize, device)
    raw.copy_(torch.from_numpy(recs.view(np.uint8).reshape(1, M, -1)))
    counts = torch.tensor([n], dtype=torch.int32, device=device)
    base = G.Detections("rect", None, raw, counts, None, M)
    return SP.RefinedDetections(base, raw, "list") if refined else base


# ------------------------------------------------------------------------------------------------ draw
def draw(src: torch.Tensor, mask: torch.Tensor, outs: Sequence[Optional[torch.Tensor]], *, color=DIAG_COLOR, alpha: float = 0.35,
         thresh: float = 0.5, prims: Optional[torch.Tensor] = None, drawn: Optional[torch.Tensor] = None, index: int = 0,
         flags: int = 0) -> None:
    """``vk_render_draw`` for one map: ``src`` uint8 [h, w, 3] and ``mask`` (uint8: nonzero, or float32: > thresh) on the device; ``outs``
    = (vis_o, vis_b, vis_v), each a uint8 [h, w, 3] device tensor whose row stride is free, or None; ``prims`` / ``drawn``: the list of
    ``primitives``, of which map ``index`` is painted.  ``alpha`` is the weight of the overlay colour, as in the reference."""
    h, w = int(src.shape[0]), int(src.shape[1])
    if tuple(mask.shape) != (h, w):
        raise ValueError("the mask %s does not fit the image %s" % (tuple(mask.shape), (h, w)))
    kind = L.VK_RENDER_MASK_U8 if mask.dtype == torch.uint8 else L.VK_RENDER_MASK_F32
    view = L.vk_render_view(src.data_ptr(), _row_stride(src), mask.data_ptr(), _row_stride(mask), (C.c_uint64 * 3)(), (C.c_int64 * 3)(), h, w)
    for i, o in enumerate(outs):
        if o is None:
            continue
        if o.dtype != torch.uint8 or tuple(o.shape) != (h, w, 3) or not o.is_cuda or (h > 1 and (o.stride(2) != 1 or o.stride(1) != 3)):
            raise ValueError("output %d: expected a uint8 device tensor [%d, %d, 3] with contiguous pixels" % (i, h, w))
        view.out[i], view.out_stride[i] = o.data_ptr(), _row_stride(o)
    view_dev = torch.empty(C.sizeof(L.vk_render_view) // 8, dtype=torch.int64, device=src.device)
    bl = _blend(color, 1.0, alpha)
    if prims is not None:
        M = int(prims.shape[1])
        plist = (prims[index].data_ptr(), drawn[index:index + 1].data_ptr(), M)
    else:
        plist = (None, None, 0)
    L.check(L.lib().vk_render_draw(1, C.byref(view), view_dev.data_ptr(), kind, float(thresh), C.byref(bl), *plist, int(flags),
                                   L.current_stream()), "vk_render_draw")


def box_reduce(img: torch.Tensor, k: int) -> torch.Tensor:
    """Box reduction of a uint8 [h, w, 3] device image by the integer factor ``k`` (1..16) -> [ceil(h / k), ceil(w / k), 3]: per channel
    the rounded mean of the block; edge blocks are partial."""
    img = _image(img, _device_of(img))
    h, w = int(img.shape[0]), int(img.shape[1])
    k = int(k)
    out = torch.empty(-(-h // max(k, 1)), -(-w // max(k, 1)), 3, dtype=torch.uint8, device=img.device)
    L.check(L.lib().vk_render_reduce(h, w, k, img.data_ptr(), _row_stride(img), out.data_ptr(), 3 * int(out.shape[1]), L.current_stream()),
            "vk_render_reduce")
    return out


def overlay(img_bgr, mask_or_prob, color=DIAG_COLOR, alpha: float = 0.35, thresh: float = 0.5) -> torch.Tensor:
    """``make_overlay`` (ui_infer_*.py) and ``overlay`` (infer_pth_gui.py: pass its colour): the image with ``color`` blended in at
    weight ``alpha`` where a uint8 mask is nonzero or a floating map is above ``thresh`` -> uint8 [h, w, 3] on the device."""
    dev = _device_of(img_bgr, mask_or_prob)
    src = _image(img_bgr, dev)
    m = _mask(mask_or_prob, src.device)
    out = torch.empty(int(src.shape[0]), int(src.shape[1]), 3, dtype=torch.uint8, device=src.device)
    draw(src, m, (None, None, out), color=color, alpha=alpha, thresh=thresh)
    return out


def compose_canvas(img_bgr, mask, color=PANEL_COLOR, alpha: float = 0.35, thresh: float = 0.5) -> torch.Tensor:
    """infer_pth_gui.py:59-64: [image | mask | overlay] side by side -> uint8 [h, 3 w, 3] on the device, BGR (the reference turns
    the row to RGB for Tk afterwards: ``canvas.flip(-1)``).  One pass: the three views are column ranges of the one canvas."""
    dev = _device_of(img_bgr, mask)
    src = _image(img_bgr, dev)
    m = _mask(mask, src.device)
    h, w = int(src.shape[0]), int(src.shape[1])
    canvas = torch.empty(h, 3 * w, 3, dtype=torch.uint8, device=src.device)
    draw(src, m, tuple(canvas[:, i * w:(i + 1) * w] for i in range(3)), color=color, alpha=alpha, thresh=thresh)
    return canvas


def draw_detections_on_three(img_bgr, clean_bin, overlay_bgr, detections: Union[G.Detections, Sequence[Dict]], *, affine=None,
                             coords: Optional[str] = None, thickness: int = 2, text_scale: int = 2, reduce: int = 1, index: int = 0,
                             color=DIAG_COLOR, alpha: float = 0.35, thresh: float = 0.5, palette=PALETTE, diag_color=DIAG_COLOR,
                             flags: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """ui_infer_*.py ``draw_detections_on_three``: box, two diagonals and ``#<n> mean=<d>px`` of every detection on the image, on the
    binary map and on the overlay -> (vis_o, vis_b, vis_v), uint8 device tensors [h, w, 3] ([ceil(h / reduce), ceil(w / reduce), 3] after
    the box reduction).  ``overlay_bgr``: None makes the overlay in the same pass from ``clean_bin`` (a uint8 mask or a floating map
    above ``thresh``) with ``color`` at weight ``alpha``; an image is drawn on as it is.  ``detections``: a device handle (map ``index``
    of it is drawn; refined records with their ``vs`` coordinates unless ``coords`` says "v") or the GUIs' list of dicts, drawn in list
    order.  ``affine``: the (ox, oy, inv_scale) row that takes "box" / "v" coordinates to this image."""
    dev = _device_of(img_bgr, clean_bin, detections.raw if isinstance(detections, G.Detections) else None)
    src = _image(img_bgr, dev)
    m = _mask(clean_bin, src.device)
    if isinstance(detections, G.Detections):
        dets = detections
    else:
        dets, index = _pack_list(list(detections), coords, src.device), 0
    prims, drawn, _ = primitives(dets, affine=affine, coords=coords, thickness=thickness, text_scale=text_scale, palette=palette,
                                 diag_color=diag_color)
    h, w = int(src.shape[0]), int(src.shape[1])
    vis = [torch.empty(h, w, 3, dtype=torch.uint8, device=src.device) for _ in range(3)]
    if overlay_bgr is None:
        draw(src, m, vis, color=color, alpha=alpha, thresh=thresh, prims=prims, drawn=drawn, index=index, flags=flags)
    else:
        draw(src, m, (vis[0], vis[1], None), color=color, alpha=alpha, thresh=thresh, prims=prims, drawn=drawn, index=index, flags=flags)
        draw(_image(overlay_bgr, src.device, "overlay"), m, (vis[2], None, None), prims=prims, drawn=drawn, index=index, flags=flags)
    if int(reduce) != 1:
        vis = [box_reduce(v, int(reduce)) for v in vis]
    return vis[0], vis[1], vis[2]


def render(seg, img_bgr, fit: str = "quad", zoom: bool = True, reduce: int = 1, method: str = "corner", **kw):
    """``Segmenter.render``: ``Segmenter.measure`` plus the three views of the image at its own size, drawn with the refined ``vs``
    coordinates -> (detection list, vis_o, vis_b, vis_v), the images as numpy uint8.  The mask shown is the un-letterboxed probability
    above the fit's threshold (the morphological cleaning happens on the letterboxed map).  ``thickness`` and ``text_scale`` in ``kw``
    go to the drawing, the rest to ``vk.zoom.refine_detections``."""
    from . import prepost as PP
    from . import zoom as Z
    style = {k: kw.pop(k) for k in ("thickness", "text_scale") if k in kw}
    src, meta, logits, dets, fine = Z._measure(seg, img_bgr, fit, zoom, method, **kw)
    prob = PP.postprocess_prob(logits, meta)
    views = draw_detections_on_three(src, prob, None, fine, reduce=reduce, thresh=G._fit(fit).bin_thresh, **style)
    return (Z._lists(dets, fine, fit)[0],) + tuple(v.cpu().numpy() for v in views)
