"""Markers of any shape: connected components of a thresholded plane (``find_blobs``; not in the reference, whose
finders are circle finders).

``label`` names the components of ``plane > threshold`` (or ``<``) on the device -- numbered in raster order of their
first pixel, as ``scipy.ndimage.label`` numbers them, with area, coordinate sums, bounding box and first pixel of each --,
``threshold_mask`` is that mask alone, ``fill_holes`` is ``scipy.ndimage.binary_fill_holes``, ``select`` keeps components by area and by whether they touch the
frame, renumbers the map and gives the marker table, ``otsu_level`` is the project's Otsu rule on a uint8 plane.  All of
it is integer arithmetic in mg_blobs.hip; ``tests/blobs_ref.py`` restates the contract in NumPy + scipy.ndimage.

``find_blobs`` is the component: time 0 of one search channel decides, windows / masks / sums come from the label-map
ROI pass (``hotpath.roi_gather_reduce(..., labels=, disks=False)``), and the outputs are laid out as ``find_beads`` lays
them out.  ``mg.blobs(data, ...)`` and ``mg.blobs_pipe(...)`` are its pipelines: this module is callable.
"""
from __future__ import annotations

import numbers
import sys
import types

import numpy as np
import torch

from . import _native as nat
from . import registry, utils
from .utils import int_in

TILE_H, TILE_W = nat.DEFINES["MG_BLOB_TILE_H"], nat.DEFINES["MG_BLOB_TILE_W"]
OVERFLOW, EBOUND = nat.DEFINES["MG_BLOB_OVERFLOW"], nat.DEFINES["MG_BLOB_EBOUND"]
MAX_ROI_LENGTH = 244  # the label-map ROI pass holds a window's flags in LDS (mg_roi_gather_reduce_batched)
STATS = ("area", "sum_y", "sum_x", "y_min", "x_min", "y_max", "x_max", "first_pixel")
_DTYPES = ("uint8", "uint16", "float32", "float64")

_WORK = {}


def _workspace(h, w, cap, device):
    """Workspace cache, as ``find._finder`` caches CircleFinder: the scratch of mg_blob_labels, its {K, status} pair and
    its (cap, 8) statistics rows per (h, w, cap, device); a caller gets a copy of the K rows in use."""
    key = (h, w, cap, str(device))
    ws = _WORK.get(key)
    if ws is None:
        if len(_WORK) > 4:
            _WORK.clear()
        n = int(nat.lib().mg_blob_scratch_bytes(h, w, cap))
        if n < 0:
            raise ValueError(f"blobs: a plane of {h} x {w} pixels is beyond the int32 indices of the label map")
        ws = {"scratch": torch.empty(max(n, 16), dtype=torch.uint8, device=device),
              "head": torch.zeros(2, dtype=torch.int32, device=device),
              "stats": torch.empty((cap, 8), dtype=torch.int64, device=device)}
        _WORK[key] = ws
    return ws


def _number(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or v != v:
        raise ValueError(f"{name} must be a real number (not NaN), got {v!r}")
    return float(v)


def _plane(name, plane, dtypes=_DTYPES):
    """A 2-D tensor / array of a supported dtype, checked on the host; h * w within int32."""
    if isinstance(plane, np.ndarray):
        plane = torch.from_numpy(np.ascontiguousarray(plane))
    if not isinstance(plane, torch.Tensor):
        raise ValueError(f"{name} must be a tensor or an array, got {type(plane).__name__}")
    if plane.dim() != 2 or plane.shape[0] < 1 or plane.shape[1] < 1:
        raise ValueError(f"{name} must be one non-empty (h, w) plane, got shape {tuple(plane.shape)}")
    if str(plane.dtype).replace("torch.", "") not in dtypes:
        raise ValueError(f"{name} must be of dtype {' / '.join(dtypes)}, got {plane.dtype}")
    if plane.shape[0] * plane.shape[1] > 2 ** 31 - 1:
        raise ValueError(f"{name}: {plane.shape[0]} x {plane.shape[1]} pixels are beyond the int32 indices of the label map")
    return plane


def _on_device(plane):
    from . import hotpath

    hotpath.require_gpu()
    return (plane if plane.is_cuda else plane.cuda()).contiguous()


def check_label(threshold, below=False, connectivity=8, max_components=1 << 20):
    """The settings of ``label``; ValueError that names the argument otherwise.  -> threshold as a float."""
    threshold = _number("threshold", threshold)
    if connectivity not in (4, 8) or isinstance(connectivity, (bool, np.bool_)):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    int_in("max_components", max_components, 1, 2 ** 31 - 1)
    if not isinstance(below, (bool, np.bool_)):
        raise ValueError(f"below must be a bool, got {below!r}")
    return threshold


def threshold_mask(plane, threshold, below=False):
    """uint8 (h, w) on the device: 1 where ``plane > threshold`` (``below``: ``<``; NaN is never on), the mask that
    ``label`` names the components of (mg_blob_threshold)."""
    from . import hotpath

    plane = _plane("plane", plane)
    threshold = check_label(threshold, below)
    plane = _on_device(plane)
    h, w = plane.shape
    on = torch.empty((h, w), dtype=torch.uint8, device=plane.device)
    hotpath._call("mg_blob_threshold", plane.data_ptr(), nat.dtype_code(plane.dtype), h, w, threshold, int(bool(below)),
                  on.data_ptr(), hotpath._stream())
    return on


def label(plane, threshold, below=False, connectivity=8, max_components=1 << 20):
    """Connected components of ``plane > threshold`` (``below``: ``<``; NaN is never on) under 4- or 8-connectivity.
    -> {"labels": int32 (h, w), -1 where off, else 0 .. K-1 in raster order of the components' first pixels;
    "count": K (an int); "stats": int64 (K, 8) = ``STATS``} on the device.
    ValueError where there are more than ``max_components`` components."""
    from . import hotpath

    plane = _plane("plane", plane)
    threshold = check_label(threshold, below, connectivity, max_components)
    plane = _on_device(plane)
    h, w = plane.shape
    # (no plane has more than ceil(h w / 2) components: a larger capacity is the same capacity)
    cap, dev = min(int(max_components), (h * w + 1) // 2), plane.device
    ws = _workspace(h, w, cap, dev)
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    head, stats = ws["head"], ws["stats"]
    hotpath._call("mg_blob_labels", plane.data_ptr(), nat.dtype_code(plane.dtype), h, w, threshold, int(bool(below)),
                  int(connectivity), labels.data_ptr(), head.data_ptr(), stats.data_ptr(), cap, head.data_ptr() + 4,
                  ws["scratch"].data_ptr(), ws["scratch"].numel(), hotpath._stream())
    k, status = (int(v) for v in head.cpu().numpy())
    if status & EBOUND:
        raise RuntimeError("mg_blob_labels: a bounded loop ran out (internal error)")
    if status & OVERFLOW:
        raise ValueError(f"max_components: the plane has {k} components, more than max_components = {cap}")
    return {"labels": labels, "count": k, "stats": stats[:k].clone()}


def fill_holes(on, max_components=1 << 20):
    """``scipy.ndimage.binary_fill_holes(on)`` (default structure) of a bool / uint8 (h, w) mask -> uint8 on the device:
    the 4-connected components of the complement that touch no side of the frame are switched on."""
    from . import hotpath

    if isinstance(on, (torch.Tensor, np.ndarray)) and str(on.dtype).replace("torch.", "") == "bool":
        on = on.view(torch.uint8 if isinstance(on, torch.Tensor) else np.uint8)
    on = _plane("on", on, ("uint8",))
    int_in("max_components", max_components, 1, 2 ** 31 - 1)
    on = _on_device(on)
    comp = label(on, 0.5, below=True, connectivity=4, max_components=max_components)  # the complement: the zero bytes
    out = on.clone()  # (a filled pixel becomes 1; a non-zero byte of the caller's stays what it was)
    if comp["count"]:
        h, w = on.shape
        hotpath._call("mg_blob_fill_holes", comp["labels"].data_ptr(), comp["stats"].data_ptr(), comp["count"], h, w,
                      out.data_ptr(), hotpath._stream())
    return out


def check_select(min_area=1, max_area=None, clear_border=False):
    int_in("min_area", min_area, 0, None)
    if max_area is not None:
        int_in("max_area", max_area, 1, None)
        if max_area < min_area:
            raise ValueError(f"max_area must be at least min_area = {min_area}, got {max_area}")
    if not isinstance(clear_border, (bool, np.bool_)):
        raise ValueError(f"clear_border must be a bool, got {clear_border!r}")


def select(labels, stats, min_area=1, max_area=None, clear_border=False):
    """Keep component k iff ``min_area <= area`` (``<= max_area`` where given) and, with ``clear_border``, its bounding
    box touches no side of the frame.  ``labels`` is REWRITTEN IN PLACE: a kept component takes its new number 0 .. M-1
    (the order stays), a rejected one -2, the background stays -1.  -> {"labels", "count": M, "stats": int64 (M, 8),
    "table": int32 (M, 3) = [row, col, r]} with row = floor((2 sum_y + area) / (2 area)), col likewise, and r the nearest
    integer to sqrt(area / pi) with pi as 355 / 113 (the largest r with 355 (2 r - 1)^2 <= 452 area)."""
    from . import hotpath

    check_select(min_area, max_area, clear_border)
    for name, t, dt in (("labels", labels, torch.int32), ("stats", stats, torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 2:
            raise ValueError(f"{name} must be the 2-D {dt} tensor that label() gave")
    if stats.shape[1] != 8:
        raise ValueError(f"stats must be (K, 8), got {tuple(stats.shape)}")
    hotpath.require_gpu()
    if not labels.is_cuda or not stats.is_cuda or not labels.is_contiguous():
        raise ValueError("labels and stats must be contiguous device tensors")
    h, w = labels.shape
    k, dev = int(stats.shape[0]), labels.device
    if k == 0:
        return {"labels": labels, "count": 0, "stats": stats[:0].clone(), "table": torch.zeros((0, 3), dtype=torch.int32, device=dev)}
    stats = stats.contiguous()
    num = torch.tensor([k, 0], dtype=torch.int32, device=dev)
    kept = torch.empty((k, 8), dtype=torch.int64, device=dev)
    table = torch.empty((k, 3), dtype=torch.int32, device=dev)
    remap = torch.empty(k, dtype=torch.int32, device=dev)
    hotpath._call("mg_blob_select", labels.data_ptr(), h, w, stats.data_ptr(), num.data_ptr(), k, int(min_area),
                  0 if max_area is None else int(max_area), int(bool(clear_border)), num.data_ptr() + 4, kept.data_ptr(),
                  table.data_ptr(), remap.data_ptr(), hotpath._stream())
    m = int(num[1].item())
    return {"labels": labels, "count": m, "stats": kept[:m], "table": table[:m]}


def otsu_histogram_level(hist) -> int:
    """The project's Otsu rule (tests/segment_ref.py::otsu_k) on a 256-bin histogram: the smallest k in 0 .. 254 of the
    largest d^2 / (w0 w1), d = stot w0 - n s0 in exact integers, the quotient in float64."""
    h = [int(v) for v in hist]
    n, stot = sum(h), sum(i * v for i, v in enumerate(h))
    best, best_k, w0, s0 = -1.0, 0, 0, 0
    for k in range(255):
        w0, s0 = w0 + h[k], s0 + k * h[k]
        w1 = n - w0
        if w0 > 0 and w1 > 0:
            d = float(stot * w0 - n * s0)
            value = (d * d) / float(w0 * w1)
            if value > best:
                best, best_k = value, k
    return best_k


def otsu_level(u8_plane) -> int:
    """Otsu's level k of a uint8 plane (the plane splits into ``<= k`` and ``> k``): its 256-bin histogram in one pass
    of mg_percentile_histogram, then ``otsu_histogram_level`` on the host."""
    from . import hotpath

    plane = _on_device(_plane("u8_plane", u8_plane, ("uint8",)))
    view, n0, s0, n1, s1, unit = hotpath._units(plane)
    hist = torch.zeros((1, 256), dtype=torch.int64, device=plane.device)
    hotpath._call("mg_percentile_histogram", view.data_ptr(), nat.MG_U8, n0, s0, n1, s1, unit, 0, 8, 0, 0, 0,
                  hist.data_ptr(), hotpath._stream())
    return otsu_histogram_level(hist[0].cpu().numpy())


def to_uint8(plane, minmax=None, smooth=False):
    """``to_uint8`` of one (h, w) plane on the device (mg_to_uint8_blur; ``minmax``: its (1, 2) float64 min / max where
    the caller has them), with ``smooth`` after the 5 x 5 Gaussian blur of the finders."""
    from . import hotpath

    plane = _on_device(_plane("plane", plane))
    h, w = plane.shape
    if minmax is None:
        minmax = hotpath.plane_minmax(plane[None])
    blur, u8 = (torch.empty((h, w), dtype=torch.uint8, device=plane.device) for _ in range(2))
    hotpath._call("mg_to_uint8_blur", plane.data_ptr(), nat.dtype_code(plane.dtype), 1, h * w, h, w, w, minmax.data_ptr(),
                  blur.data_ptr(), u8.data_ptr(), hotpath._stream())
    return blur if smooth else u8


# --------------------------------------------------------------------------------------
# find_blobs
# --------------------------------------------------------------------------------------


def check_blobs(threshold="otsu", search_channel=None, polarity="bright", smooth=False, connectivity=8, fill_holes=False,
                min_area=20, max_area=None, clear_border=False, roi_length=None, max_components=1 << 20):
    """The settings of ``find_blobs`` as the pipelines take them; ValueError that names the argument otherwise.
    -> (use_otsu, threshold)."""
    if isinstance(threshold, str):
        if threshold != "otsu":
            raise ValueError(f'threshold must be "otsu" or a number, got {threshold!r}')
        use_otsu, level = True, 0.0
    else:
        use_otsu, level = False, _number("threshold", threshold)
    if len(utils.to_list(search_channel)) > 1:
        raise ValueError(f"search_channel: find_blobs searches one channel, got {search_channel!r}")
    if polarity not in ("bright", "dark"):
        raise ValueError(f'polarity must be "bright" or "dark", got {polarity!r}')
    for name, v in (("smooth", smooth), ("fill_holes", fill_holes)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, got {v!r}")
    if smooth and not use_otsu:
        raise ValueError("smooth=True blurs the uint8 plane of threshold=\"otsu\"; it cannot go with a number")
    check_label(0.0, False, connectivity, max_components)
    check_select(min_area, max_area, clear_border)
    if roi_length is not None:
        int_in("roi_length", roi_length, 1, None)
        if roi_length > MAX_ROI_LENGTH:
            raise ValueError(f"roi_length must not exceed {MAX_ROI_LENGTH} (the ROI pass holds a window in LDS), got {roi_length}")
    return use_otsu, level


def auto_roi_length(stats) -> int:
    """The smallest even L that is at least the largest bounding-box side + 8 (``stats``: host (M, 8))."""
    if len(stats) == 0:
        return 8
    side = int(max((stats[:, 5] - stats[:, 3]).max(), (stats[:, 6] - stats[:, 4]).max())) + 1
    return side + 8 + (side & 1)


class BlobFinder:
    def __init__(self, threshold="otsu", search_channel=None, polarity="bright", smooth=False, connectivity=8,
                 fill_holes=False, min_area=20, max_area=None, clear_border=False, roi_length=None,
                 max_components=1 << 20):
        self.use_otsu, self.level = check_blobs(threshold, search_channel, polarity, smooth, connectivity, fill_holes,
                                                min_area, max_area, clear_border, roi_length, max_components)
        self.search_channels = utils.to_list(search_channel)
        self.dark, self.smooth, self.connectivity, self.fill = polarity == "dark", bool(smooth), connectivity, bool(fill_holes)
        self.min_area, self.max_area, self.clear_border = min_area, max_area, bool(clear_border)
        self.roi_length, self.max_components = roi_length, max_components

    def detect(self, plane, minmax=None):
        """(h, w) device plane -> (label() result or None for a flat plane under "otsu", threshold in plane units)."""
        from . import hotpath

        kw = dict(connectivity=self.connectivity, max_components=self.max_components)
        if self.use_otsu:
            if minmax is None:
                minmax = hotpath.plane_minmax(plane[None])
            lo, hi = (float(v) for v in minmax.reshape(2).cpu().numpy())
            if not (np.isfinite(hi - lo) and hi > lo):
                return None, float("nan")
            u8 = to_uint8(plane, minmax, self.smooth)
            k = otsu_level(u8)
            source, cut, level = u8, k + 0.5, lo + (k + 1) * (hi - lo) / 255
        else:
            source, cut, level = plane, self.level, self.level
        if self.fill:  # the mask, its complement labelled and the holes filled, then the filled mask labelled
            filled = fill_holes(threshold_mask(source, cut, self.dark), self.max_components)
            return label(filled, 0.0, **kw), level
        return label(source, cut, below=self.dark, **kw), level

    def __call__(self, assay):
        from . import find, hotpath
        from ._dataset import channel_index
        from .xr_lite import DataArray

        image = find._image_tensor(assay)
        n_c, n_t, h, w = image.shape
        ch = channel_index(assay, self.search_channels[0]) if self.search_channels else 0
        found, level = self.detect(image[ch, 0], find._plane_minmax(assay, image, (ch, 0)))
        dev = image.device
        if found is None:  # a flat plane: no marker
            components, stats = 0, np.zeros((0, 8), dtype=np.int64)
            table, labels = np.zeros((0, 3), dtype=np.int32), None
        else:
            components = found["count"]
            kept = select(found["labels"], found["stats"], self.min_area, self.max_area, self.clear_border)
            stats, table, labels = kept["stats"].cpu().numpy(), kept["table"].cpu().numpy(), kept["labels"]
        m = len(table)
        L = self.roi_length if self.roi_length is not None else auto_roi_length(stats)
        if m and (L > MAX_ROI_LENGTH or L > min(h, w)):
            raise ValueError(f"find_blobs: the windows would be {L} pixels long (the limit is min({MAX_ROI_LENGTH}, image "
                             f"height, image width) = {min(MAX_ROI_LENGTH, h, w)}): set max_area or roi_length")
        L = min(L, h, w)
        if labels is None:
            labels = torch.full((h, w), -1, dtype=torch.int32, device=dev)
        out = hotpath.roi_gather_reduce(image[None], [table], L, labels, disks=False)
        fg = out["fg"].view(torch.bool)[:, None].expand(m, n_t, L, L)  # geometry replicated over time, as find_beads
        bg = out["bg"].view(torch.bool)[:, None].expand(m, n_t, L, L)
        per = {"mark": utils.roi_mark_chunk(m, n_c, n_t, L)}
        assay["roi"] = DataArray(out["roi"], ("mark", "channel", "time", "roi_y", "roi_x")).chunk(per)
        row, col = table[:, 0].astype(np.int64), table[:, 1].astype(np.int64)
        top, left = utils.window_origin(row, L, h), utils.window_origin(col, L, w)
        clipped = ((stats[:, 3] < top) | (stats[:, 5] >= top + L) | (stats[:, 4] < left) | (stats[:, 6] >= left + L)).reshape(m)
        area = stats[:, 0].astype(np.float64)
        over_time = lambda v: np.repeat(np.asarray(v)[:, None], n_t, axis=1)  # noqa: E731
        assay = assay.assign_coords(
            fg=DataArray(fg, ("mark", "time", "roi_y", "roi_x")).chunk(per),
            bg=DataArray(bg, ("mark", "time", "roi_y", "roi_x")).chunk(per),
            x=(("mark", "time"), over_time(col.astype(np.float64))),
            y=(("mark", "time"), over_time(row.astype(np.float64))),
            valid=(("mark", "time"), over_time(~clipped)),
            area=(("mark",), stats[:, 0].copy()),
            bbox_top=(("mark",), stats[:, 3].copy()), bbox_left=(("mark",), stats[:, 4].copy()),
            bbox_bottom=(("mark",), stats[:, 5].copy()), bbox_right=(("mark",), stats[:, 6].copy()),
            x_centroid=(("mark",), stats[:, 2] / np.maximum(area, 1)), y_centroid=(("mark",), stats[:, 1] / np.maximum(area, 1)),
            clipped=(("mark",), clipped),
        )
        assay.attrs["blob_threshold"] = float(level)
        assay.attrs["blob_components"] = int(components)
        assay._cache["roi_sums"] = out["sums"]
        assay._cache["roi_counts"] = out["counts"]
        assay._cache["radius"] = table[:, 2].copy()
        return assay

    @registry.components.register("find_blobs")
    def make(threshold="otsu", search_channel=None, polarity="bright", smooth=False, connectivity=8, fill_holes=False,
             min_area=20, max_area=None, clear_border=False, roi_length=None, max_components=1 << 20):
        return BlobFinder(threshold=threshold, search_channel=search_channel, polarity=polarity, smooth=smooth,
                          connectivity=connectivity, fill_holes=fill_holes, min_area=min_area, max_area=max_area,
                          clear_border=clear_border, roi_length=roi_length, max_components=max_components)


class _CallableModule(types.ModuleType):
    """``mg.blobs(data, ...)``: the pipeline of this module's finder (registry.blobs), next to ``mg.beads(data, ...)``."""

    def __call__(self, data, **settings):
        return registry.blobs(data, **settings)


sys.modules[__name__].__class__ = _CallableModule
