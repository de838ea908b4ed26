"""NumPy + scipy.ndimage restatement of the blob contracts (include/magnify_hip.h "Blobs", magnify_amd/blobs.py):
``label`` with its statistics, ``select`` with the marker table, ``fill_holes``, the Otsu front end and the whole
``find_blobs`` component.  Written from the contracts, not from the kernels; the device has to equal it exactly.

Not in the reference project, whose finders are circle finders."""
from __future__ import annotations

import math

import numpy as np
import scipy.ndimage as ndi

from segment_ref import bins_of, otsu_k

S4 = ndi.generate_binary_structure(2, 1)
S8 = np.ones((3, 3), dtype=bool)
STATS = ("area", "sum_y", "sum_x", "y_min", "x_min", "y_max", "x_max", "first_pixel")


def on_mask(plane, threshold, below=False):
    """(double)v > threshold, or < with ``below``; NaN is never on."""
    v = np.asarray(plane).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return v < float(threshold) if below else v > float(threshold)


def label_mask(on, connectivity=8):
    """-> (int32 map: -1 off, else 0 .. K-1; K; int64 (K, 8) statistics).  scipy numbers components in raster order of
    their first pixel for both structures: asserted here, every time."""
    on = np.asarray(on, dtype=bool)
    h, w = on.shape
    lab, k = ndi.label(on, S8 if connectivity == 8 else S4)
    labels = lab.astype(np.int32) - 1
    stats = np.zeros((k, 8), dtype=np.int64)
    if k:
        ys, xs = np.nonzero(on)
        ids = labels[ys, xs]
        stats[:, 0] = np.bincount(ids, minlength=k)
        np.add.at(stats[:, 1], ids, ys)
        np.add.at(stats[:, 2], ids, xs)
        for i, sl in enumerate(ndi.find_objects(lab)):
            stats[i, 3:7] = sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1
        lin = ys.astype(np.int64) * w + xs  # ascending: np.nonzero walks in raster order
        first = np.full(k, h * w, dtype=np.int64)
        np.minimum.at(first, ids, lin)
        stats[:, 7] = first
        assert np.all(np.diff(first) > 0), "scipy.ndimage.label did not number in raster order of the first pixels"
    return labels, k, stats


def label(plane, threshold, below=False, connectivity=8):
    return label_mask(on_mask(plane, threshold, below), connectivity)


def radius(area: int) -> int:
    """The largest r with 355 (2 r - 1)^2 <= 452 area: the nearest integer to sqrt(area / pi), pi as 355 / 113."""
    return (math.isqrt(452 * int(area) // 355) + 1) // 2


def select(labels, stats, min_area=1, max_area=None, clear_border=False):
    """-> (map with kept components renumbered in order, rejected -2, off -1; kept statistics; int32 (M, 3) table)."""
    h, w = labels.shape
    keep = stats[:, 0] >= max(min_area, 1)
    if max_area is not None:
        keep &= stats[:, 0] <= max_area
    if clear_border:
        keep &= (stats[:, 3] > 0) & (stats[:, 4] > 0) & (stats[:, 5] < h - 1) & (stats[:, 6] < w - 1)
    new = np.where(keep, np.cumsum(keep) - 1, -2).astype(np.int32)
    out = np.where(labels >= 0, new[np.maximum(labels, 0)] if len(new) else -2, -1).astype(np.int32)
    kept = stats[keep]
    table = np.zeros((len(kept), 3), dtype=np.int32)
    for i, s in enumerate(kept.tolist()):
        a = s[0]
        table[i] = (2 * s[1] + a) // (2 * a), (2 * s[2] + a) // (2 * a), radius(a)
    return out, kept, table


def fill_holes(on):
    return ndi.binary_fill_holes(np.asarray(on) != 0)


def otsu_plane(plane):
    """-> (uint8 plane of ``to_uint8``, Otsu level k, lo, hi); None where the plane is flat."""
    v = np.asarray(plane).astype(np.float64)
    lo, hi = float(v.min()), float(v.max())
    if not (np.isfinite(hi - lo) and hi > lo):
        return None
    b = bins_of(plane, lo, hi)
    return b.astype(np.uint8), otsu_k(b), lo, hi


def auto_roi_length(stats) -> int:
    if len(stats) == 0:
        return 8
    side = int(max((stats[:, 5] - stats[:, 3]).max(), (stats[:, 6] - stats[:, 4]).max())) + 1
    return side + 8 if (side + 8) % 2 == 0 else side + 9


def component(image, threshold="otsu", search_channel=0, polarity="bright", connectivity=8, fill=False, min_area=20,
              max_area=None, clear_border=False, roi_length=None):
    """``find_blobs`` on a host image (channel, time, y, x) (no ``smooth``: the blur has its own oracle) -> dict of what
    the component has to put on the dataset."""
    from magnify_amd.utils import bounding_box

    image = np.asarray(image)
    n_c, n_t, h, w = image.shape
    plane = image[search_channel, 0]
    dark = polarity == "dark"
    if threshold == "otsu":
        front = otsu_plane(plane)
        if front is None:
            on, level = None, float("nan")
        else:
            u8, k, lo, hi = front
            on = u8 <= k if dark else u8 > k
            level = lo + (k + 1) * (hi - lo) / 255
    else:
        on, level = on_mask(plane, threshold, dark), float(threshold)
    if on is None:
        labels, components = np.full((h, w), -1, dtype=np.int32), 0
        kept, table = np.zeros((0, 8), dtype=np.int64), np.zeros((0, 3), dtype=np.int32)
    else:
        if fill:
            on = fill_holes(on)
        labels, components, stats = label_mask(on, connectivity)
        labels, kept, table = select(labels, stats, min_area, max_area, clear_border)
    m = len(table)
    L = min(roi_length if roi_length is not None else auto_roi_length(kept), h, w)
    roi = np.zeros((m, n_c, n_t, L, L), dtype=image.dtype)
    fg, bg = np.zeros((m, n_t, L, L), dtype=bool), np.zeros((m, n_t, L, L), dtype=bool)
    clipped = np.zeros(m, dtype=bool)
    for i, (row, col, _) in enumerate(table.tolist()):
        top, bottom, left, right = bounding_box(col, row, L, w, h)
        roi[i] = image[:, :, top:bottom, left:right]
        fg[i] = labels[top:bottom, left:right] == i
        bg[i] = labels[top:bottom, left:right] == -1
        clipped[i] = kept[i, 3] < top or kept[i, 5] >= bottom or kept[i, 4] < left or kept[i, 6] >= right
    rep = lambda v: np.repeat(np.asarray(v)[:, None], n_t, axis=1)  # noqa: E731
    return {"roi": roi, "fg": fg, "bg": bg, "x": rep(table[:, 1].astype(np.float64)), "y": rep(table[:, 0].astype(np.float64)),
            "valid": rep(~clipped), "clipped": clipped, "area": kept[:, 0], "bbox_top": kept[:, 3], "bbox_left": kept[:, 4],
            "bbox_bottom": kept[:, 5], "bbox_right": kept[:, 6],
            "x_centroid": kept[:, 2] / np.maximum(kept[:, 0], 1).astype(np.float64),
            "y_centroid": kept[:, 1] / np.maximum(kept[:, 0], 1).astype(np.float64),
            "blob_threshold": level, "blob_components": components, "labels": labels, "table": table, "roi_length": L}
