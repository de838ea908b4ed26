"""Hot pixels: compare every pixel with the median of its window and replace the ones that stand out, on the device
(not in the reference, whose finders scale every plane by its global minimum and maximum, utils.py:20-27, so that one
saturated pixel sets the grey scale of the whole plane; DESIGN.md, "Despeckle").

Planes are a device tensor ``(..., H, W)`` of uint8, uint16, float32 or float64.  ``median`` is the plain window median
filter (``scipy.ndimage.median_filter(mode="nearest")``); ``remove_outliers`` replaces the pixels that are more than
``threshold`` above (``which="bright"``), below ("dark") or away from ("both") their window median, or the pixels of a
defect map; ``outlier_votes`` counts, per pixel, the planes in which it stands out, and ``defect_map`` turns the votes
of the planes of one sensor into a map of its fixed defects.  The component ``remove_outliers`` does this to the tiles
of a DataArray / Dataset directly after ``standardize_format``; the pipelines take it as ``despeckle=``.  Both kernels
are in ``mg_despeckle.hip``; ``tests/despeckle_ref.py`` restates the contract in NumPy.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as nat
from . import registry
from ._dataset import page_view, plane_block
from .utils import int_in, number

TILE = nat.DEFINES["MG_DESPECKLE_TILE"]  # the output tile of a workgroup (TILE x TILE pixels)
MAX_K = nat.DEFINES["MG_DESPECKLE_MAX_K"]
RADII = tuple(range(1, MAX_K + 1))
WHICH = {"bright": nat.DEFINES["MG_OUTLIER_BRIGHT"], "dark": nat.DEFINES["MG_OUTLIER_DARK"],
         "both": nat.DEFINES["MG_OUTLIER_BOTH"]}
ALL = nat.DEFINES["MG_OUTLIER_ALL"]  # every pixel becomes its window median: ``median``, and background's ``smooth=``
SCOPES = ("plane", "sensor")


def check_despeckle(threshold, radius=1, which="bright", scope="plane", min_fraction=0.5):
    """The settings of ``remove_outliers`` as the pipelines take them: ``threshold`` a finite real number >= 0 (in pixel
    units), ``radius`` 1 or 2, ``which`` "bright", "dark" or "both", ``scope`` "plane" or "sensor", ``min_fraction`` in
    (0, 1].  ValueError otherwise."""
    if number("despeckle threshold", threshold) < 0:
        raise ValueError(f"despeckle threshold must be >= 0, got {threshold!r}")
    int_in("despeckle radius", radius, 1, MAX_K)
    if not isinstance(which, str) or which not in WHICH:
        raise ValueError(f"despeckle which must be one of {tuple(WHICH)}, got {which!r}")
    if not isinstance(scope, str) or scope not in SCOPES:
        raise ValueError(f"despeckle scope must be one of {SCOPES}, got {scope!r}")
    if not 0 < number("despeckle min_fraction", min_fraction) <= 1:
        raise ValueError(f"despeckle min_fraction must be in (0, 1], got {min_fraction!r}")


def _replace(b, radius, which, threshold, defects, want_counts):
    from . import hotpath

    out = torch.empty_like(b.block)
    counts = torch.empty(b.lead, dtype=torch.int64, device=b.block.device) if want_counts else None  # (the entry zeroes it)
    if b.block.numel() == 0:
        return out, None if counts is None else counts.zero_()
    hotpath._call("mg_despeckle_planes", b.block.data_ptr(), out.data_ptr(), b.code, b.n, b.h, b.w, radius, which,
                  float(threshold), hotpath._ptr(defects), hotpath._ptr(counts), hotpath._stream())
    return out, counts


def median(planes, radius=1):
    """(..., H, W) -> the window median of every pixel, window 2 * radius + 1, edges replicated."""
    check_despeckle(0, radius)
    out, _ = _replace(plane_block(planes, "despeckle.median"), radius, ALL, 0.0, None, False)
    return out


def remove_outliers(planes, threshold, radius=1, which="bright", defects=None, want_counts=True):
    """-> (out (..., H, W), counts (...) int64 or None).  A pixel becomes its window median where pixel - median >
    ``threshold`` ("bright"), median - pixel > ``threshold`` ("dark") or either ("both"), in float64, strictly; a pixel
    or a median that is NaN leaves the pixel alone.  With ``defects`` (bool / uint8 (H, W), a tensor or an array, one map
    for all planes) exactly the mapped pixels are replaced and ``threshold`` / ``which`` play no part.  ``counts``: the
    pixels replaced in every plane."""
    check_despeckle(threshold, radius, which)
    b = plane_block(planes, "despeckle.remove_outliers")
    if defects is not None:
        if not isinstance(defects, torch.Tensor):
            defects = torch.from_numpy(np.ascontiguousarray(defects))
        if defects.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"a defect map is bool or uint8, got {defects.dtype}")
        if tuple(defects.shape) != (b.h, b.w):
            raise ValueError(f"the defect map must have the planes' shape {(b.h, b.w)}, got {tuple(defects.shape)}")
        defects = defects.to(device=b.block.device, dtype=torch.uint8).contiguous()
    return _replace(b, radius, WHICH[which], threshold, defects, want_counts)


def outlier_votes(planes, threshold, radius=1, which="bright"):
    """-> int32 (H, W): in how many of the leading planes every pixel passes the outlier test of ``remove_outliers``."""
    from . import hotpath

    check_despeckle(threshold, radius, which)
    b = plane_block(planes, "despeckle.outlier_votes")
    votes = torch.empty((b.h, b.w), dtype=torch.int32, device=b.block.device)  # (the entry zeroes it)
    if b.block.numel() == 0:
        return votes.zero_()
    hotpath._call("mg_outlier_votes", b.block.data_ptr(), b.code, b.n, b.h, b.w, radius, WHICH[which], float(threshold),
                  votes.data_ptr(), hotpath._stream())
    return votes


def defect_map(planes, threshold, radius=1, which="bright", min_fraction=0.5):
    """-> bool (H, W): the pixels that stand out in at least max(1, ceil(min_fraction * n)) of the n planes -- the fixed
    defects of the sensor all planes were taken with, as opposed to a speck in one of them."""
    check_despeckle(threshold, radius, which, min_fraction=min_fraction)
    n = int(np.prod(planes.shape[:-2], dtype=np.int64)) if isinstance(planes, torch.Tensor) else 0
    return outlier_votes(planes, threshold, radius, which) >= max(1, math.ceil(min_fraction * n))


@registry.component("remove_outliers")
def remove_outliers_component(xp, threshold, radius=1, which="bright", scope="plane", min_fraction=0.5):
    """Replace the hot pixels of the tiles (a DataArray, or the ``tile`` of a Dataset) by their window medians.  The
    pages are ``tile_y`` / ``tile_x`` or ``y`` / ``x``; every other dimension counts planes.  ``scope`` "plane" tests
    every plane on its own; "sensor" first votes over all planes (channels, timepoints and tiles of one acquisition
    share the sensor), maps the pixels that stand out in at least ``min_fraction`` of them and replaces exactly those in
    every plane -- a speck in a single plane stays, a fixed defect goes even where a bright marker hides it from the
    per-plane test.  Every dimension, coordinate and attribute is kept; ``attrs["despeckle_replaced"]`` is the number
    of pixels replaced and, for "sensor", ``attrs["despeckle_defects"]`` the number of pixels in the map."""
    check_despeckle(threshold, radius, which, scope, min_fraction)
    view = page_view(xp, "tile", (("tile_y", "tile_x"), ("y", "x")), "remove_outliers")
    extra = {}
    defects = None
    if scope == "sensor":
        defects = defect_map(view.planes, threshold, radius, which, min_fraction)
        extra["despeckle_defects"] = int(defects.sum().item())
    out, counts = remove_outliers(view.planes, threshold, radius, which, defects=defects)
    extra["despeckle_replaced"] = int(counts.sum().item())
    return view.rebuild(out, extra)
