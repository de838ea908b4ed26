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
import numbers

import numpy as np
import torch

from . import _native as nat
from . import registry, xr_lite
from .xr_lite import DataArray

TILE = nat.DEFINES["MG_DESPECKLE_TILE"]  # the output tile of a workgroup (TILE x TILE pixels)
MAX_K = nat.DEFINES["MG_DESPECKLE_MAX_K"]
RADII = tuple(range(1, MAX_K + 1))
WHICH = {"bright": nat.DEFINES["MG_OUTLIER_BRIGHT"], "dark": nat.DEFINES["MG_OUTLIER_DARK"],
         "both": nat.DEFINES["MG_OUTLIER_BOTH"]}
_ALL = nat.DEFINES["MG_OUTLIER_ALL"]
SCOPES = ("plane", "sensor")


def check_despeckle(threshold, radius=1, which="bright", scope="plane", min_fraction=0.5):
    """The settings of ``remove_outliers`` as the pipelines take them: ``threshold`` a finite real number >= 0 (in pixel
    units), ``radius`` 1 or 2, ``which`` "bright", "dark" or "both", ``scope`` "plane" or "sensor", ``min_fraction`` in
    (0, 1].  ValueError otherwise."""
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, numbers.Real):
        raise ValueError(f"despeckle threshold must be a real number, got {threshold!r}")
    if not math.isfinite(threshold) or threshold < 0:
        raise ValueError(f"despeckle threshold must be finite and >= 0, got {threshold!r}")
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or radius not in RADII:
        raise ValueError(f"despeckle radius must be one of {RADII}, got {radius!r}")
    if not isinstance(which, str) or which not in WHICH:
        raise ValueError(f"despeckle which must be one of {tuple(WHICH)}, got {which!r}")
    if not isinstance(scope, str) or scope not in SCOPES:
        raise ValueError(f"despeckle scope must be one of {SCOPES}, got {scope!r}")
    if (isinstance(min_fraction, (bool, np.bool_)) or not isinstance(min_fraction, numbers.Real)
            or not 0 < min_fraction <= 1):
        raise ValueError(f"despeckle min_fraction must be in (0, 1], got {min_fraction!r}")


def _block(planes, what):
    """-> (the planes as a contiguous tensor, leading shape, n, h, w, dtype code).  Raises before any launch."""
    from . import hotpath

    if not isinstance(planes, torch.Tensor):
        raise TypeError(f"{what} takes a device tensor (..., H, W), got {type(planes).__name__}")
    code = nat.dtype_code(planes.dtype)  # TypeError for an unsupported dtype
    if planes.dim() < 2:
        raise ValueError(f"{what} takes planes (..., H, W), got shape {tuple(planes.shape)}")
    hotpath.require_gpu()
    if not planes.is_cuda:
        raise ValueError(f"{what} takes a device tensor; move it with preprocess.to_device")
    lead = tuple(planes.shape[:-2])
    h, w = (int(v) for v in planes.shape[-2:])
    return planes.contiguous(), lead, int(np.prod(lead, dtype=np.int64)), h, w, code


def _replace(block, lead, n, h, w, code, radius, which, threshold, defects, want_counts):
    from . import hotpath

    out = torch.empty_like(block)
    counts = torch.empty(lead, dtype=torch.int64, device=block.device) if want_counts else None  # (the entry zeroes it)
    if block.numel() == 0:
        return out, None if counts is None else counts.zero_()
    hotpath._call("mg_despeckle_planes", block.data_ptr(), out.data_ptr(), code, n, h, w, radius, which, float(threshold),
                  hotpath._ptr(defects), hotpath._ptr(counts), hotpath._stream())
    return out, counts


def median(planes, radius=1):
    """(..., H, W) -> the window median of every pixel, window 2 * radius + 1, edges replicated."""
    check_despeckle(0, radius)
    out, _ = _replace(*_block(planes, "despeckle.median"), radius, _ALL, 0.0, None, False)
    return out


def remove_outliers(planes, threshold, radius=1, which="bright", defects=None, want_counts=True):
    """-> (out (..., H, W), counts (...) int64 or None).  A pixel becomes its window median where pixel - median >
    ``threshold`` ("bright"), median - pixel > ``threshold`` ("dark") or either ("both"), in float64, strictly; a pixel
    or a median that is NaN leaves the pixel alone.  With ``defects`` (bool / uint8 (H, W), a tensor or an array, one map
    for all planes) exactly the mapped pixels are replaced and ``threshold`` / ``which`` play no part.  ``counts``: the
    pixels replaced in every plane."""
    check_despeckle(threshold, radius, which)
    block, lead, n, h, w, code = _block(planes, "despeckle.remove_outliers")
    if defects is not None:
        if not isinstance(defects, torch.Tensor):
            defects = torch.from_numpy(np.ascontiguousarray(defects))
        if defects.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"a defect map is bool or uint8, got {defects.dtype}")
        if tuple(defects.shape) != (h, w):
            raise ValueError(f"the defect map must have the planes' shape {(h, w)}, got {tuple(defects.shape)}")
        defects = defects.to(device=block.device, dtype=torch.uint8).contiguous()
    return _replace(block, lead, n, h, w, code, radius, WHICH[which], threshold, defects, want_counts)


def outlier_votes(planes, threshold, radius=1, which="bright"):
    """-> int32 (H, W): in how many of the leading planes every pixel passes the outlier test of ``remove_outliers``."""
    from . import hotpath

    check_despeckle(threshold, radius, which)
    block, _, n, h, w, code = _block(planes, "despeckle.outlier_votes")
    votes = torch.empty((h, w), dtype=torch.int32, device=block.device)  # (the entry zeroes it)
    if block.numel() == 0:
        return votes.zero_()
    hotpath._call("mg_outlier_votes", block.data_ptr(), code, n, h, w, radius, WHICH[which], float(threshold),
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
    from .preprocess import to_device

    check_despeckle(threshold, radius, which, scope, min_fraction)
    xp = xr_lite.from_any(xp)
    is_array = isinstance(xp, DataArray)
    if not is_array and "tile" not in xp.data_vars:
        raise ValueError("remove_outliers: the Dataset has no 'tile' variable")
    tile = xp if is_array else xp.data_vars["tile"]
    pages = next((p for p in (("tile_y", "tile_x"), ("y", "x")) if p[0] in tile.dims and p[1] in tile.dims), None)
    if pages is None:
        raise ValueError(f"remove_outliers: no page dimensions (tile_y, tile_x) or (y, x) in {tile.dims}")
    lead = tuple(d for d in tile.dims if d not in pages)
    data = tile.transpose(*lead, *pages).data
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data)
    planes = to_device(data)
    extra = {}
    defects = None
    if scope == "sensor":
        defects = defect_map(planes, threshold, radius, which, min_fraction)
        extra["despeckle_defects"] = int(defects.sum().item())
    out, counts = remove_outliers(planes, threshold, radius, which, defects=defects)
    extra["despeckle_replaced"] = int(counts.sum().item())
    cleaned = DataArray(out, lead + pages, None, tile.name, tile.attrs).transpose(*tile.dims)
    if is_array:
        return DataArray(cleaned.raw, tile.dims, dict(xp.coords), xp.name, dict(xp.attrs, **extra))
    res = xp.copy()
    res.attrs.update(extra)
    res["tile"] = cleaned
    return res
