"""NumPy restatement of the hot-pixel removal (``mg_despeckle_planes`` / ``mg_outlier_votes``,
``magnify_amd.despeckle``), written from the contract (include/magnify_hip.h, "Hot pixels"), not from the kernels: the
plane is padded by edge replication, the (2k + 1)^2 shifted views are stacked, ``np.sort`` on the last axis puts every
NaN behind +inf and the middle element is the window median; the outlier test, the replacement, the counts and the
votes are float64 / integer NumPy expressions.  Planes are (..., H, W): every leading index is a plane of its own."""
from __future__ import annotations

import math

import numpy as np

WHICH = ("bright", "dark", "both", "all")


def median(planes, k):
    """The window median of every pixel, window 2k + 1, edges replicated; the planes' dtype.  (..., H, W): every
    leading index is a plane of its own."""
    planes = np.asarray(planes)
    h, w = planes.shape[-2:]
    padded = np.pad(planes, [(0, 0)] * (planes.ndim - 2) + [(k, k), (k, k)], mode="edge")
    views = [padded[..., dy:dy + h, dx:dx + w] for dy in range(2 * k + 1) for dx in range(2 * k + 1)]
    ordered = np.sort(np.stack(views, axis=-1), axis=-1)
    return np.ascontiguousarray(ordered[..., ((2 * k + 1) ** 2 - 1) // 2])


def median_banded(plane, k, bands=16):
    """``median`` of one large plane (H, W), taken band by band in a thread pool (np.sort releases the interpreter
    lock): a band of rows with k rows of the plane on either side has the plane's own medians in its inner rows, and
    the first and last band keep the plane's replicated edge."""
    from concurrent.futures import ThreadPoolExecutor

    plane = np.asarray(plane)
    h = plane.shape[0]
    cuts = [h * i // bands for i in range(bands + 1)]

    def band(i):
        y0, y1 = cuts[i], cuts[i + 1]
        lo, hi = max(y0 - k, 0), min(y1 + k, h)
        return median(plane[lo:hi], k)[y0 - lo:y0 - lo + (y1 - y0)]

    with ThreadPoolExecutor(max_workers=bands) as pool:
        return np.concatenate(list(pool.map(band, range(bands))), axis=0)


def flags(planes, k, which, threshold, med=None):
    """bool (..., H, W): the outlier test.  d = float64(pixel) - float64(median); strict; False wherever d is NaN.
    ``med``: the planes' ``median(planes, k)`` where the caller has it already."""
    planes = np.asarray(planes)
    if which == "all":
        return np.ones(planes.shape, dtype=bool)
    med = median(planes, k) if med is None else med
    with np.errstate(invalid="ignore"):
        d = planes.astype(np.float64) - med.astype(np.float64)
        bright, dark = d > np.float64(threshold), -d > np.float64(threshold)
    return {"bright": bright, "dark": dark, "both": bright | dark}[which]


def remove(planes, k, which="bright", threshold=0.0, defects=None, med=None):
    """-> (out (..., H, W), counts int64 (...)): the median where the condition holds (the defect map (H, W) if there
    is one, else the outlier test), the pixel itself elsewhere; counts = the pixels of every plane for which it held."""
    planes = np.asarray(planes)
    med = median(planes, k) if med is None else med
    if defects is not None:
        cond = np.broadcast_to(np.asarray(defects) != 0, planes.shape)
    else:
        cond = flags(planes, k, which, threshold, med)
    return np.where(cond, med, planes).astype(planes.dtype), cond.sum(axis=(-2, -1), dtype=np.int64)


def votes(block, k, which, threshold, med=None):
    """int32 (H, W): in how many planes of the block (N, H, W) every pixel passes the outlier test."""
    return flags(block, k, which, threshold, med).sum(axis=0, dtype=np.int32)


def defect_map(block, k, which, threshold, min_fraction=0.5):
    n = np.asarray(block).shape[0]
    return votes(block, k, which, threshold) >= max(1, math.ceil(min_fraction * n))


def same(a, b) -> bool:
    """Equality of pixel arrays by value: shape and dtype equal, NaN equals NaN, -0.0 equals 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def random_planes(rng, dtype, shape, specks=0.01):
    """Planes of smooth-ish noise around a mid level (integers: mid-range +- 1/16 of the range; floats: -100 +- 50, so
    there are negative values) with about ``specks`` of the pixels pushed far up or down.  -> (block, a threshold that
    some but not all specks pass at either radius)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        top = np.iinfo(dtype).max
        base = rng.integers(top // 2 - top // 16, top // 2 + top // 16 + 1, size=shape).astype(np.int64)
        jump, threshold = top // 4, top // 4 + top // 16 + 0.5
    else:
        base = rng.normal(-100.0, 50.0, size=shape)
        jump, threshold = 400.0, 480.25
    hit = rng.random(shape) < specks
    sign = np.where(rng.random(shape) < 0.5, -1, 1)
    size = jump * (1 + rng.random(shape))  # the jump and up to twice it: some specks stay below the threshold
    block = np.where(hit, base + sign * size, base)
    if dtype.kind == "u":
        block = np.clip(np.rint(block), 0, top)
    return block.astype(dtype), float(threshold)
