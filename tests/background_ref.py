"""NumPy restatement of the background rule (``mg_background_planes``, ``magnify_amd.background``), written from the
contract (include/magnify_hip.h, "Background"), not from the kernels.  The window of a pixel is the (2R + 1)^2 square
centred on it; positions outside the plane and NaN pixels are left out, a window with nothing left is NaN.  Erosion E =
the minimum of the filtered plane F over the window, opening B = the maximum of E over the window; ``subtract`` is
P - B where P > B, else 0, in the planes' dtype, NaN where either is.  Minimum and maximum over a square are
separable: every pass is a 1-D sliding window (``sliding_window_view``) over a float64 copy padded with NaN, reduced
with ``nanmin`` / ``nanmax`` -- exact for all four dtypes, whose values float64 holds.  Planes are (..., H, W): every
leading index is a plane of its own."""
from __future__ import annotations

import warnings

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def _slide(a, radius, axis, reduce):
    """float64 (..., H, W) -> the nan-reduction of every window i - radius .. i + radius along ``axis``."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (radius, radius)
    padded = np.pad(a, pad, mode="constant", constant_values=np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "All-NaN slice encountered": the answer is NaN, as the rule says
        return reduce(sliding_window_view(padded, 2 * radius + 1, axis=axis), axis=-1)


def erode(planes, radius):
    """float64 E of planes (..., H, W) of any dtype."""
    a = np.asarray(planes).astype(np.float64)
    return _slide(_slide(a, radius, -1, np.nanmin), radius, -2, np.nanmin)


def dilate(planes, radius):
    a = np.asarray(planes).astype(np.float64)
    return _slide(_slide(a, radius, -2, np.nanmax), radius, -1, np.nanmax)


def opening(planes, radius):
    """B of F = ``planes``, in their dtype."""
    planes = np.asarray(planes)
    return np.ascontiguousarray(dilate(erode(planes, radius), radius).astype(planes.dtype))


def filtered(planes, smooth):
    """F: the planes themselves (smooth = 0) or their window median of radius ``smooth`` (tests/despeckle_ref.py)."""
    if smooth == 0:
        return np.asarray(planes)
    import despeckle_ref

    return despeckle_ref.median(planes, smooth)


def estimate(planes, radius, smooth=0):
    return opening(filtered(planes, smooth), radius)


def minus(planes, background):
    """P - B where P > B, else 0, in the dtype; NaN where P or B is NaN."""
    p, b = np.asarray(planes), np.asarray(background)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(p > b, p - b, p.dtype.type(0)).astype(p.dtype)
    if p.dtype.kind == "f":
        out[np.isnan(p) | np.isnan(b)] = np.nan
    return out


def subtract(planes, radius, smooth=0, background=None):
    return minus(planes, estimate(planes, radius, smooth) if background is None else background)


def opening_by_shifts(plane, radius):
    """``opening`` of one large NaN-free plane (H, W) in its own dtype, without the float64 copy: every pass folds the
    2 * radius + 1 shifted slices of the plane with np.minimum / np.maximum, a slice that would leave the plane cut to
    what is inside.  For small radii on planes of many megapixels."""
    def fold(a, axis, op):
        out = a.copy()
        n = a.shape[axis]
        for d in range(1, min(radius, n - 1) + 1):
            lo, hi = [slice(None)] * 2, [slice(None)] * 2
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            lo, hi = tuple(lo), tuple(hi)
            op(out[lo], a[hi], out=out[lo])  # position i takes in i + d
            op(out[hi], a[lo], out=out[hi])  # position i + d takes in i
        return out

    plane = np.asarray(plane)
    e = fold(fold(plane, 1, np.minimum), 0, np.minimum)
    return fold(fold(e, 0, np.maximum), 1, np.maximum)


def same(a, b) -> bool:
    """Equality of pixel arrays by value: shape and dtype equal, NaN equals NaN, -0.0 equals 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
