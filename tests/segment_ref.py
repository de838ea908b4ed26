"""NumPy + scipy.ndimage restatement of mg_roi_threshold_masks (include/magnify_hip.h): the data-driven fg / bg masks of
``segment_rois``.  Written from the contract, one window at a time; the kernel has to equal it bit for bit.

Not in the reference project, whose masks are drawn shapes (find.py:383-400, 561-586)."""
from __future__ import annotations

import numpy as np
import scipy.ndimage as ndi

S = np.ones((3, 3), dtype=bool)


def erode(mask, times):
    """``times`` erosions by S, outside the window off; checked against scipy's own iteration."""
    out = np.asarray(mask, dtype=bool)
    for _ in range(times):
        out = ndi.binary_erosion(out, S, border_value=0)
    if times > 0:
        assert np.array_equal(out, ndi.binary_erosion(mask, S, iterations=times, border_value=0))
    return out


def dilate(mask, times, within=None):
    """``times`` steps of ``x = dilate(x, S) & within``; checked against scipy's masked, iterated dilation."""
    out = np.asarray(mask, dtype=bool)
    for _ in range(times):
        out = ndi.binary_dilation(out, S, border_value=0)
        if within is not None:
            out &= within
    if times > 0:
        # (scipy leaves pixels outside its mask as they were: every caller here starts inside `within`)
        assert np.array_equal(out, ndi.binary_dilation(mask, S, iterations=times, mask=within, border_value=0))
    return out


def opening(on, radius):
    out = dilate(erode(on, radius), radius)
    if radius > 0:
        assert np.array_equal(out, ndi.binary_opening(on, S, iterations=radius))
    return out


def window_range(w):
    """(lo, hi, flat): float64 min / max of the non-NaN pixels; flat = the window is unsegmented."""
    v = np.asarray(w).astype(np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return np.inf, -np.inf, True
    lo, hi = float(v.min()), float(v.max())
    with np.errstate(invalid="ignore", over="ignore"):
        rng = np.float64(hi) - np.float64(lo)
    return lo, hi, not (np.isfinite(rng) and rng > 0)


def bins_of(w, lo, hi):
    """b(v) = floor((255.0 * (v - lo)) / (hi - lo)) in float64 (at most 255), -1 for NaN pixels."""
    v = np.asarray(w).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (255.0 * (v - np.float64(lo))) / (np.float64(hi) - np.float64(lo))
        b = np.minimum(np.floor(u), 255.0)
    return np.where(np.isnan(v), -1, b).astype(np.int64)


def otsu_k(b):
    """k*: the smallest k in 0 .. 254 of the largest (d * d) / (w0 * w1)."""
    h = np.bincount(b[b >= 0].reshape(-1), minlength=256).astype(np.int64)
    n, stot = int(h.sum()), int((np.arange(256) * h).sum())
    w0 = np.cumsum(h)[:255]
    s0 = np.cumsum(np.arange(256) * h)[:255]
    w1 = n - w0
    d = (stot * w0 - n * s0).astype(np.float64)
    ok = (w0 > 0) & (w1 > 0)
    value = np.full(255, -1.0)
    value[ok] = (d[ok] * d[ok]) / (w0[ok] * w1[ok]).astype(np.float64)
    return int(np.argmax(value))


def segment_window(w, fg0, bg0, allowed=None, method="otsu", open_radius=1, max_grow=4, bg_guard=2, min_area=1):
    """One window -> (fg, bg, threshold, (n_fg, n_bg), segmented)."""
    fg0, bg0 = np.asarray(fg0) != 0, np.asarray(bg0) != 0
    lo, hi, flat = window_range(w)

    def fallback(threshold):
        return fg0.copy(), bg0.copy(), threshold, (int(fg0.sum()), int(bg0.sum())), False

    if flat:
        return fallback(np.nan)
    if method == "otsu":
        b = bins_of(w, lo, hi)
        k = otsu_k(b)
        on = b > k
        threshold = np.float64(lo) + ((k + 1) * (np.float64(hi) - np.float64(lo))) / 255.0
    else:
        v = np.asarray(w).astype(np.float64)
        with np.errstate(invalid="ignore"):
            on = v > np.float64(method)
        threshold = np.float64(method)
    opened = opening(on, open_radius)
    if allowed is not None:
        opened = opened & (np.asarray(allowed) != 0)
    fg = dilate(opened & fg0, max_grow, within=opened)
    if int(fg.sum()) < max(int(min_area), 1):
        return fallback(float(threshold))
    bg = bg0 & ~dilate(on | fg, bg_guard)
    return fg, bg, float(threshold), (int(fg.sum()), int(bg.sum())), True


def segment(roi, fg0, bg0, allowed=None, **kw):
    """roi (M, T, L, L) of one channel; fg0 / bg0 / allowed (M, T', L, L) with T' = T or 1 ->
    fg, bg uint8 (M, T, L, L), threshold float64 (M, T), counts int32 (M, T, 2), segmented uint8 (M, T)."""
    roi = np.asarray(roi)
    m, n_t, L, _ = roi.shape
    fg = np.zeros((m, n_t, L, L), dtype=np.uint8)
    bg = np.zeros((m, n_t, L, L), dtype=np.uint8)
    thr = np.zeros((m, n_t), dtype=np.float64)
    counts = np.zeros((m, n_t, 2), dtype=np.int32)
    seg = np.zeros((m, n_t), dtype=np.uint8)

    def at(mask, g, t):
        return None if mask is None else np.asarray(mask)[g, t if np.asarray(mask).shape[1] > 1 else 0]

    for g in range(m):
        for t in range(n_t):
            f, b, thr[g, t], counts[g, t], seg[g, t] = segment_window(roi[g, t], at(fg0, g, t), at(bg0, g, t),
                                                                       at(allowed, g, t), **kw)
            fg[g, t], bg[g, t] = f, b
    return fg, bg, thr, counts, seg
