"""The contract of mg_roi_unmix_stats and mg_unmix_planes (include/magnify_hip.h) in plain NumPy.

Elementwise operations only, in the stated order -- no ``@`` and no ``dot``: BLAS picks its own order of additions.
Every product is rounded, then every sum, left to right over the used channels; the division is IEEE.  ``np.sort`` on
the order-preserving keys gives the order statistics (so that -0.0 sorts below +0.0, as the radix select has it) and
``math.fsum`` the exact sum."""
from __future__ import annotations

import math

import numpy as np


def volumes(x, matrix):
    """x (n_k, ...) float64, matrix (n_ln, n_k) -> v (n_ln, ...): v_k = (...((w_k0 x_0) + w_k1 x_1) + ...)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(matrix, dtype=np.float64)
    out = np.empty((w.shape[0],) + x.shape[1:], dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(w.shape[0]):
            v = w[k, 0] * x[0]
            for j in range(1, w.shape[1]):
                v = v + w[k, j] * x[j]
            out[k] = v
    return out


def derived(x, matrix):
    """The D = 2 n_ln - 1 derived values of every pixel: v_0 .. v_{n_ln-1}, then r_k = v_k / v_0 for k = 1 .. n_ln-1."""
    v = volumes(x, matrix)
    with np.errstate(all="ignore"):
        r = v[1:] / v[0]
    return np.concatenate([v, r], axis=0)


def keys(values):
    """The order-preserving uint64 image of float64 values: sign bit flipped (positive) or all bits inverted."""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def from_keys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    pos = (k >> np.uint64(63)).astype(bool)
    return np.where(pos, k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def sorted_values(values):
    """The values that take part (not NaN), sorted by key."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    return from_keys(np.sort(keys(v[~np.isnan(v)])))


def exact_sum(values):
    """fsum of finite values; where an infinity takes part, the class numpy's sum gives (inf, -inf or NaN)."""
    v = np.asarray(values, dtype=np.float64)
    if len(v) == 0:
        return 0.0
    if not np.isfinite(v).all():
        with np.errstate(all="ignore"):
            return float(np.sum(v))
    try:
        return math.fsum(v.tolist())
    except OverflowError:  # the sum itself is beyond float64
        with np.errstate(all="ignore"):
            return float(np.sum(v))


def order_pairs(sorted_vals, q):
    """(n_q, 2): {sorted[lo], sorted[hi]} with pos = (n - 1) q, lo = floor(pos), hi = min(lo + 1, n - 1); NaN for n = 0."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    out = np.full((len(q), 2), np.nan)
    n = len(sorted_vals)
    if n:
        for j, f in enumerate(q):
            lo = int(math.floor(float(n - 1) * float(f)))
            out[j] = sorted_vals[lo], sorted_vals[min(lo + 1, n - 1)]
    return out


def window_values(roi, mask, channels, matrix, offset=None):
    """values[g][t][d]: the sorted values that take part of window (g, t) and derived value d.
    roi (m, C, T, L, L); mask None or bool / uint8 broadcastable to (m, T, L, L); offset None or (m, C, T)."""
    roi = np.asarray(roi)
    m, _, n_t, L, _ = roi.shape
    mk = np.ones((m, n_t, L, L), dtype=bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, (m, n_t, L, L))
    out = []
    for g in range(m):
        row = []
        for t in range(n_t):
            sel = mk[g, t]
            x = np.stack([roi[g, c, t][sel].astype(np.float64) - (0.0 if offset is None else np.float64(offset[g, c, t]))
                          for c in channels]) if sel.any() else np.zeros((len(channels), 0))
            row.append([sorted_values(dv) for dv in derived(x, matrix)])
        out.append(row)
    return out


def roi_unmix_stats(roi, mask, channels, matrix, offset=None, q=()):
    """(count int32 (m, T, D), sum float64 (m, T, D) -- the exact sum, rounded once --, order float64 (m, T, D, n_q, 2),
    values) of mg_roi_unmix_stats; ``values`` as ``window_values`` gives them."""
    vals = window_values(roi, mask, channels, matrix, offset)
    m, n_t, d = len(vals), np.asarray(roi).shape[2], 2 * np.asarray(matrix).shape[0] - 1
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    count = np.zeros((m, n_t, d), dtype=np.int32)
    total = np.zeros((m, n_t, d), dtype=np.float64)
    order = np.full((m, n_t, d, len(q), 2), np.nan)
    for g in range(m):
        for t in range(n_t):
            for k in range(d):
                v = vals[g][t][k]
                count[g, t, k] = len(v)
                total[g, t, k] = exact_sum(v)
                order[g, t, k] = order_pairs(v, q)
    return count, total, order, vals


def sum_bound(values):
    """gamma(n - 1) sum |v| + u |sum v|: what any order of summing n float64 terms stays within of the rounded exact sum
    (u = 2^-53, gamma(k) = k u / (1 - k u))."""
    u = 2.0 ** -53
    n = len(values)
    if n == 0:
        return 0.0
    g = (n - 1) * u / (1.0 - (n - 1) * u)
    return g * math.fsum(np.abs(values).tolist()) + u * abs(math.fsum(np.asarray(values).tolist()))


def planes(src, channels, matrix, offset=None, ratios=False):
    """mg_unmix_planes in float64: src (C, T, H, W) -> (n_out, T, H, W); cast with ``.astype(np.float32)``."""
    src = np.asarray(src)
    x = np.stack([src[c].astype(np.float64) - (0.0 if offset is None else np.float64(offset[j]))
                  for j, c in enumerate(channels)])
    return derived(x, matrix) if ratios else volumes(x, matrix)


def nanmedian_windows(roi, mask):
    """roi.where(mask).median over the window, numpy's nanmedian: roi (m, C, T, L, L), mask (m, T, L, L) -> (m, C, T)."""
    roi = np.asarray(roi)
    m, c, n_t = roi.shape[:3]
    mk = np.broadcast_to(np.asarray(mask) != 0, (m, n_t) + roi.shape[3:])
    out = np.full((m, c, n_t), np.nan)
    for g in range(m):
        for t in range(n_t):
            for ch in range(c):
                v = roi[g, ch, t][mk[g, t]].astype(np.float64)
                v = v[~np.isnan(v)]
                if len(v):
                    out[g, ch, t] = np.median(v)
    return out


def interpolate(count, order, q):
    """numpy's linear quantile between the order statistics, operation for operation (reduce.interpolate_quantiles)."""
    qv = np.asarray(q, dtype=np.float64).reshape(-1)
    n = np.asarray(count).astype(np.float64)[..., None]
    pos = (n - 1.0) * qv
    g = pos - np.floor(pos)
    a, b = order[..., 0], order[..., 1]
    with np.errstate(all="ignore"):
        d = b - a
        return np.where(g >= 0.5, b - d * (1.0 - g), a + d * g)


def identify_pixel(roi, fg, bg, matrix, use, q=(0.25, 0.5, 0.75)):
    """identify_mrbles(unmix="pixel") from the dataset's own roi (m, C, T, L, L), fg, bg (m, T, L, L) at time 0:
    (ln_vol, ln_ratio, ln_ratio_spread (m, n_ln), ln_pixels (m,) int32)."""
    roi, fg, bg = np.asarray(roi)[:, :, :1], np.asarray(fg)[:, :1], np.asarray(bg)[:, :1]
    off = nanmedian_windows(roi, bg)
    count, _, order, _ = roi_unmix_stats(roi, fg, use, matrix, off, q)
    quart = interpolate(count, order, q)[:, 0]  # (m, D, 3)
    n_ln = np.asarray(matrix).shape[0]
    vol = quart[:, :n_ln, 1]
    with np.errstate(all="ignore"):
        ratio = np.concatenate([vol[:, :1] / vol[:, :1], quart[:, n_ln:, 1]], axis=1)
        spread = np.concatenate([ratio[:, :1] - ratio[:, :1], (quart[:, n_ln:, 2] - quart[:, n_ln:, 0]) / 2.0], axis=1)
    return vol, ratio, spread, count[:, 0, 0].astype(np.int32)
