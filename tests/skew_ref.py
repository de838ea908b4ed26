"""NumPy restatement of ``rotation="auto"``, independent of magnify_amd/skew.py and of the kernel.

``profiles`` is mg_skew_profiles: integer arithmetic only, int64 ``bincount``.
  * D = min(h, w), nb = D + 2; dy = 2 y - (h - 1), dx = 2 x - (w - 1); a pixel takes part iff dy^2 + dx^2 <= (D - 1)^2.
  * (C, S) = (rint(32768 cos a), rint(32768 sin a)); kr = ((dy C - dx S) >> 16) + nb // 2, kc = ((dx C + dy S) >> 16) +
    nb // 2 (arithmetic shift); sums[a, 0, kr] += q, counts[a, 0, kr] += 1, and the same on axis 1 at kc.
  * q = p for integer pixels; for float pixels t = (p - lo) * scale in float64, q = 0 below 0, 65535 above 65535, else
    floor(t); a NaN pixel is left out.  lo = min, scale = 65535 / (max - min) (0 on a flat plane) unless given.
``score``: the bins with |2 (k - nb // 2) + 1| <= floor(0.8 D); m = sums / counts; sum over both axes of diff(m)^2.
``estimate_rotation``: a coarse pass on the plane binned by b (float32 sums, so quantised), a fine pass of 51 angles on
the plane itself, the vertex of the parabola through the best fine score and its neighbours.
"""
import math

import numpy as np

MAX_ANGLES = 64


def angle_table(angles_deg):
    a = np.radians(np.asarray(angles_deg, dtype=np.float64))
    return np.stack([np.rint(32768.0 * np.cos(a)), np.rint(32768.0 * np.sin(a))], axis=1).astype(np.int32)


def float_range(plane):
    lo, hi = float(plane.min()), float(plane.max())  # (NaN propagates, as in mg_plane_minmax)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("the plane's min / max is not finite")
    return lo, (65535.0 / (hi - lo) if hi > lo else 0.0)


def quantise(plane, lo=None, scale=None):
    """(q int64, valid bool) of every pixel."""
    if plane.dtype.kind == "u":
        return plane.astype(np.int64), np.ones(plane.shape, dtype=bool)
    if lo is None or scale is None:
        lo, scale = float_range(plane)
    p = plane.astype(np.float64)
    valid = ~np.isnan(p)
    with np.errstate(invalid="ignore"):
        t = (np.where(valid, p, 0.0) - np.float64(lo)) * np.float64(scale)
        q = np.where(t < 0, 0.0, np.where(t > 65535.0, 65535.0, np.where(t == t, np.floor(t), 0.0)))
    return q.astype(np.int64), valid


def bin_indices(h, w, cs):
    """(kr, kc, inside) of every pixel for one (C, S)."""
    nb = min(h, w) + 2
    dy = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    dx = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    c, s = int(cs[0]), int(cs[1])
    kr = ((dy * c - dx * s) >> 16) + nb // 2
    kc = ((dx * c + dy * s) >> 16) + nb // 2
    return kr, kc, dy * dy + dx * dx <= (min(h, w) - 1) ** 2


def profiles(plane, angles_deg, lo=None, scale=None):
    """(sums uint64, counts uint32), both (n_angles, 2, nb)."""
    h, w = plane.shape
    nb = min(h, w) + 2
    q, valid = quantise(plane, lo, scale)
    table = angle_table(angles_deg)
    sums = np.zeros((len(table), 2, nb), dtype=np.uint64)
    counts = np.zeros((len(table), 2, nb), dtype=np.uint32)
    take = bin_indices(h, w, table[0])[2] & valid  # (the disk does not depend on the angle)
    weights = q[take].astype(np.float64)  # (exact: a bin holds at most 32768^2 * 65535 < 2^53)
    for a, cs in enumerate(table):
        kr, kc, _ = bin_indices(h, w, cs)
        for axis, k in enumerate((kr, kc)):
            k = np.broadcast_to(k, (h, w))[take]
            assert k.min(initial=0) >= 0 and k.max(initial=0) < nb
            sums[a, axis] = np.bincount(k, weights=weights, minlength=nb).astype(np.uint64)
            counts[a, axis] = np.bincount(k, minlength=nb)
    return sums, counts


def score(sums, counts):
    """(n_angles,) float64."""
    nb = sums.shape[-1]
    k = np.arange(nb)
    keep = np.abs(2 * (k - nb // 2) + 1) <= math.floor(0.8 * (nb - 2))
    m = sums[..., keep].astype(np.float64) / counts[..., keep].astype(np.float64)
    return (np.diff(m, axis=-1) ** 2).sum(axis=(-2, -1))


def bin_plane(plane, b):
    """(h // b, w // b) float32: the block sums, integer pixels exactly, float pixels in float64 (mg_bin_planes)."""
    h, w = plane.shape
    hb, wb = h // b, w // b
    acc = np.int64 if plane.dtype.kind == "u" else np.float64
    return plane[:hb * b, :wb * b].astype(acc).reshape(hb, b, wb, b).sum(axis=(1, 3)).astype(np.float32)


def coarse_bin(feature):
    return next((b for b in (8, 4, 2) if feature / b >= 8), 1)


def coarse_angles(feature, b, d_b, max_angle):
    step = math.degrees((feature / b) / (2 * d_b))
    n = math.ceil(max_angle / step)
    return step, np.arange(-n, n + 1, dtype=np.float64) * step


def vertex(scores, angles):
    """The argmax angle, moved to the vertex of the parabola through it and its neighbours where it is interior and the
    parabola is concave."""
    j = int(np.argmax(scores))
    best = float(angles[j])
    if 0 < j < len(scores) - 1:
        left, mid, right = float(scores[j - 1]), float(scores[j]), float(scores[j + 1])
        curve = left - 2.0 * mid + right
        if curve < 0:
            best += 0.5 * (left - right) / curve * float(angles[j + 1] - angles[j])
    return best


def estimate_rotation(plane, feature, max_angle=10.0):
    """(rotation, confidence): the rotation that puts the grid straight."""
    h, w = plane.shape
    b = coarse_bin(feature)
    coarse = bin_plane(plane, b) if b > 1 else plane
    step, angles = coarse_angles(feature, b, min(coarse.shape), max_angle)
    s = score(*profiles(coarse, angles))
    j = int(np.argmax(s))
    median = float(np.median(s))
    confidence = float(s[j]) / median if median > 0 else 0.0
    fine = float(angles[j]) + np.arange(-25, 26, dtype=np.float64) * (step / 25)
    return vertex(score(*profiles(plane, fine)), fine), confidence
