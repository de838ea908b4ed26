"""NumPy / Python oracle of the masked ROI statistics (mg_roi_masked_stats, ``hotpath.masked_stats``) and the error
bounds its tests hold the kernel to.  A pixel takes part iff its mask is set and it is not NaN.

Per window: ``n``; for integer pixels the exact ``sum`` and ``sum of squares`` as Python ints (so m2 is an exact
``Fraction``); for float pixels ``np.longdouble`` sums; ``min`` / ``max``; ``np.sort`` of the survivors for the order
statistics; ``np.nanquantile`` of the float64 NaN copy for the interpolated value."""
import warnings
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit roundoff of float64
LD = np.longdouble


def survivors(values, mask):
    v = np.asarray(values).reshape(-1)
    keep = np.asarray(mask).reshape(-1) != 0
    if v.dtype.kind == "f":
        keep = keep & ~np.isnan(v)
    return v[keep]


def ranks(n, q):
    """(lo, hi) of numpy's linear method: pos = (n - 1) q in float64, lo = floor(pos), hi = min(lo + 1, n - 1)."""
    pos = np.float64(n - 1) * np.asarray(q, dtype=np.float64)
    lo = np.floor(pos).astype(np.int64)
    return lo, np.minimum(lo + 1, n - 1)


def window(values, mask, q=()):
    """The oracle's record of one window: values (L, L) of uint8 / uint16 / float32 / float64, mask (L, L)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    x = survivors(values, mask)
    n = int(x.size)
    rec = {"n": n, "integer": x.dtype.kind == "u"}
    if rec["integer"]:
        wide = x.astype(object)  # Python ints
        rec["sum"] = int(wide.sum()) if n else 0
        rec["sumsq"] = int((wide * wide).sum()) if n else 0
        rec["m2"] = Fraction(rec["sumsq"]) - Fraction(rec["sum"] ** 2, n) if n else Fraction(0)
        rec["abs_sum"] = rec["sum"]
    else:
        wide = x.astype(LD)
        with np.errstate(invalid="ignore", over="ignore"):
            rec["sum"] = wide.sum() if n else LD(0)
            rec["abs_sum"] = np.abs(wide).sum() if n else LD(0)
            mean = rec["sum"] / LD(n) if n else LD(0)
            rec["m2"] = ((wide - mean) ** 2).sum() if n else LD(0)
    rec["min"] = float(x.min()) if n else np.nan
    rec["max"] = float(x.max()) if n else np.nan
    rec["constant"] = bool(n and (x == x[0]).all())
    rec["finite"] = bool(np.isfinite(x.astype(np.float64)).all())
    s = np.sort(x).astype(np.float64)
    order = np.full((len(q), 2), np.nan)
    if n and len(q):
        lo, hi = ranks(n, q)
        order[:, 0], order[:, 1] = s[lo], s[hi]
    rec["order"] = order
    v64 = np.where(np.asarray(mask).reshape(-1) != 0, np.asarray(values).reshape(-1).astype(np.float64), np.nan)
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        rec["quantile"] = np.nanquantile(v64, q) if len(q) else np.empty(0)
        rec["nanvar"] = np.nanvar(v64) if n else np.nan
    return rec


def stack(roi, mask, q=()):
    """Records of every window of roi (M, C, T, L, L) under mask (M, L, L) or (M, T or 1, L, L): a nested list [g][c][t]."""
    roi, mask = np.asarray(roi), np.asarray(mask)
    if mask.ndim == 3:
        mask = mask[:, None]
    m, c, t = roi.shape[:3]
    return [[[window(roi[g, k, i], mask[g, i if mask.shape[1] > 1 else 0], q) for i in range(t)] for k in range(c)]
            for g in range(m)]


def field(recs, name, dtype=np.float64):
    """One field of ``stack``'s records as an array (M, C, T, ...)."""
    return np.array([[[np.asarray(r[name], dtype=dtype) for r in row] for row in plane] for plane in recs])


def interpolate(n, order, q):
    """numpy's ``method="linear"`` between the two order statistics, operation for operation in float64."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    pos = (np.asarray(n, dtype=np.float64)[..., None] - 1.0) * q
    g = pos - np.floor(pos)
    a, b = order[..., 0], order[..., 1]
    with np.errstate(invalid="ignore"):
        d = b - a
        return np.where(g >= 0.5, b - d * (1.0 - g), a + d * g)


def sum_bound(rec):
    """|sum - ref| allowed for float pixels: (n - 1) 2^-53 sum|x| (n - 1 roundings of partial sums, none above
    sum|x|); integer sums are exact."""
    return LD(max(rec["n"] - 1, 0)) * LD(U) * rec["abs_sum"]


def m2_bound(rec):
    """|m2 - ref| allowed.  x - fl(mean) is exact or one rounding; the common error D of the mean cancels to first
    order because sum (x - mean) = 0; what remains is n D^2 plus the n + 2 roundings of squaring and summing
    non-negative terms.  Integer pixels (the mean of an exact sum: D^2 below the roundings): (n + 8) 2^-53 exact.
    Float pixels: (n + 8) 2^-53 (ref + n D^2) + n D^2 with D = (n + 2) 2^-53 sum|x| / n."""
    n = rec["n"]
    if rec["integer"]:
        return Fraction(n + 8, 2 ** 53) * rec["m2"]
    d = LD(n + 2) * LD(U) * rec["abs_sum"] / LD(max(n, 1))
    return LD(n + 8) * LD(U) * (rec["m2"] + n * d * d) + n * d * d


def disk(L, cy=None, cx=None, r=None):
    yy, xx = np.mgrid[:L, :L]
    cy, cx = (L - 1) / 2 if cy is None else cy, (L - 1) / 2 if cx is None else cx
    r = L / 3 if r is None else r
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


MASK_KINDS = ("empty", "one", "two", "full", "disk", "half")


def make_mask(kind, L, rng):
    m = np.zeros((L, L), dtype=bool)
    if kind == "one":
        m.reshape(-1)[rng.integers(L * L)] = True
    elif kind == "two":
        m.reshape(-1)[rng.choice(L * L, size=min(2, L * L), replace=False)] = True
    elif kind == "full":
        m[:] = True
    elif kind == "disk":
        m = disk(L)
    elif kind == "half":
        m = rng.random((L, L)) < 0.5
    return m


def mask_set(m, t, L, rng):
    """(m, t, L, L) bool: the six kinds of mask dealt over the (marker, timepoint) slots, every kind at least once
    when m t >= 6."""
    out = np.zeros((m, t, L, L), dtype=bool)
    for i in range(m * t):
        out[i // t, i % t] = make_mask(MASK_KINDS[i % len(MASK_KINDS)], L, rng)
    return out


def full_range(dtype, shape, rng):
    """Pixels over the whole range of the type: every integer value; every finite float32 bit pattern; float64 with
    exponents within +-100 (their squares and sums stay finite in float64, as they do in the longdouble oracle)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    if dtype == np.float32:
        bits = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
        bits = np.where((bits & 0x7F800000) == 0x7F800000, bits & np.uint32(0xBFFFFFFF), bits).astype(np.uint32)
        return bits.view(np.float32)
    return (rng.choice([-1.0, 1.0], size=shape) * (1 + rng.random(shape)) * 2.0 ** rng.integers(-100, 101, size=shape))
