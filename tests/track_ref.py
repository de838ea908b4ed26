"""NumPy restatement of ``find_beads(track="ncc")`` ("find_beads: following beads through time"),
independent of magnify_amd/track.py and of the kernel.

planes (T, h, w) of one channel, beads (M, 3) [row, col, r], half, md = max_drift, W = 2 md + 1, t_ref.
Patch of bead (row, col): the pixels (y, x) with |y - row| <= half, |x - col| <= half, md <= y < h - md,
md <= x < w - md -- a rectangle of n pixels (possibly 0).  B = plane[t_ref] on the patch; for (dy, dx) in [-md, md]^2,
A(y, x) = plane[t][y + dy, x + dx].  fixed = [n, sum B, sum B^2]; sums[t, dy + md, dx + md] = [sum A, sum A^2, sum A B]
(int64 for integer pixels, float64 else).  Score z = (n sAB - sA sB) / sqrt((n sAA - sA^2)(n sBB - sB^2)) in float64,
0 where a variance term is <= 0 or z is not finite.  Pick: largest z, ties to the smallest dy^2 + dx^2, then dy, then
dx.  Row t_ref: shift (0, 0), score 1.  Tables: (row + dy, col + dx, r), the centre clamped into the image; where
score < min_score the bead keeps its t_ref position and is not followed.
"""
import numpy as np

from synth import draw_beads, random_bead_positions


def patch(row, col, half, md, h, w):
    """((y0, y1), (x0, x1)) half-open; y1 <= y0 or x1 <= x0: empty."""
    y0, y1 = max(row - half, md), min(row + half + 1, h - md)
    x0, x1 = max(col - half, md), min(col + half + 1, w - md)
    return (y0, max(y1, y0)), (x0, max(x1, x0))


def track_sums(planes, beads, half, md, t_ref=0):
    """sums (M, T, W, W, 3), fixed (M, 3)."""
    n_t, h, w = planes.shape
    acc = np.int64 if planes.dtype.kind == "u" else np.float64
    width = 2 * md + 1
    sums = np.zeros((len(beads), n_t, width, width, 3), dtype=acc)
    fixed = np.zeros((len(beads), 3), dtype=acc)
    for g, (row, col, _) in enumerate(np.asarray(beads).reshape(-1, 3)):
        (y0, y1), (x0, x1) = patch(int(row), int(col), half, md, h, w)
        if y1 == y0 or x1 == x0:
            continue
        B = planes[t_ref, y0:y1, x0:x1].astype(acc)
        fixed[g] = [B.size, B.sum(), (B * B).sum()]
        for t in range(n_t):
            A = planes[t].astype(acc)
            for dy in range(-md, md + 1):
                for dx in range(-md, md + 1):
                    Ad = A[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
                    assert Ad.shape == B.shape
                    sums[g, t, dy + md, dx + md] = [Ad.sum(), (Ad * Ad).sum(), (Ad * B).sum()]
    return sums, fixed


def scores(sums, fixed):
    """(M, T, W, W) float64, one displacement at a time."""
    z = np.zeros(sums.shape[:-1], dtype=np.float64)
    for g in range(sums.shape[0]):
        n, sb, sbb = (np.float64(x) for x in fixed[g])
        vb = n * sbb - sb * sb
        for t in range(sums.shape[1]):
            for i in range(sums.shape[2]):
                for j in range(sums.shape[3]):
                    sa, saa, sab = (np.float64(x) for x in sums[g, t, i, j])
                    va = n * saa - sa * sa
                    with np.errstate(all="ignore"):
                        val = (n * sab - sa * sb) / np.sqrt(va * vb)
                    z[g, t, i, j] = val if (va > 0 and vb > 0 and np.isfinite(val)) else 0.0
    return z


def pick(z, t_ref=0):
    """(shift (M, T, 2), best (M, T), gap (M, T): best minus the second-best score): plain loops."""
    md = (z.shape[-1] - 1) // 2
    shift = np.zeros(z.shape[:2] + (2,), dtype=np.int64)
    best, gap = np.zeros(z.shape[:2]), np.zeros(z.shape[:2])
    for g in range(z.shape[0]):
        for t in range(z.shape[1]):
            keys = sorted((-z[g, t, dy + md, dx + md], dy * dy + dx * dx, dy, dx)
                          for dy in range(-md, md + 1) for dx in range(-md, md + 1))
            shift[g, t], best[g, t] = (keys[0][2], keys[0][3]), -keys[0][0]
            gap[g, t] = keys[1][0] - keys[0][0]
    shift[:, t_ref], best[:, t_ref], gap[:, t_ref] = 0, 1.0, np.inf
    return shift, best, gap


def track(planes, beads, half, md, t_ref=0):
    """{"sums", "fixed", "z", "shift", "score", "gap"} of the restatement."""
    sums, fixed = track_sums(planes, beads, half, md, t_ref)
    z = scores(sums, fixed)
    shift, best, gap = pick(z, t_ref)
    return {"sums": sums, "fixed": fixed, "z": z, "shift": shift, "score": best, "gap": gap}


def tables(beads, shift, score, min_score, h, w):
    """(tables (T, M, 3), followed (M, T))."""
    beads = np.asarray(beads).reshape(-1, 3)
    m, n_t = score.shape
    out = np.zeros((n_t, m, 3), dtype=np.int64)
    followed = np.zeros((m, n_t), dtype=bool)
    for g in range(m):
        for t in range(n_t):
            followed[g, t] = bool(score[g, t] >= min_score)
            dy, dx = (int(shift[g, t, 0]), int(shift[g, t, 1])) if followed[g, t] else (0, 0)
            out[t, g] = (min(max(int(beads[g, 0]) + dy, 0), h - 1), min(max(int(beads[g, 1]) + dx, 0), w - 1), beads[g, 2])
    return out, followed


def scene(seed, shape, n, r_lo, r_hi, m, T, channels=None, background=100, poisson=20.0, read_noise=3.0):
    """(planes (T, h, w) uint16, beads (n', 3) [row, col, r] at time 0, offsets (n', T, 2)): beads from
    ``random_bead_positions(rng, shape, n, r_hi + m + 2)``, per timepoint an integer offset in [-m, m]^2 per bead (time 0
    unmoved), fresh Poisson and read noise per timepoint as ``synth.noisy_bead_image``.  ``channels``: planes
    (channels, T, h, w) -- every channel with bead values and noise of its own, the beads moving together."""
    rng = np.random.default_rng(seed)
    pos = random_bead_positions(rng, shape, n, r_hi + m + 2)
    radii = rng.integers(r_lo, r_hi + 1, size=len(pos))
    offsets = rng.integers(-m, m + 1, size=(len(pos), T, 2))
    offsets[:, 0] = 0
    planes = np.empty((channels or 1, T) + tuple(shape), dtype=np.uint16)
    for c in range(channels or 1):
        values = rng.integers(500, 4001, size=len(pos))
        for t in range(T):
            img = background + rng.poisson(poisson, size=shape).astype(np.float64)
            disks = draw_beads(shape, pos + offsets[:, t], 2 * radii, values).astype(np.float64)
            img = np.where(disks > 0, disks + img, img)
            img = np.rint(img + rng.normal(0, read_noise, size=shape))
            planes[c, t] = np.clip(img, 0, 65535).astype(np.uint16)
    return (planes if channels else planes[0]), np.column_stack([pos, radii]), offsets


def _stripes(period, shift):
    _, x = np.mgrid[0:40, 0:44]
    return (100 + 50 * ((x + shift) % period)).astype(np.uint16)


def _checker(shift):
    y, x = np.mgrid[0:40, 0:44]
    return (100 + 50 * ((x + y + shift) % 2)).astype(np.uint16)


# name -> (planes (2, 40, 44): time 0 and time 1, the pick at time 1 among exactly tied displacements); m = 2, one bead
# at TIE_BEAD with half = 6
TIE_BEAD, TIE_HALF, TIE_M = np.array([[20, 22, 5]]), 6, 2
TIES = {
    "stripes, unmoved": (np.stack([_stripes(2, 0), _stripes(2, 0)]), (0, 0)),        # every even dx, every dy
    "stripes, one column": (np.stack([_stripes(2, 0), _stripes(2, 1)]), (0, -1)),    # dx -1 or 1: the smaller dx
    "stripes of 4, two columns": (np.stack([_stripes(4, 0), _stripes(4, 2)]), (0, -2)),
    "checkerboard, one step": (np.stack([_checker(0), _checker(1)]), (-1, 0)),       # dy + dx odd: the smallest dy
}
