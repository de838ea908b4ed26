"""Oracles of the chip path's oldest device code -- the offset costs of ``cluster_1d`` (mg_cluster1d_costs) and the
fg / bg masks of the chambers (mg_button_masks) -- the error bound the costs are held to, and the inputs that the CPU
and the GPU tests of them share.

The boundaries and centres of the clusters are float64 values, formed as the reference forms them; everything after
them is exact: squared distances as integers over one power-of-two denominator, means, penalty terms and totals as
``Fraction``, ``sqrt(ideal)`` to 40 significant digits."""
import decimal
import functools
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit roundoff of float64
SQRT_DIGITS = 40

# ---- cluster costs -------------------------------------------------------------------------------------------------------


def boundaries(n_clusters, cluster_length, offset):
    """Float64 boundaries and centres of the clusters at one offset, as find.py:647-649 forms them."""
    b = np.arange(n_clusters + 1) * cluster_length + offset
    return b, (b[1:] + b[:-1]) / 2


def _exact_sqrt(value):
    with decimal.localcontext() as ctx:
        ctx.prec = SQRT_DIGITS
        return Fraction(decimal.Decimal(float(value)).sqrt())


def _scaled(values, shift):
    """The float64 ``values`` times 2**shift as Python ints (exact: shift covers every value's last bit)."""
    out = []
    for v in values:
        num, den = float(v).as_integer_ratio()
        out.append(num << (shift - (den.bit_length() - 1)))
    return out


def _last_bit(values):
    return max([float(v).as_integer_ratio()[1].bit_length() - 1 for v in values], default=0)


def cluster_costs_exact(points, n_offsets, n_clusters, cluster_length, ideal, penalty):
    """cost(offset) = sum_k [ var_k * sqrt(ideal_k) + penalty * (ideal_k - n_k)**2 ] of find.py:632-677 for the offsets
    0 .. n_offsets - 1, without rounding: var_k is the mean squared distance of the cluster's points to its (float64)
    centre, membership is ``searchsorted(side="left")`` of the (float64) boundaries in the sorted points, empty clusters
    take the largest var of their offset (0 if all are empty).  Returns (float64 nearest values, list of Fraction).

    The sum of a cluster's squared distances comes from exact integer prefix sums of p and p*p:
    sum (p - c)**2 = sum p*p - 2 c sum p + n c*c, all over the denominator 4**shift."""
    pts = np.sort(np.asarray(points, dtype=np.float64).reshape(-1))
    ideal = [Fraction(float(v)) for v in np.asarray(ideal).reshape(-1)]
    assert len(ideal) == n_clusters
    root = [_exact_sqrt(v) for v in ideal]
    penalty = Fraction(float(penalty))
    grids = [boundaries(n_clusters, cluster_length, off) for off in range(n_offsets)]
    shift = max([_last_bit(pts)] + [_last_bit(c) for _, c in grids])
    p1, p2 = [0], [0]
    for p in _scaled(pts, shift):
        p1.append(p1[-1] + p)
        p2.append(p2[-1] + p * p)
    exact = []
    for bounds, centres in grids:
        spans = np.searchsorted(pts, bounds, side="left").tolist()
        var = [None] * n_clusters
        for k, c in enumerate(_scaled(centres, shift)):
            lo, hi = spans[k], spans[k + 1]
            if hi > lo:
                squares = (p2[hi] - p2[lo]) - 2 * c * (p1[hi] - p1[lo]) + (hi - lo) * c * c
                var[k] = Fraction(squares, (hi - lo) << (2 * shift))
        vmax = max([v for v in var if v is not None], default=Fraction(0))
        total = Fraction(0)
        for k in range(n_clusters):
            n_k = spans[k + 1] - spans[k]
            total += (vmax if var[k] is None else var[k]) * root[k] + penalty * (ideal[k] - n_k) ** 2
        exact.append(total)
    return np.array([float(c) for c in exact], dtype=np.float64), exact


def largest_cluster(points, n_offsets, n_clusters, cluster_length):
    """The largest number of points that one cluster holds at any of the offsets."""
    pts = np.sort(np.asarray(points, dtype=np.float64).reshape(-1))
    most = 0
    for off in range(n_offsets):
        spans = np.searchsorted(pts, boundaries(n_clusters, cluster_length, off)[0], side="left")
        most = max(most, int(np.diff(spans).max()))
    return most


def cost_bound(points, n_offsets, n_clusters, cluster_length):
    """Relative error bound (n_max + K + 8) * 2**-53 of a cost, for any float64 evaluation that forms the terms of the
    sum from the float64 centres and adds them up, each term on its own; n_max = ``largest_cluster``, K = n_clusters.

    Derivation (u = 2**-53, every operation correctly rounded, result (1 + d) exact with abs(d) <= u).  For
    penalty >= 0 every quantity below is >= 0, so relative errors never grow by cancellation: a sum of non-negative terms
    with relative errors <= e has a relative error <= e, and each rounding multiplies by one more (1 + d).
      p - c                         1 rounding
      (p - c) * (p - c)             3 factors (the difference twice, the product once)
      sum of n such squares         at most n - 1 more on any one of them, in any order of adding
      / n                           1:  var carries at most n + 3 factors (an empty cluster takes the var of another)
      sqrt(ideal)                   1
      var * sqrt(ideal)             1:  n + 5
      penalty * miss * miss         2 (miss = ideal - n is exact for counts): fewer than the above
      term = the two added          1:  n + 6
      total of K terms from 0       K - 1 (0 + x is exact): n + K + 5 factors at most.
    (1 + u)**m - 1 <= m u / (1 - m u), which stays below (m + 3) u as long as m * m * u < 3 -- m below 1e8 here.  So
    abs(computed - exact) <= (n_max + K + 8) u exact.  A difference of one running sum over all points is NOT such an
    evaluation (it cancels), so the reference's own cumsum form is only as good as this bound where no cluster is much
    smaller than what was added before it."""
    return (largest_cluster(points, n_offsets, n_clusters, cluster_length) + n_clusters + 8) * U


def error_ratio(have, exact, bound):
    """max over the offsets of abs(have - exact) / (bound * exact), exactly; 0 where both are 0, inf where only the exact
    cost is 0."""
    worst = 0.0
    for h, e in zip(np.asarray(have, dtype=np.float64).tolist(), exact):
        if not np.isfinite(h):
            return float("inf")
        err = abs(Fraction(h) - e)
        if err:
            worst = max(worst, float(err / (Fraction(bound) * e))) if e else float("inf")
    return worst


def separation(exact, bound):
    """True when the smallest exact cost is more than 4 * bound * cost away from the second smallest (a single offset
    is separated): two evaluations within ``bound`` of the exact costs then agree on the first minimum."""
    if len(exact) < 2:
        return True
    first, second = sorted(exact)[:2]
    return second - first > 4 * Fraction(bound) * second


def labels_of(points, n_clusters, cluster_length, offset):
    """Cluster of every point at one offset (-1 outside), in the order the points came in."""
    points = np.asarray(points, dtype=np.float64).reshape(-1)
    bounds = boundaries(n_clusters, cluster_length, offset)[0]
    k = np.searchsorted(bounds, points, side="right") - 1  # bounds[k] <= p < bounds[k + 1]
    return np.where((k >= 0) & (k < n_clusters), k, -1)


# ---- the sweep's inputs ----------------------------------------------------------------------------------------------------

CLUSTERS = (1, 2, 63, 64, 65, 130)
LENGTHS = (7.0, 9.0, 10.5, 33.3)
OFFSETS = (1, 2, 37)
PENALTIES = (0, 50)
LONG = 3000  # points of the one crowded cluster
# sets marked separated whose first draw was not (``separation``): they take the next seed, and the CPU test holds
# every set that is left to the condition
RESEED = {("integers", 1, 7.0, 2, 50): 1, ("integers", 1, 9.0, 37, 0): 1, ("integers", 1, 10.5, 37, 0): 1,
          ("integers", 1, 33.3, 2, 0): 1, ("integers", 2, 33.3, 2, 0): 1}


def _rng(kind, n_clusters, cluster_length, n_offsets, penalty):
    key = (kind, n_clusters, cluster_length, n_offsets, penalty)
    return np.random.default_rng([{"uniform": 1, "integers": 2, "one": 3, "ideal0": 4, "long": 5, "other": 6}[kind],
                                  n_clusters, int(cluster_length * 10), n_offsets, penalty, RESEED.get(key, 0)])


@functools.lru_cache(maxsize=None)
def point_sets(n_clusters, cluster_length, n_offsets, penalty):
    """The point sets of one (clusters, length, offsets, penalty): a tuple of dicts {name, points (unsorted, read-only),
    ideal (int64, drawn from 0 .. 5), separated, exact (Fractions), bound}."""
    K, L = n_clusters, cluster_length
    span = K * L + n_offsets  # the clusters of all offsets lie in [0, span)
    sets = []

    def add(name, points, ideal, separated=False):
        points = np.asarray(points, dtype=np.float64)
        points.setflags(write=False)
        _, exact = cluster_costs_exact(points, n_offsets, K, L, ideal, penalty)
        sets.append(dict(name=name, points=points, ideal=np.asarray(ideal, dtype=np.int64), separated=separated,
                         exact=exact, bound=cost_bound(points, n_offsets, K, L)))

    dense = 3 * K + 2 + 2 * n_offsets  # few offsets without any point: with penalty 0 those all cost 0, a tie
    rng = _rng("uniform", K, L, n_offsets, penalty)
    add("uniform", rng.uniform(0, span, dense), rng.integers(0, 6, K), separated=True)
    rng = _rng("integers", K, L, n_offsets, penalty)
    add("integers", rng.integers(0, int(np.ceil(span)), dense), rng.integers(0, 6, K), separated=True)
    rng = _rng("other", K, L, n_offsets, penalty)
    first, last = boundaries(K, L, 0)[0], boundaries(K, L, n_offsets - 1)[0]
    add("boundaries", rng.permutation(np.concatenate([first, last, first[:: max(1, K // 7)]])), rng.integers(0, 6, K))
    add("left", [-span, -3.5, -1.0, -2.0 ** -40], rng.integers(0, 6, K))
    add("right", [last[-1], np.nextafter(last[-1], np.inf), span + 5, 1e6, last[-1]], rng.integers(0, 6, K))
    add("none", [], rng.integers(0, 6, K))
    rng = _rng("one", K, L, n_offsets, penalty)
    add("one", rng.uniform(0, span, 1), rng.integers(0, 6, K))
    rng = _rng("ideal0", K, L, n_offsets, penalty)
    k0 = K // 2
    ideal = rng.integers(0, 6, K)
    ideal[k0] = 0
    add("ideal0", np.concatenate([rng.uniform(0, span, 2 * K), rng.uniform(k0 * L, (k0 + 1) * L, 4)]), ideal)
    rng = _rng("long", K, L, n_offsets, penalty)
    add("long", rng.permutation(np.concatenate([rng.uniform(0, span, K), rng.uniform(k0 * L, (k0 + 1) * L, LONG)])),
        rng.integers(0, 6, K))
    return tuple(sets)


# hand-made ties: (points, total_length, clusters, length, ideal, penalty, the offsets that tie at the minimum).  Small
# integers and halves: every float64 operation of any evaluation is exact up to the two products with sqrt(2), which are
# the same two numbers at both offsets, added in either order.
TIES = (
    ([10, 10, 30, 30], 60, 3, 9.0, [2, 0, 2], 50, (6, 7)),
    ([30, 10, 30, 10], 60, 3, 11.0, [2, 0, 2], 50, (3, 4)),
    ([10, 10, 30, 30], 60, 3, 9.0, [2, 0, 2], 7.5, (6, 7)),  # (with a penalty near 0 the offsets that hold no point win)
    ([12.5, 12.5], 40, 1, 8.0, [2], 50, (8, 9)),  # one cluster, centre off + 4: 0.5 to either side
)


def tie_offsets(total_length, n_clusters, cluster_length):
    return int(total_length - round(n_clusters * cluster_length))


# ---- button masks -----------------------------------------------------------------------------------------------------------


def disk_halfwidths(radius):
    """half[ady] = the largest adx of cv.circle's filled disk in the rows cy +- ady (oracle.ref_opencv.filled_circle_mask's
    walk of cv::Circle, restated)."""
    half = np.full(radius + 1, -1, dtype=np.int64)
    err, dx, dy = 0, radius, 0
    plus, minus = 1, 2 * radius - 1
    while dx >= dy:
        half[dy] = max(half[dy], dx)
        half[dx] = max(half[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return half


def button_masks_ref(centers, radii, L, outer_r, inner_r):
    """fg (m, L, L) uint8 = cv.circle's filled disk of radius_i about centre_i = (row, col) in window coordinates,
    bg = disk(outer_r) and not disk(inner_r) about the same centre -- all markers at once: the half width of every
    window row of every marker, then one comparison per pixel."""
    centers = np.asarray(centers, dtype=np.int64).reshape(-1, 2)
    radii = np.asarray(radii, dtype=np.int64).reshape(-1)
    m = len(radii)
    top = int(max([outer_r, inner_r, 0] + radii.tolist()))
    table = np.full((top + 1, top + 1), -1, dtype=np.int64)
    for r in set([int(outer_r), int(inner_r)] + radii.tolist()):
        table[r, : r + 1] = disk_halfwidths(r)
    ady = np.abs(np.arange(L, dtype=np.int64)[None, :] - centers[:, 0:1])  # (m, L)
    adx = np.abs(np.arange(L, dtype=np.int64)[None, :] - centers[:, 1:2])

    def disk(r):
        r = np.broadcast_to(np.asarray(r, dtype=np.int64), (m,))[:, None]
        rows = np.where(ady <= r, table[r, np.minimum(ady, top)], -1)  # (m, L): half width of each window row
        return adx[:, None, :] <= rows[:, :, None]

    fg = disk(radii)
    bg = disk(outer_r) & ~disk(inner_r)
    return fg.astype(np.uint8), bg.astype(np.uint8)


MASK_LENGTHS = (1, 2, 17, 72, 73)
MASK_PAIRS = ((15, 30), (0, 30), (30, 30), (31, 30))  # (inner, outer); the last two annuli are empty
MASK_M = 300


def mask_markers(L, outer_r):
    """Every centre of {inside, the corners and edges, -1 and L, just out of the outer disk's reach, +-2**20} on each
    axis with every radius of {0, 1, 2, 15, outer, outer + 5, 100}, in a seeded order: (567, 2) centres (row, col) and
    (567,) radii."""
    axis = [L // 2, 0, L - 1, -1, L, -outer_r - 1, L + outer_r, -2 ** 20, 2 ** 20]
    radii = [0, 1, 2, 15, outer_r, outer_r + 5, 100]
    grid = np.array([(cy, cx, r) for cy in axis for cx in axis for r in radii], dtype=np.int64)
    grid = grid[np.random.default_rng([L, outer_r]).permutation(len(grid))]
    return grid[:, :2].copy(), grid[:, 2].copy()


def mask_batches(L, outer_r):
    """The markers of ``mask_markers`` as two calls of MASK_M markers that cover all of them (they overlap)."""
    centers, radii = mask_markers(L, outer_r)
    return [(centers[:MASK_M], radii[:MASK_M]), (centers[-MASK_M:], radii[-MASK_M:])]
