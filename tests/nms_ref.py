"""Greedy suppression in plain NumPy, and the seeded planes the suppression tests run on (CPU and GPU tests alike).

The oracle is ``oracle.ref_numeric.filter_neighbors`` (utils.py:254-292, pinned by the ``filter_neighbors`` golden) applied
in the suppression order: score descending, then tie key ascending as UNSIGNED 32-bit (the circle's list index when there
are no keys).  Everything here is integer-exact.

A *plane* (``Plane``) is a list of circles with scores and unique tie keys plus the ``d_max_rc`` handed to the kernels.
``lay_out`` spreads it over a larger circle list the way the kernels see it: ``d_alive`` is a random permutation of a
random subset of ``[0, circle_cap)``, and whatever is not alive holds sentinels that no kernel may read or write.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import ref_numeric as rn

H, W = 700, 900          # the image of the claim-grid planes
BUCKET_R, BUCKET_C = 32, 64  # mg_nms_sparse buckets: borders at rows / columns that are multiples of these (bias 64 keeps them)
SPARSE_CAP, SPARSE_MAXB = 12288, 9216  # the kernel's stated limits: alive circles, buckets per plane
STATE_SENTINEL, KEY_SENTINEL, COORD_SENTINEL, SCORE_SENTINEL = 0xA5, 0xDEADBEEF, -30000, -7.0
CHAIN_LEN, CHAIN2_LEN = 400, 200


class Plane(NamedTuple):
    circles: np.ndarray  # (n, 3) int32 (row, col, r)
    scores: np.ndarray   # (n,) float32
    keys: np.ndarray     # (n,) uint32, unique
    max_rc: np.ndarray   # (2,) int32: d_max_rc of the plane


class Layout(NamedTuple):
    circles: np.ndarray  # (cap, 3) int32
    scores: np.ndarray   # (cap,) float32
    keys: np.ndarray     # (cap,) uint32
    alive: np.ndarray    # (n,) int32: d_alive
    max_rc: np.ndarray


# ---- the rule ------------------------------------------------------------------------------------------------------
def priority_order(scores, tie):
    """Suppression order of circles with these scores and tie keys (None: their index)."""
    scores = np.asarray(scores)
    tie = np.arange(len(scores)) if tie is None else np.asarray(tie)
    return np.lexsort((tie.astype(np.uint64), -scores.astype(np.float64)))


def expected(circles, scores, tie, alive, min_dist):
    """(state bytes indexed as d_state is: 1 kept, 2 dropped, 0 not alive; kept rows in order; their scores) of the alive
    circles of one plane's circle list.  ``tie`` None: the circle's index in the list."""
    alive = np.asarray(alive, dtype=np.int64)
    t = alive if tie is None else np.asarray(tie)[alive]
    s = alive[priority_order(np.asarray(scores)[alive], t)]
    keep = rn.filter_neighbors(circles[s], min_dist) if min_dist > 0 else np.ones(len(s), dtype=bool)
    state = np.zeros(len(circles), dtype=np.uint8)
    state[s] = np.where(keep, 1, 2)
    return state, circles[s][keep], np.asarray(scores)[s][keep]


def difference_table(d):
    """(4 d + 1, 4 d + 1) bool: [dr + 2 d, dc + 2 d] is bit (dr + 2 d)(4 d + 1) + dc + 2 d of hotpath._ring_difference_bits."""
    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    side = 4 * d + 1
    words = hotpath._ring_difference_bits(nat.circle_points(d, True), d).view(np.uint32)
    assert len(words) == (side * side + 31) // 32
    bit = np.arange(side * side)
    return ((words[bit >> 5] >> (bit & 31).astype(np.uint32)) & 1).astype(bool).reshape(side, side)


def greedy_by_differences(circles_in_order, min_dist):
    """mg_nms_sparse's rule: keep i iff no earlier kept j has c_i - c_j in D.  Returns the keep mask."""
    c = np.asarray(circles_in_order, dtype=np.int64)[:, :2]
    table, reach = difference_table(min_dist).tolist(), 2 * min_dist
    keep = np.zeros(len(c), dtype=bool)
    cells = {}  # kept centres by cell of side 2 d + 1: whatever is within reach lies in the 3 x 3 cells around
    for i, (r, col) in enumerate(c.tolist()):
        br, bc = r // (reach + 1), col // (reach + 1)
        hit = False
        for nr_ in (br - 1, br, br + 1):
            for nc_ in (bc - 1, bc, bc + 1):
                for kr, kc in cells.get((nr_, nc_), ()):
                    dr, dc = r - kr, col - kc
                    if abs(dr) <= reach and abs(dc) <= reach and table[dr + reach][dc + reach]:
                        hit = True
        if not hit:
            keep[i] = True
            cells.setdefault((br, bc), []).append((r, col))
    return keep


# ---- planes --------------------------------------------------------------------------------------------------------
def _scores(rng, n):
    return np.round(rng.uniform(0.3, 1.0, n), 2).astype(np.float32)  # two decimals: many equal scores


def _keys(rng, n):
    """n unique 32-bit keys, about 60 % of them with bit 31 set."""
    low = rng.choice(1 << 31, size=n, replace=False).astype(np.uint32)
    return low | (rng.random(n) < 0.6).astype(np.uint32) << np.uint32(31)


def _plane(c, scores, keys, max_rc=None):
    c = np.asarray(c, dtype=np.int32).reshape(-1, 3)
    if max_rc is None:
        max_rc = [c[:, 0].max(), c[:, 1].max()] if len(c) else [0, 0]
    return Plane(c, np.asarray(scores, dtype=np.float32), np.asarray(keys, dtype=np.uint32), np.asarray(max_rc, dtype=np.int32))


def crowded(seed, n, d, max_row=H - 1, max_col=W - 1, cluster=8):
    """n circles in clusters of about ``cluster`` within reach (2 d) of each other, centres in [-(d + 1), max]: many conflicts,
    many equal scores, offsets inside the reach square but outside D, twenty circles on one centre."""
    rng = np.random.default_rng([seed, n, d])
    k = max(1, n // cluster)
    cl = np.column_stack([rng.integers(-(d + 1), max_row + 1, k), rng.integers(-(d + 1), max_col + 1, k)])
    c = cl[rng.integers(0, k, n)] + rng.integers(-2 * d, 2 * d + 1, size=(n, 2))
    c = np.column_stack([np.clip(c[:, 0], -(d + 1), max_row), np.clip(c[:, 1], -(d + 1), max_col), rng.integers(5, 20, n)])
    c[20:40, :2] = c[20, :2]
    return _plane(c, _scores(rng, n), _keys(rng, n))


def with_circles(plane, seed, rows, max_rc=None):
    """``plane`` with its first circles moved to ``rows`` ((row, col) each); d_max_rc the true maxima unless given."""
    c = plane.circles.copy()
    rows = np.asarray(rows).reshape(-1, 2)
    c[: len(rows), :2] = rows
    return _plane(c, plane.scores, plane.keys, max_rc)


def wrap_plane(seed, n, d):
    """Centres at -(d + 2) and below (the reference's claim index goes negative and wraps) and one at H + 20; d_max_rc is
    the true maxima, so the oracle's modulus is the kernel's."""
    base = crowded(seed, n, d)
    return with_circles(base, seed, [[-(d + 2), 40], [55, -(d + 2)], [-(2 * d + 5), 300], [H + 20, 33], [-(d + 3), -(d + 4)],
                                     [-(d + 2), 44], [H + 20, 33 + d]])


def empty_plane():
    return _plane(np.zeros((0, 3)), np.zeros(0), np.zeros(0))


def chain_path(length, d, row0, width):
    """Centres ``d`` apart along one row while it fits in ``width`` columns, else folded: rows 3 d apart (out of each
    other's reach) joined by vertical links of the same spacing, so the path stays one chain."""
    per_row = max(2, (width - 20) // d)
    pts, r, c, step = [], row0, 10, 1
    while len(pts) < length:
        for _ in range(per_row):
            pts.append((r, c))
            c += step * d
        c -= step * d
        pts += [(r + d, c), (r + 2 * d, c)]
        r, step = r + 3 * d, -step
    return np.asarray(pts[:length], dtype=np.int64)


def chain_plane(seed, d, width=W):
    """Two chains whose decisions pass from circle to circle: 400 circles ``d`` apart with scores strictly decreasing along
    the path (every third one is kept, each only after the two before it are rejected), and 200 with one score, ordered
    by tie key against the path's direction."""
    rng = np.random.default_rng([seed, d, 77])
    p1 = chain_path(CHAIN_LEN, d, 10, width)
    p2 = chain_path(CHAIN2_LEN, d, int(p1[:, 0].max()) + 4 * d, width)
    n = len(p1) + len(p2)
    c = np.column_stack([np.concatenate([p1, p2]), rng.integers(5, 20, n)])
    scores = np.concatenate([np.float32(0.99) - np.arange(len(p1), dtype=np.float32) * np.float32(0.001),
                             np.full(len(p2), 0.5, dtype=np.float32)])
    assert (np.diff(scores[: len(p1)]) < 0).all()
    keys = _keys(rng, n)
    keys[len(p1):] = np.sort(keys[len(p1):])[::-1]
    return _plane(c, scores, keys)


BORDER_SITES = (4, 8)  # sites 128 apart: 128 is a multiple of both bucket edges


def border_plane(seed, d):
    """Pairs at centre differences (+-2d, 0), (0, +-2d), (+-d, +-d) -- rings that just meet -- and (+-(2d + 1), 0),
    (0, +-(2d + 1)) -- rings that just miss --, each pair astride a row-bucket border, a column-bucket border and a bucket
    corner.  Pairs are 128 apart: no pair is within reach of another."""
    rng = np.random.default_rng([seed, d, 31])
    deltas = [(2 * d, 0), (-2 * d, 0), (0, 2 * d), (0, -2 * d), (d, d), (d, -d), (-d, d), (-d, -d),
              (2 * d + 1, 0), (-2 * d - 1, 0), (0, 2 * d + 1), (0, -2 * d - 1)]
    rows, site = [], 0
    for kind in ("row", "col", "corner"):
        for dr, dc in deltas:
            if (kind == "row" and dr == 0) or (kind == "col" and dc == 0):
                continue  # (such a pair cannot straddle that border)
            r_b, c_b = 128 * (1 + site // BORDER_SITES[1]), 128 * (1 + site % BORDER_SITES[1])
            site += 1
            # the first circle on the near side of the border (row r_b, column c_b), the second across it
            if kind == "row":
                ar, ac = (r_b - 1 if dr > 0 else r_b), c_b + 32
            elif kind == "col":
                ar, ac = r_b + 16, (c_b - 1 if dc > 0 else c_b)
            else:
                ar, ac = (r_b - 1 if dr >= 0 else r_b), (c_b - 1 if dc >= 0 else c_b)
            rows += [(ar, ac), (ar + dr, ac + dc)]
    assert site <= BORDER_SITES[0] * BORDER_SITES[1]
    n = len(rows)
    c = np.column_stack([np.asarray(rows), rng.integers(5, 20, n)])
    return _plane(c, _scores(rng, n), _keys(rng, n), [128 * (BORDER_SITES[0] + 1) - 1, 128 * (BORDER_SITES[1] + 1) - 1])


def lay_out(plane, cap, seed):
    """The plane as the kernels see it: its circles at a random subset of the ``cap`` list slots, d_alive a random
    permutation of those, sentinels everywhere else."""
    n = len(plane.circles)
    assert cap > n  # circle_cap is larger than the alive count
    rng = np.random.default_rng([seed, cap, n])
    slots = rng.choice(cap, size=n, replace=False)
    circles = np.full((cap, 3), COORD_SENTINEL, dtype=np.int32)
    scores = np.full((cap,), SCORE_SENTINEL, dtype=np.float32)
    keys = np.full((cap,), KEY_SENTINEL, dtype=np.uint32)
    circles[slots], scores[slots], keys[slots] = plane.circles, plane.scores, plane.keys
    return Layout(circles, scores, keys, rng.permutation(slots).astype(np.int32), plane.max_rc)


def expected_of(layout, use_keys, min_dist):
    return expected(layout.circles, layout.scores, layout.keys if use_keys else None, layout.alive, min_dist)


# ---- the planes of the tests -----------------------------------------------------------------------------------------
SPARSE_DISTS = (1, 2, 8, 15)
GRID_DISTS = (2, 8, 15)
STAGE_DISTS = (1, 8, 15)
SPARSE_LIST_CAP = 12500


@functools.lru_cache(maxsize=None)
def sparse_planes(d):
    """The planes of one mg_nms_sparse launch: name -> (Plane, d_done the kernel must report)."""
    full = crowded(1, SPARSE_CAP, d)
    over = crowded(2, SPARSE_CAP + 1, d)
    # 96 x 96 buckets exactly (per = 9): circles in all four corners of the extent, a few near each so that they conflict
    lo = -(d + 1)
    corners = [[lo, lo], [lo, 6079], [3007, lo], [3007, 6079], [lo + d, lo], [lo, 6079 - d], [3007 - d, lo + 1], [3007, 6079 - 2 * d]]
    big = with_circles(crowded(3, SPARSE_CAP, d, 3007, 6079), 3, corners, [3007, 6079])
    big_over = big._replace(max_rc=np.array([3007, 6080], dtype=np.int32))
    # 37 x 34 (even) and 37 x 35 (odd: the last 16-bit start shares its word with bstart[nb]) buckets, per = 2
    even = with_circles(crowded(4, 3000, d, 1100, 2100), 4, [[1100, 2100], [1100 - d, 2100]], [1100, 2100])
    odd = with_circles(crowded(5, 3000, d, 1100, 2170), 5, [[1100, 2170], [1100, 2170 - d]], [1100, 2170])
    # a centre at exactly -(d + 1) in a row and in a column: the last the kernel takes; one at -(d + 2): refused
    at_edge = with_circles(crowded(6, 600, d, 200, 300), 6, [[lo, 50], [60, lo], [lo, 50 + d], [60 + d, lo], [lo, lo]])
    past_edge = with_circles(at_edge, 6, [[lo - 1, 50]])
    # d_max_rc one less than a circle's row
    under = crowded(7, 600, d, 200, 300)
    under = under._replace(max_rc=under.max_rc - np.array([1, 0], dtype=np.int32))
    planes = {"full": (full, 1), "over": (over, 0), "big": (big, 1), "big_over": (big_over, 0), "per2_even": (even, 1),
              "per2_odd": (odd, 1), "at_edge": (at_edge, 1), "past_edge": (past_edge, 0), "understated": (under, 0),
              "empty": (empty_plane(), 1), "border": (border_plane(8, d), 1), "chain": (chain_plane(9, d, 6100), 1)}
    return planes


def sparse_buckets(plane):
    """(bucket rows, bucket columns) mg_nms_sparse derives from the plane's d_max_rc."""
    return ((int(plane.max_rc[0]) + 64) >> 5) + 1, ((int(plane.max_rc[1]) + 64) >> 6) + 1


GRID_N = 3000  # alive circles of the crowded claim-grid plane: below the smallest circle_cap of the lane mappings (3 200)


@functools.lru_cache(maxsize=None)
def grid_planes(d, seed):
    """The four 700 x 900 planes of the claim-grid tests: crowded (3 000 circles: clusters of twelve, for enough equal-score
    conflicts), wrap, empty, chain."""
    return (crowded(10 + seed, GRID_N, d, cluster=12), wrap_plane(20 + seed, 1500, d), empty_plane(), chain_plane(30 + seed, d))


@functools.lru_cache(maxsize=None)
def grid_case(d, seed, cap, use_keys):
    """Layouts of grid_planes(d, seed) in lists of ``cap`` and their expected (state, rows, scores)."""
    layouts = tuple(lay_out(p, cap, 100 * seed + k) for k, p in enumerate(grid_planes(d, seed)))
    return layouts, tuple(expected_of(lo, use_keys, d) for lo in layouts)


@functools.lru_cache(maxsize=None)
def sparse_case(d, use_keys):
    layouts = {name: lay_out(p, SPARSE_LIST_CAP, k) for k, (name, (p, _)) in enumerate(sparse_planes(d).items())}
    want = {name: expected_of(layouts[name], use_keys, d) for name, (_, done) in sparse_planes(d).items() if done}
    return layouts, want


def wraps(plane, d):
    """Whether a ring of the plane reaches a negative claim index (the sparse kernel's refusal, the oracle's wrap)."""
    return len(plane.circles) > 0 and bool((plane.circles[:, :2] < -(d + 1)).any())


def conditions(plane, d):
    """What makes a plane a test of the suppression: kept share, conflicting pairs with equal float32 scores, pairs
    inside the reach square that are not in D, the largest group on one centre."""
    from scipy.spatial import cKDTree

    c = plane.circles[:, :2].astype(np.int64)
    order = priority_order(plane.scores, plane.keys)
    keep = rn.filter_neighbors(plane.circles[order], d)
    pairs = cKDTree(c).query_pairs(2 * d, p=np.inf, output_type="ndarray")
    diff = c[pairs[:, 0]] - c[pairs[:, 1]]
    in_d = difference_table(d)[diff[:, 0] + 2 * d, diff[:, 1] + 2 * d]
    equal = plane.scores[pairs[:, 0]] == plane.scores[pairs[:, 1]]
    _, counts = np.unique(c, axis=0, return_counts=True)
    return {"kept": int(keep.sum()), "share": float(keep.mean()), "equal_conflicts": int((in_d & equal).sum()),
            "not_in_d": int((~in_d).sum()), "same_centre": int(counts.max())}
