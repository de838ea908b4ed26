"""What of the chip path's cluster costs and chamber masks can be held to account without a GPU: the exact oracle of
tests/buttons_ref.py against the reference's own float64 formula (``oracle.ref_pipeline.cluster_1d``) and its labels,
the condition under which the GPU tests may demand equal labels, the hand-made ties, and the vectorised mask oracle
against ``oracle.ref_opencv.filled_circle_mask`` marker by marker -- on the inputs that the GPU tests use."""
from fractions import Fraction

import numpy as np
import pytest

import buttons_ref as ref
from oracle import ref_opencv as rcv
from oracle import ref_pipeline as rp


def reference_costs(points, n_offsets, n_clusters, cluster_length, ideal, penalty):
    """The total of every offset as ``rp.cluster_1d`` computes it (its loop body, find.py:647-668)."""
    pts = np.sort(np.asarray(points, dtype=np.float64))
    ideal = np.asarray(ideal)
    totals = []
    for offset in range(n_offsets):
        bounds = np.arange(n_clusters + 1) * cluster_length + offset
        centers = (bounds[1:] + bounds[:-1]) / 2
        spans = np.searchsorted(pts, bounds)
        n_in = spans[1:] - spans[:-1]
        sq = (pts[spans[0]: spans[-1]] - np.repeat(centers, n_in)) ** 2
        run = np.insert(np.cumsum(sq), 0, 0)
        cost = np.diff(run[spans - spans[0]])
        has = n_in > 0
        cost[has] /= n_in[has]
        cost[~has] = np.max(cost)
        cost *= np.sqrt(ideal)
        cost = cost + penalty * (ideal - n_in) ** 2
        totals.append(cost.sum())
    return np.array(totals, dtype=np.float64)


def first_minimum(exact):
    return min(range(len(exact)), key=lambda i: (exact[i], i))


@pytest.mark.parametrize("n_clusters", ref.CLUSTERS)
@pytest.mark.parametrize("cluster_length", ref.LENGTHS)
def test_exact_costs_agree_with_the_reference_formula(n_clusters, cluster_length):
    """Within ``cost_bound`` on every set of the sweep; the labels of the exact first minimum equal ``rp.cluster_1d``'s
    on every separated set, and every such set is separated."""
    for n_offsets in ref.OFFSETS:
        for penalty in ref.PENALTIES:
            for s in ref.point_sets(n_clusters, cluster_length, n_offsets, penalty):
                what = (s["name"], n_clusters, cluster_length, n_offsets, penalty)
                have = reference_costs(s["points"], n_offsets, n_clusters, cluster_length, s["ideal"], penalty)
                assert ref.error_ratio(have, s["exact"], s["bound"]) <= 1.0, what
                if s["separated"]:
                    assert ref.separation(s["exact"], s["bound"]), what
                    total = n_offsets + round(n_clusters * cluster_length)
                    want = rp.cluster_1d(s["points"], total, n_clusters, cluster_length, s["ideal"], penalty)
                    best = first_minimum(s["exact"])
                    np.testing.assert_array_equal(ref.labels_of(s["points"], n_clusters, cluster_length, best), want, str(what))


def test_exact_costs_on_sets_with_a_known_answer():
    """No point inside any cluster: penalty * sum(ideal**2) at every offset.  One point at the centre of its cluster:
    nothing but the penalty terms."""
    for K, L, n_off, penalty in ((1, 7.0, 1, 50), (65, 33.3, 37, 50), (130, 10.5, 2, 0)):
        for s in ref.point_sets(K, L, n_off, penalty):
            if s["name"] in ("left", "right", "none"):
                assert s["exact"] == [Fraction(penalty * int((s["ideal"] ** 2).sum()))] * n_off
                assert (ref.labels_of(s["points"], K, L, 0) == -1).all()
    _, exact = ref.cluster_costs_exact([14.0], 3, 4, 8.0, [1, 1, 0, 2], 50)  # centres 4, 12, ... at offset 0
    assert exact[2] == 50 * (1 + 0 + 0 + 4)  # offset 2: the point is the centre of cluster 1
    assert exact[0] == 4 * (1 + 1 + Fraction(ref._exact_sqrt(2))) + 50 * (1 + 0 + 0 + 4)  # var 4 in cluster 1, taken by the empty ones
    b = ref.boundaries(5, 9.0, 3)[0]
    np.testing.assert_array_equal(ref.labels_of(b, 5, 9.0, 3), [0, 1, 2, 3, 4, -1])  # a boundary starts its cluster


def test_golden_clusters_labels(golden):
    g = golden("clusters")
    for pts, k, length, ideal, want in ((g["y"], 6, float(g["rd"]), g["ideal_r"], g["row_labels"]),
                                        (g["x"], 5, float(g["cd"]), g["ideal_c"], g["col_labels"])):
        n_off = 900 - round(k * length)
        have, exact = ref.cluster_costs_exact(pts, n_off, k, length, ideal, 50)
        bound = ref.cost_bound(pts, n_off, k, length)
        assert ref.separation(exact, bound)
        assert ref.error_ratio(reference_costs(pts, n_off, k, length, ideal, 50), exact, bound) <= 1.0
        np.testing.assert_array_equal(ref.labels_of(pts, k, length, first_minimum(exact)), want)
        np.testing.assert_array_equal(rp.cluster_1d(pts, 900, k, length, ideal, 50), want)


@pytest.mark.parametrize("case", ref.TIES)
def test_hand_made_ties_are_exact(case):
    points, total, k, length, ideal, penalty, (a, b) = case
    n_off = ref.tie_offsets(total, k, length)
    have, exact = ref.cluster_costs_exact(points, n_off, k, length, ideal, penalty)
    assert exact[a] == exact[b] == min(exact) and sorted(exact)[2] > exact[a]
    float_costs = reference_costs(points, n_off, k, length, ideal, penalty)
    assert float_costs[a] == float_costs[b] == float_costs.min() and int(np.argmin(float_costs)) == a
    np.testing.assert_array_equal(rp.cluster_1d(points, total, k, length, ideal, penalty),
                                  ref.labels_of(points, k, length, a))


@pytest.mark.parametrize("L", ref.MASK_LENGTHS)
@pytest.mark.parametrize("inner_r,outer_r", ref.MASK_PAIRS)
def test_mask_oracle_equals_filled_circle_mask(L, inner_r, outer_r):
    centers, radii = ref.mask_markers(L, outer_r)
    fg, bg = ref.button_masks_ref(centers, radii, L, outer_r, inner_r)
    assert fg.dtype == np.uint8 and fg.shape == bg.shape == (len(radii), L, L)
    disks = {}

    def disk(c, r):
        key = (int(c[0]), int(c[1]), int(r))
        if key not in disks:
            disks[key] = rcv.filled_circle_mask((L, L), c, int(r))
        return disks[key]

    for i, (c, r) in enumerate(zip(centers, radii)):
        np.testing.assert_array_equal(fg[i].astype(bool), disk(c, r), f"fg of {c}, {r}")
        np.testing.assert_array_equal(bg[i].astype(bool), disk(c, outer_r) & ~disk(c, inner_r), f"bg of {c}")
    if inner_r >= outer_r:
        assert not bg.any()
    one = ref.button_masks_ref([[L // 2, L // 2]], [100], L, outer_r, inner_r)[0]
    assert one.all()  # radius 100 covers every window here
    empty = ref.button_masks_ref(np.zeros((0, 2)), [], L, outer_r, inner_r)
    assert empty[0].shape == empty[1].shape == (0, L, L)
    for r in range(0, 41):
        np.testing.assert_array_equal(ref.button_masks_ref([[45, 45]], [r], 91, 0, 0)[0][0].astype(bool),
                                      rcv.filled_circle_mask((91, 91), (45, 45), r))
