"""The premises of the suppression tests, without a GPU: the bitmap of D = ring (-) ring that mg_nms_sparse reads is what
it is documented to be, "keep i iff no earlier kept j has c_i - c_j in D" IS filter_neighbors while nothing wraps, the
oracle wrapper reproduces the golden, and the planes the GPU tests run on (tests/nms_ref.py) are hard enough that a wrong
kernel cannot pass them by luck."""
import math

import numpy as np
import pytest

import nms_ref as nr
from oracle import ref_numeric as rn


@pytest.mark.parametrize("d", range(1, 17))
def test_difference_bitmap_is_ring_minus_ring(d):
    """Bit (dr, dc) is set iff the ring and the ring shifted by (dr, dc) share a cell: brute force over the whole square.
    For d >= 2 some offset of the square is NOT in D (rings, not disks; the square's corners at the least)."""
    from magnify_amd import _native as nat

    ring = rn.circle_points(d, four_connected=True)
    np.testing.assert_array_equal(nat.circle_points(d, True), ring)
    cells = {(int(r), int(c)) for r, c in ring}
    table = nr.difference_table(d)
    want = np.zeros_like(table)
    for dr in range(-2 * d, 2 * d + 1):
        for dc in range(-2 * d, 2 * d + 1):
            want[dr + 2 * d, dc + 2 * d] = any((r + dr, c + dc) in cells for r, c in cells)
    np.testing.assert_array_equal(table, want)
    assert table[2 * d, 2 * d]  # a ring meets itself
    np.testing.assert_array_equal(table, table[::-1, ::-1])  # D = -D
    if d >= 2:
        assert not table.all()
    else:
        assert table.all()  # d = 1: the ring is the 8-neighbourhood, D the whole 5 x 5 square


def _no_wrap_planes():
    for d in nr.SPARSE_DISTS:
        for name, (plane, _) in nr.sparse_planes(d).items():
            if len(plane.circles) and not nr.wraps(plane, d):
                yield f"sparse {name} d={d}", plane, d
    for d in sorted(set(nr.GRID_DISTS + nr.STAGE_DISTS)):
        for seed in (0, 1):
            for k, plane in enumerate(nr.grid_planes(d, seed)):
                if len(plane.circles) and not nr.wraps(plane, d):
                    yield f"grid {k} seed={seed} d={d}", plane, d


def test_difference_rule_is_filter_neighbors():
    """Without a wrap, the sparse kernel's rule and the claim grid decide alike, on every such plane of the builders."""
    n = 0
    for what, plane, d in _no_wrap_planes():
        c = plane.circles[nr.priority_order(plane.scores, plane.keys)]
        np.testing.assert_array_equal(nr.greedy_by_differences(c, d), rn.filter_neighbors(c, d), err_msg=what)
        n += 1
    assert n >= 40


def test_expected_reproduces_the_golden(golden):
    g = golden("filter_neighbors")
    for case in range(4):
        c = g[f"circles_{case}"].astype(np.int32)
        n = len(c)
        scores = np.linspace(1.0, 0.5, n).astype(np.float32)
        assert (np.diff(scores) < 0).all()
        alive = np.random.default_rng(case).permutation(n)
        state, rows, kept_scores = nr.expected(c, scores, None, alive, int(g[f"min_dist_{case}"]))
        valid = g[f"valid_{case}"]
        np.testing.assert_array_equal(state, np.where(valid, 1, 2))
        np.testing.assert_array_equal(rows, c[valid])
        np.testing.assert_array_equal(kept_scores, scores[valid])
    # no suppression: every alive circle, in order
    state, rows, _ = nr.expected(c, scores, None, alive[:10], 0)
    assert state.sum() == 10
    np.testing.assert_array_equal(rows, c[np.sort(alive[:10])])


def test_priority_order_takes_keys_as_unsigned():
    scores = np.array([0.5, 0.5, 0.5, 0.7], dtype=np.float32)
    keys = np.array([0x80000001, 5, 0xFFFFFFFF, 0x90000000], dtype=np.uint32)
    assert nr.priority_order(scores, keys).tolist() == [3, 1, 0, 2]
    assert nr.priority_order(scores, keys.view(np.int32).astype(np.int64).astype(np.uint32)).tolist() == [3, 1, 0, 2]
    assert nr.priority_order(scores, None).tolist() == [3, 0, 1, 2]


def _crowded_planes():
    for d in nr.SPARSE_DISTS:
        for name in ("full", "big"):
            yield f"sparse {name} d={d}", nr.sparse_planes(d)[name][0], d, (nr.H, nr.W) if name == "full" else (3008, 6080)
    for d in sorted(set(nr.GRID_DISTS + nr.STAGE_DISTS)):
        for seed in (0, 1):
            yield f"grid crowded seed={seed} d={d}", nr.grid_planes(d, seed)[0], d, (nr.H, nr.W)


def test_crowded_planes_are_crowded():
    """Every crowded plane keeps between 10 % and 90 % of its circles, has >= 100 conflicting pairs with equal float32
    scores, >= 100 pairs inside the reach square that are not in D, and twenty circles on one centre.  Two exceptions that
    no plane can avoid: for d = 1 the square IS D (asserted above), so there is no such pair; and kept circles of one
    radius are a packing of discs of radius d (rings within 2 d of each other meet), at most A / (2 sqrt(3) d^2) of them
    over the extent A the centres range over -- where 10 % of the plane exceeds that (12 288 circles on 700 x 900 at
    d = 15: at most 825 can be kept), the plane must keep 100 circles instead."""
    seen = 0
    for what, plane, d, (h, w) in _crowded_planes():
        got = nr.conditions(plane, d)
        n = len(plane.circles)
        packing = (h + d + 1) * (w + d + 1) / (2 * math.sqrt(3) * d * d)
        print(what, n, got, f"packing bound {packing:.0f}")
        if 0.1 * n <= packing:
            assert 0.1 <= got["share"] <= 0.9, (what, got)
        else:
            assert (d, n, (h, w)) == (15, nr.SPARSE_CAP, (nr.H, nr.W)), what  # the one plane this is true of
            assert got["kept"] >= 100 and got["share"] <= 0.9, (what, got)
        assert got["equal_conflicts"] >= 100, (what, got)
        assert got["not_in_d"] >= (100 if d >= 2 else 0), (what, got)
        assert got["same_centre"] >= 20, (what, got)
        keys = plane.keys
        assert len(np.unique(keys)) == n and (keys >> 31).mean() >= 0.5, what
        seen += 1
    assert seen == 2 * len(nr.SPARSE_DISTS) + 2 * len(set(nr.GRID_DISTS + nr.STAGE_DISTS))


def test_limit_planes_are_at_their_limits():
    """The planes of the mg_nms_sparse launch sit where they are meant to: bucket counts, circle counts, the centres at
    and past -(d + 1), the understated extent, the straddling pairs, the chains."""
    for d in nr.SPARSE_DISTS:
        planes = nr.sparse_planes(d)
        count = {name: len(p.circles) for name, (p, _) in planes.items()}
        assert count["full"] == nr.SPARSE_CAP and count["over"] == nr.SPARSE_CAP + 1 and count["big"] == nr.SPARSE_CAP
        assert count["empty"] == 0 and max(count.values()) < nr.SPARSE_LIST_CAP
        assert nr.sparse_buckets(planes["big"][0]) == (96, 96) and 96 * 96 == nr.SPARSE_MAXB
        assert nr.sparse_buckets(planes["big_over"][0]) == (96, 97)
        assert nr.sparse_buckets(planes["per2_even"][0]) == (37, 34) and nr.sparse_buckets(planes["per2_odd"][0]) == (37, 35)
        big = planes["big"][0].circles
        for corner in ([-(d + 1), -(d + 1)], [-(d + 1), 6079], [3007, -(d + 1)], [3007, 6079]):
            assert (big[:, :2] == corner).all(axis=1).any()
        for name, (p, done) in planes.items():
            if not len(p.circles):
                continue
            c = p.circles
            inside = (c[:, 0] <= p.max_rc[0]).all() and (c[:, 1] <= p.max_rc[1]).all()
            assert inside == (name != "understated"), name
            assert nr.wraps(p, d) == (name == "past_edge"), name
            nbr, nbc = nr.sparse_buckets(p)
            assert done == int(len(c) <= nr.SPARSE_CAP and nbr * nbc <= nr.SPARSE_MAXB and inside and not nr.wraps(p, d)), name
        edge = planes["at_edge"][0].circles
        assert edge[:, 0].min() == -(d + 1) == edge[:, 1].min()
        past = planes["past_edge"][0].circles
        assert past[:, 0].min() == -(d + 2) and (past[1:] == planes["at_edge"][0].circles[1:]).all()
        under = planes["understated"][0]
        assert under.circles[:, 0].max() == under.max_rc[0] + 1
        # border pairs: both circles of a pair in different buckets; pairs at 2 d conflict, at 2 d + 1 do not
        b = planes["border"][0].circles.astype(np.int64)
        a0, a1 = b[0::2, :2], b[1::2, :2]
        crossed_r = (a0[:, 0] + 64) // nr.BUCKET_R != (a1[:, 0] + 64) // nr.BUCKET_R
        crossed_c = (a0[:, 1] + 64) // nr.BUCKET_C != (a1[:, 1] + 64) // nr.BUCKET_C
        assert (crossed_r | crossed_c).all() and (crossed_r & ~crossed_c).sum() >= 8 and (~crossed_r & crossed_c).sum() >= 2
        assert (crossed_r & crossed_c).sum() >= 4
        diff = a1 - a0
        in_d = nr.difference_table(d)[np.clip(diff[:, 0], -2 * d, 2 * d) + 2 * d, np.clip(diff[:, 1], -2 * d, 2 * d) + 2 * d]
        far = np.abs(diff).max(axis=1) > 2 * d
        assert far.sum() == 8 and in_d[~far].all()  # (at d = 1 a diagonal pair is at (1, 1): in D as well)
        order = nr.priority_order(planes["border"][0].scores, planes["border"][0].keys)
        keep = np.empty(len(b), dtype=bool)
        keep[order] = rn.filter_neighbors(b[order], d)
        assert (keep[0::2] & keep[1::2]).tolist() == far.tolist()  # no pair is within reach of another pair
        # the chain: on one row in this launch, every third circle kept, each link within reach of the one before
        ch = planes["chain"][0]
        first = ch.circles[: nr.CHAIN_LEN]
        assert (first[:, 0] == first[0, 0]).all() and (np.diff(first[:, 1]) == d).all()
        order = nr.priority_order(ch.scores, ch.keys)
        assert order[: nr.CHAIN_LEN].tolist() == list(range(nr.CHAIN_LEN))
        assert order[nr.CHAIN_LEN:].tolist() == list(range(len(ch.circles) - 1, nr.CHAIN_LEN - 1, -1))
        keep = np.empty(len(ch.circles), dtype=bool)
        keep[order] = rn.filter_neighbors(ch.circles[order], d)
        assert keep[: nr.CHAIN_LEN].tolist() == [k % 3 == 0 for k in range(nr.CHAIN_LEN)]
        assert keep[nr.CHAIN_LEN:][::-1].tolist() == [k % 3 == 0 for k in range(nr.CHAIN2_LEN)]
    for d in nr.GRID_DISTS:
        for seed in (0, 1):
            crowded, wrap, empty, chain = nr.grid_planes(d, seed)
            assert nr.wraps(wrap, d) and wrap.max_rc[0] == nr.H + 20 and not nr.wraps(crowded, d) and not len(empty.circles)
            assert len(crowded.circles) == nr.GRID_N and chain.max_rc[0] < nr.H and chain.max_rc[1] < nr.W
            # folded or not, consecutive circles of the chain are d apart
            step = np.abs(np.diff(chain.circles[: nr.CHAIN_LEN, :2].astype(np.int64), axis=0))
            assert (step.sum(axis=1) == d).all()
