"""The prefilter's perimeter walk (mg_score.hip, Walk<R>) as the host sees it: mg_score_walk_reads(r) is the number of
LDS byte reads of the walk of radius r, taken from the structure the kernel is instantiated from.  A window byte
carries a pixel and its right neighbour, so a maximal horizontal run of L perimeter points costs ceil(L / 2) reads."""
import numpy as np
import pytest

from magnify_amd import _native as nat


def _perimeter(r):
    first = nat.score_pairs(r).astype(np.int64)
    return first, np.concatenate([first, -first])


def _paired_reads(points):
    """Sum of ceil(L / 2) over the maximal runs of consecutive columns of every row."""
    reads = 0
    for row in np.unique(points[:, 0]):
        cols = np.sort(points[points[:, 0] == row, 1])
        runs = np.split(cols, np.nonzero(np.diff(cols) != 1)[0] + 1)
        reads += sum((len(run) + 1) // 2 for run in runs)
    return reads


@pytest.mark.parametrize("r", range(2, 27))
def test_walk_reads_match_the_horizontal_runs(r):
    first, points = _perimeter(r)
    assert len(np.unique(points, axis=0)) == len(points) == 2 * len(first)  # all distinct
    reads = nat.lib().mg_score_walk_reads(r)
    assert reads == _paired_reads(points)
    assert reads <= 2 * len(first)
    want = {5: 26, 10: 46, 15: 70, 20: 90, 25: 114}
    if r in want:
        assert reads == want[r]


def test_walk_reads_outside_the_supported_radii():
    for r in (-3, 0, 1, 27, 100):
        assert nat.lib().mg_score_walk_reads(r) == 0


def test_walk_reads_sum_over_the_documented_range():
    """R = 5..25: 1462 reads against 1820 points, -19.7 %."""
    reads = sum(nat.lib().mg_score_walk_reads(r) for r in range(5, 26))
    points = sum(2 * len(nat.score_pairs(r)) for r in range(5, 26))
    assert (reads, points) == (1462, 1820)
