"""tests/roi_ref.py is what the GPU tests of the ROI pass compare with; here it is held to the oracle it restates:
rn.circle_labels + rn.bounding_box + rp.roi_reduce, and the golden circle_labels fixture."""
import math

import numpy as np
import pytest

import roi_ref
from oracle import ref_numeric as rn
from oracle import ref_pipeline as rp


def random_assays(rng, h, w, sizes, r_lo=2, r_hi=14):
    return [np.column_stack([rng.integers(-5, h + 5, n), rng.integers(-5, w + 5, n), rng.integers(r_lo, r_hi, n)])
            for n in sizes]


def oracle_route(images, assays, L):
    """The same outputs by the oracle's own functions, marker by marker."""
    A, C, T, h, w = images.shape
    rois, fgs, bgs = [], [], []
    for a, beads in enumerate(assays):
        lab = rn.circle_labels(beads, h, w)
        for i, (row, col, _) in enumerate(beads):
            top, bottom, left, right = rn.bounding_box(int(col), int(row), L, w, h)
            rois.append(images[a, :, :, top:bottom, left:right])
            fgs.append(lab[top:bottom, left:right] == i)
            bgs.append(lab[top:bottom, left:right] == -1)
    roi, fg, bg = np.stack(rois), np.stack(fgs), np.stack(bgs)
    red = rp.roi_reduce(roi, np.repeat(fg[:, None], T, axis=1), np.repeat(bg[:, None], T, axis=1), medians=False)
    return roi, fg, bg, red


@pytest.mark.parametrize("dtype,L,time_major", [(np.uint16, 40, False), (np.uint16, 33, True), (np.uint8, 2, False),
                                                (np.float32, 41, False), (np.float64, 16, True)])
def test_roi_ref_equals_oracle(dtype, L, time_major):
    rng = np.random.default_rng(7)
    C, T, h, w = 3, 2, 90, 110
    assays = random_assays(rng, h, w, (25, 0, 12))
    A = len(assays)
    if np.dtype(dtype).kind == "f":
        images = (rng.choice([-1.0, 1.0], (A, C, T, h, w)) * 10.0 ** rng.uniform(-3, 6, (A, C, T, h, w))).astype(dtype)
    else:
        images = rng.integers(0, np.iinfo(dtype).max + 1, (A, C, T, h, w)).astype(dtype)
    given = images.transpose(0, 2, 1, 3, 4).copy() if time_major else images
    ref = roi_ref.roi_ref(given, assays, L, 14, time_major=time_major)
    roi, fg, bg, red = oracle_route(images, assays, L)
    np.testing.assert_array_equal(ref["roi"], roi)
    assert ref["roi"].dtype == images.dtype
    np.testing.assert_array_equal(ref["fg"], fg)
    np.testing.assert_array_equal(ref["bg"], bg)
    np.testing.assert_array_equal(ref["counts"][:, 0], red["fg_count"][:, 0])
    np.testing.assert_array_equal(ref["counts"][:, 1], red["bg_count"][:, 0])
    assert ref["fg"].any() and ref["bg"].any() and (ref["labels"] == -2).any()
    if images.dtype.kind == "f":
        # numpy's pairwise float64 sum against fsum: within the recursive-summation bound, far inside it in fact
        for k, name in enumerate(("fg_sum", "bg_sum")):
            n = ref["counts"][:, k][:, None, None]
            assert (np.abs(ref["sums"][..., k] - red[name]) <= n * 2.0 ** -52 * ref["abs_sums"][..., k]).all()
        g = int(np.argmax(ref["counts"][:, 0]))
        vals = ref["roi"][g, 1, 1][ref["fg"][g].astype(bool)].astype(np.float64)
        assert ref["sums"][g, 1, 1, 0] == math.fsum(vals) and ref["abs_sums"][g, 1, 1, 0] == math.fsum(np.abs(vals))
    else:
        assert ref["sums"].dtype == np.int64
        np.testing.assert_array_equal(ref["sums"][..., 0], red["fg_sum"])
        np.testing.assert_array_equal(ref["sums"][..., 1], red["bg_sum"])


def test_ownership_equals_golden_labels(golden):
    g = golden("circle_labels")
    h, w = (int(v) for v in g["shape"])
    lab = roi_ref.ownership(g["beads"], h, w, int(g["beads"][:, 2].max()))
    assert lab.dtype == np.int32
    np.testing.assert_array_equal(lab, g["labels"])
    np.testing.assert_array_equal(lab, rn.circle_labels(g["beads"], h, w))


def test_excluded_radii_cover_nothing_and_keep_their_index():
    """With radii below 2 or above max_r in the table: the oracle's route on the remaining beads, indices mapped back."""
    rng = np.random.default_rng(8)
    C, T, h, w, L, max_r = 2, 1, 80, 100, 30, 9
    beads = random_assays(rng, h, w, (40,), r_lo=-1, r_hi=13)[0]
    beads[:4] = [[40, 50, 9], [42, 52, 1], [44, 54, 10], [40, 50, 0]]  # excluded beads inside a drawn disk
    keep = np.nonzero((beads[:, 2] >= 2) & (beads[:, 2] <= max_r))[0]
    assert 0 < len(keep) < len(beads) and (beads[:, 2] < 2).any() and (beads[:, 2] > max_r).any()
    images = rng.integers(0, 65536, (1, C, T, h, w)).astype(np.uint16)
    ref = roi_ref.roi_ref(images, [beads], L, max_r)
    lab = rn.circle_labels(beads[keep], h, w)
    back = np.where(lab >= 0, keep[np.clip(lab, 0, None)], lab)
    np.testing.assert_array_equal(ref["labels"][0], back)
    kept = roi_ref.roi_ref(images, [beads[keep]], L, max_r)
    for j, i in enumerate(keep):
        for name in ("roi", "fg", "bg", "counts", "sums", "windows"):
            np.testing.assert_array_equal(ref[name][i], kept[name][j])
    for i in np.setdiff1d(np.arange(len(beads)), keep):  # an excluded marker: no foreground, background as everyone's
        top, left = ref["windows"][i]
        assert not ref["fg"][i].any() and ref["counts"][i, 0] == 0 and not ref["sums"][i, ..., 0].any()
        np.testing.assert_array_equal(ref["bg"][i], back[top:top + L, left:left + L] == -1)
        np.testing.assert_array_equal(ref["roi"][i], images[0, :, :, top:top + L, left:left + L])


def test_window_order_ref():
    beads = np.array([[70, 5, 3], [3, 9, 3], [-4, 9, 3], [63, 2, 3], [64, 1, 3], [1 << 21, 0, 3], [5, 1 << 18, 3], [5, -7, 3]])
    got = roi_ref.window_order_ref([beads[:0], beads, beads[:3]], 10, np.full(12, -1))
    # band 0: cols -7 -> 0 (7), 2 (3), 9 (1, 2 in table order), 2^17 - 1 (6); band 1: 1 (4), 5 (0); last band: 5
    np.testing.assert_array_equal(got, [7, 3, 1, 2, 6, 4, 0, 5, 9, 8, -1, -1])
    big = np.column_stack([np.arange(8193)[::-1], np.zeros(8193, int), np.full(8193, 3)])
    np.testing.assert_array_equal(roi_ref.window_order_ref([big], 8193, np.zeros(8193)), np.arange(8193))
    assert roi_ref.window_order_ref([big], 8192, np.zeros(8193))[0] != 0  # cut to the cap by the bound: ordered


def test_counts_to_offsets_ref():
    np.testing.assert_array_equal(roi_ref.counts_to_offsets_ref([3, -2, 0, 9, 5], 5), [0, 3, 3, 3, 8, 13])
    np.testing.assert_array_equal(roi_ref.counts_to_offsets_ref([], 5), [0])


def test_marker_table_ref():
    assays = [np.array([[1, 2, 3]]), np.empty((0, 3), int), np.array([[4, 5, 6], [7, 8, 9]])]
    counts = np.arange(6).reshape(3, 2)
    sums = np.arange(3 * 2 * 3 * 2, dtype=np.float64).reshape(3, 2, 3, 2)
    tab = roi_ref.marker_table_ref(assays, 10, counts, sums, 2)
    np.testing.assert_array_equal(tab[2], [12, 7, 8, 9, 4, 5, sums[2, 0, 2, 0], sums[2, 1, 2, 0], sums[2, 0, 2, 1], sums[2, 1, 2, 1]])
    np.testing.assert_array_equal(tab[0, :6], [10, 1, 2, 3, 0, 1])
