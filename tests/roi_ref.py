"""The ROI pass restated in NumPy: what mg_roi_segment_reduce / mg_roi_gather_reduce_batched, mg_roi_window_order,
mg_counts_to_offsets and mg_marker_table have to return, written as plainly as include/magnify_hip.h states it.

Windows come from ``ref_numeric.bounding_box``; ownership is computed as ``ref_numeric.circle_labels`` computes it,
from ``filled_circle_points`` -- with the one rule of the header that ``circle_labels`` cannot express: a bead with
r < 2 or r > max_r covers nothing, contests nothing and keeps its index.  Integer sums are exact (int64); float sums are
``math.fsum`` of the float64 values, and come with the sum of the absolute values for a derived error bound.
tests/test_cpu_roi_ref.py anchors all of it to the oracle."""
import math

import numpy as np

from oracle import ref_numeric as rn

ORDER_CAP = 8192  # an assay with more markers keeps its order
ORDER_BAND = 6    # log2 of the band height


def ownership(beads, h, w, max_r):
    """rn.circle_labels of the beads (n, 3) [row, col, r], the beads with r < 2 or r > max_r left out of the drawing
    but not of the numbering."""
    beads = np.asarray(beads, dtype=np.int64).reshape(-1, 3)
    labels = np.full((h, w), -1, dtype=np.int32)
    for i, (row, col, r) in enumerate(beads):
        if r < 2 or r > max_r:
            continue
        pts = rn.filled_circle_points(int(r)) + np.array([row, col], dtype=np.int64)
        ok = (pts[:, 0] >= 0) & (pts[:, 0] < h) & (pts[:, 1] >= 0) & (pts[:, 1] < w)
        rr, cc = pts[ok, 0], pts[ok, 1]
        taken = labels[rr, cc] != -1
        labels[rr[taken], cc[taken]] = -2
        labels[rr[~taken], cc[~taken]] = i
    return labels


def windows(beads, L, h, w):
    """(n, 2) [top, left] of the beads' L x L windows."""
    beads = np.asarray(beads, dtype=np.int64).reshape(-1, 3)
    out = np.zeros((len(beads), 2), dtype=np.int64)
    for i, (row, col, _) in enumerate(beads):
        top, bottom, left, right = rn.bounding_box(int(col), int(row), L, w, h)
        assert bottom - top == L and right - left == L and top >= 0 and left >= 0 and bottom <= h and right <= w
        out[i] = top, left
    return out


def roi_ref(images, assays, L, max_r, time_major=False, labels=None):
    """images (A, C, T, h, w), or (A, T, C, h, w) with ``time_major``; assays: one (n_a, 3) bead table per assay.
    ``labels`` (A, h, w): the ownership maps to use instead of computing them (label mode hands the kernel a map).

    Returns roi (M, C, T, L, L), fg / bg (M, L, L) uint8, counts (M, 2) int32 and sums (M, C, T, 2) [fg, bg] -- int64
    for integer pixels, the fsum as float64 for float pixels; plus abs_sums (M, C, T, 2) float64 (sum of |v| under the
    mask), windows (M, 2) [top, left] and labels (A, h, w)."""
    images = np.asarray(images)
    if time_major:
        images = images.transpose(0, 2, 1, 3, 4)
    A, C, T, h, w = images.shape
    assert len(assays) == A
    is_float = images.dtype.kind == "f"
    M = sum(len(b) for b in assays)
    out = {
        "roi": np.zeros((M, C, T, L, L), dtype=images.dtype),
        "fg": np.zeros((M, L, L), dtype=np.uint8),
        "bg": np.zeros((M, L, L), dtype=np.uint8),
        "counts": np.zeros((M, 2), dtype=np.int32),
        "sums": np.zeros((M, C, T, 2), dtype=np.float64 if is_float else np.int64),
        "abs_sums": np.zeros((M, C, T, 2), dtype=np.float64),
        "windows": np.zeros((M, 2), dtype=np.int64),
        "labels": np.full((A, h, w), -1, dtype=np.int32),
    }
    g = 0
    for a, beads in enumerate(assays):
        beads = np.asarray(beads, dtype=np.int64).reshape(-1, 3)
        lab = ownership(beads, h, w, max_r) if labels is None else np.asarray(labels[a])
        out["labels"][a] = lab
        for i, (top, left) in enumerate(windows(beads, L, h, w)):
            sub = lab[top:top + L, left:left + L]
            masks = (sub == i, sub == -1)
            win = images[a, :, :, top:top + L, left:left + L]
            out["roi"][g] = win
            out["fg"][g], out["bg"][g] = masks
            out["counts"][g] = masks[0].sum(), masks[1].sum()
            out["windows"][g] = top, left
            for k, mask in enumerate(masks):
                if is_float:
                    vals = win[:, :, mask].astype(np.float64)  # (C, T, n)
                    for c in range(C):
                        for t in range(T):
                            out["sums"][g, c, t, k] = math.fsum(vals[c, t])
                            out["abs_sums"][g, c, t, k] = math.fsum(np.abs(vals[c, t]))
                else:
                    vals = win[:, :, mask].astype(np.int64)
                    out["sums"][g, :, :, k] = vals.sum(axis=-1)
                    out["abs_sums"][g, :, :, k] = vals.sum(axis=-1)
            g += 1
    return out


def window_order_ref(assays, m, order):
    """mg_roi_window_order: ``order`` (the array as it was before the call, at least m long) with the markers of every
    assay in stable order of their key -- band of 64 rows, then column -- written to it.  Markers at or beyond the
    bound m are untouched; an assay with more than ORDER_CAP markers (below the bound) keeps its order."""
    order = np.array(order, dtype=np.int32)
    first = 0
    for beads in assays:
        beads = np.asarray(beads, dtype=np.int64).reshape(-1, 3)
        n = min(first + len(beads), m) - first
        if n > ORDER_CAP:
            order[first:first + n] = first + np.arange(n)
        elif n > 0:
            key = ((np.clip(beads[:n, 0], 0, (1 << 20) - 1) >> ORDER_BAND) << 17) | np.clip(beads[:n, 1], 0, (1 << 17) - 1)
            order[first:first + n] = first + np.argsort(key, kind="stable")
        first += len(beads)
    return order


def counts_to_offsets_ref(counts, cap):
    """mg_counts_to_offsets: (n + 1,) exclusive prefix sums of the counts cut to [0, cap]."""
    cut = np.clip(np.asarray(counts, dtype=np.int64), 0, cap)
    return np.concatenate([[0], np.cumsum(cut)]).astype(np.int32)


def marker_table_ref(assays, assay_offset, counts, sums, t_index):
    """mg_marker_table: rows [assay_offset + assay, row, col, r, fg_count, bg_count, fg_sum[C], bg_sum[C]] (float64) of
    all markers, from counts (M, 2) and sums (M, C, T, 2) at time index t_index."""
    counts, sums = np.asarray(counts), np.asarray(sums)
    M, C = sums.shape[:2]
    table = np.zeros((M, 6 + 2 * C), dtype=np.float64)
    g = 0
    for a, beads in enumerate(assays):
        for bead in np.asarray(beads, dtype=np.int64).reshape(-1, 3):
            table[g, 0] = assay_offset + a
            table[g, 1:4] = bead
            table[g, 4:6] = counts[g]
            table[g, 6:6 + C] = sums[g, :, t_index, 0]
            table[g, 6 + C:] = sums[g, :, t_index, 1]
            g += 1
    assert g == M
    return table
