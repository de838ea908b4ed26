"""NumPy restatement of ``magnify_amd.plot.percentile_limits`` and ``magnify_amd.plot.roishow`` (DESIGN.md, section
19): the exact lower order statistic at an integer rank, the layout of the montage and the montage itself.  The kernels
(csrc/mg_percentile.hip, csrc/mg_montage.hip) are held to it bit for bit; it is itself held to plain loops by
tests/test_cpu_roishow.py.  Everything runs in float64, one operation at a time.  Below ``s = 2**level`` and ``lk =
ceil(L / s)``, the side of a cell."""
import math

import numpy as np

import plot_ref as pr

BG_RGB, FG_RGB = (255.0, 0.0, 0.0), (0.0, 255.0, 0.0)


def percentile_rank(n, q):
    """``q`` in thousandths of a percent; the rank in Python integers."""
    qm = round(float(q) * 1000)
    assert 0 <= qm <= 100000 and n >= 1
    return (int(n) - 1) * qm // 100000


def percentile(values, q):
    """``sorted(non-NaN values)[percentile_rank(N, q)]`` as float64; float64 values are rounded to float32 first."""
    v = np.asarray(values).reshape(-1)
    if v.dtype == np.float64:
        with np.errstate(over="ignore"):
            v = v.astype(np.float32)
    if v.dtype.kind == "f":
        v = v[~np.isnan(v)]
    if v.size == 0:
        raise ValueError("no value that is not NaN")
    return np.float64(np.sort(v)[percentile_rank(v.size, q)])


def percentile_limits(stack, lo, hi):
    """stack (C, ...): per channel (percentile lo, percentile hi) over everything else, float64 (C, 2)."""
    return np.array([[percentile(chan, lo), percentile(chan, hi)] for chan in stack], dtype=np.float64)


def montage_layout(tags, m, columns=None):
    """int32 (rows, cols) mark of every cell, -1 where there is none (plot/image.py:16-23 with tags)."""
    if m == 0:
        return np.zeros((0, 0), dtype=np.int32)
    if tags is not None:
        tags = np.asarray(tags).reshape(-1)
        names, counts = np.unique(tags, return_counts=True)
        layout = np.full((counts.max(), len(names)), -1, dtype=np.int32)
        for j, name in enumerate(names):
            marks = [i for i in range(m) if tags[i] == name]
            layout[:len(marks), j] = marks
        return layout
    if columns is None:
        columns = math.ceil(math.sqrt(m))
    rows = math.ceil(m / columns)
    layout = np.full((rows, columns), -1, dtype=np.int32)
    for i in range(m):
        layout[i // columns, i % columns] = i
    return layout


def default_level(rows, cols, L):
    for level in range(7):
        lk = math.ceil(L / (1 << level))
        if rows * lk * cols * lk <= 1024 ** 2:
            return level
    return 6


def block_any(mask, level):
    """(lk, lk) bool: any set pixel of the L x L mask in every s x s block."""
    L = mask.shape[0]
    s = 1 << level
    lk = -(L // -s)
    padded = np.zeros((lk * s, lk * s), dtype=bool)
    padded[:L, :L] = mask
    return padded.reshape(lk, s, lk, s).any(axis=(1, 3))


def roishow(roi, layout, level, limits, colors, fg=None, bg=None, overlay="fill", alpha=0.7):
    """roi (M, C, T, L, L), layout (rows, cols), fg / bg (M, T, L, L) bool or None -> uint8 (T, rows lk, cols lk, 3)."""
    m, n_c, n_t, L, _ = roi.shape
    rows, cols = layout.shape
    s = 1 << level
    lk = -(L // -s)
    acc = np.zeros((n_t, rows * lk, cols * lk, 3), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(rows):
            for cc in range(cols):
                g = layout[r, cc]
                if g < 0:
                    continue
                cell = acc[:, r * lk:(r + 1) * lk, cc * lk:(cc + 1) * lk]  # a view
                for c in range(n_c):
                    lo, hi = np.float64(limits[c][0]), np.float64(limits[c][1])
                    for t in range(n_t):
                        total, n = pr.block_sums(roi[g, c, t], level)
                        mean = total / n
                        u = (mean - lo) / (hi - lo)
                        u = np.where(np.isnan(u) | (u < 0) | (not hi > lo), 0.0, u)
                        u = np.where(u > 1, 1.0, u)
                        for j in range(3):
                            cell[t, ..., j] = np.minimum(cell[t, ..., j] + u * np.float64(colors[c][j]), 1.0)
                if overlay not in ("fill", "outline"):
                    continue
                for mask, rgb in ((bg, BG_RGB), (fg, FG_RGB)):
                    if mask is None:
                        continue
                    for t in range(n_t):
                        on = block_any(mask[g, t], level)
                        a = np.float64(alpha)
                        if overlay == "outline":
                            pad = np.pad(on, 1)
                            on = on & ~(pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:])
                            a = np.float64(1.0)
                        mixed = (1.0 - a) * cell[t] + (a * np.array(rgb, dtype=np.float64)) / 255.0
                        cell[t] = np.where(on[..., None], mixed, cell[t])
    return np.floor(255.0 * acc + 0.5).astype(np.uint8)


def scene(dtype, L, seed=0, n_t=2, per_time=True):
    """The 5-mark scene: roi (5, 2, n_t, L, L) of ``dtype``, fg / bg (5, n_t, L, L), tags ["b", "a", "b", "", "b"].
    fg and bg overlap (marks 0 .. 2), fg of mark 3 is empty, bg of mark 4 is the whole window; with ``per_time`` the
    masks of timepoint 1 differ from those of timepoint 0."""
    rng = np.random.default_rng(seed + 7 * L)
    if np.dtype(dtype).kind == "u":
        roi = rng.integers(0, np.iinfo(dtype).max + 1, size=(5, 2, n_t, L, L)).astype(dtype)
    else:
        roi = (rng.random((5, 2, n_t, L, L)) * 1e4 - 3e3).astype(dtype)
    fg = np.zeros((5, n_t, L, L), dtype=bool)
    bg = np.zeros((5, n_t, L, L), dtype=bool)
    speckle = rng.random((n_t, L, L)) < 0.1
    for t in range(n_t):
        d = t if per_time else 0
        for i in range(3):
            fg[i, t] = pr.disk(L, L / 2 + d, L / 2 - i, L / 4 + i)
            bg[i, t] = pr.disk(L, L / 2, L / 2 + d, L / 2.5 + i) & ~pr.disk(L, L / 2, L / 2, L / 6)
        bg[3, t] = speckle[d]
        bg[4, t] = True
        fg[4, t] = pr.disk(L, L - 1, 0, L / 3 + d)
    return roi, fg, bg, np.array(["b", "a", "b", "", "b"])
