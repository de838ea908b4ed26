"""``plot.roishow`` / ``plot.percentile_limits`` without a GPU: the NumPy restatement (tests/roishow_ref.py) against
plain loops, ``montage_layout`` against the reference's grouping written out (plot/image.py:16-23), the integer rank,
and the argument errors that are raised before the device is needed.

tests/test_gpu_percentile.py and tests/test_gpu_roishow.py hold the kernels to the same restatement bit for bit."""
import math

import numpy as np
import pytest

import roishow_ref as rr
from magnify_amd import _native as nat
from magnify_amd import plot


# ---- the oracle against loops ---------------------------------------------------------------------------------------


def loop_roishow(roi, layout, level, limits, colors, fg, bg, overlay, alpha):
    m, n_c, n_t, L, _ = roi.shape
    s = 1 << level
    lk = math.ceil(L / s)
    rows, cols = layout.shape
    out = np.zeros((n_t, rows * lk, cols * lk, 3), dtype=np.uint8)

    def on(mask, by, bx):
        if mask is None or not (0 <= by < lk and 0 <= bx < lk):
            return False
        return bool(mask[by * s:(by + 1) * s, bx * s:(bx + 1) * s].any())

    for t in range(n_t):
        for Y in range(rows * lk):
            for X in range(cols * lk):
                g = layout[Y // lk, X // lk]
                if g < 0:
                    continue
                by, bx = Y % lk, X % lk
                acc = [0.0, 0.0, 0.0]
                for c in range(n_c):
                    block = roi[g, c, t, by * s:(by + 1) * s, bx * s:(bx + 1) * s]
                    total = 0.0
                    for row in block:
                        for v in row:
                            total = total + float(v)
                    mean = total / block.size
                    lo, hi = float(limits[c][0]), float(limits[c][1])
                    u = (mean - lo) / (hi - lo) if hi != lo else 0.0
                    if not hi > lo or not u >= 0.0:
                        u = 0.0
                    u = min(u, 1.0)
                    for j in range(3):
                        acc[j] = min(acc[j] + u * float(colors[c][j]), 1.0)
                if overlay in ("fill", "outline"):
                    for masks, rgb in ((bg, (255.0, 0.0, 0.0)), (fg, (0.0, 255.0, 0.0))):
                        mk = None if masks is None else masks[g, t]
                        hit, a = on(mk, by, bx), float(alpha)
                        if overlay == "outline":
                            hit = hit and not (on(mk, by - 1, bx) and on(mk, by + 1, bx) and on(mk, by, bx - 1)
                                               and on(mk, by, bx + 1))
                            a = 1.0
                        if hit:
                            acc = [(1.0 - a) * acc[j] + (a * rgb[j]) / 255.0 for j in range(3)]
                out[t, Y, X] = [math.floor(255.0 * acc[j] + 0.5) for j in range(3)]
    return out


@pytest.mark.parametrize("overlay", ["fill", "outline", "none"])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_the_restatement_equals_plain_loops(dtype, level, overlay):
    roi, fg, bg, _ = rr.scene(dtype, 7)
    roi, fg, bg = roi[:3], fg[:3], bg[:3]
    layout = rr.montage_layout(np.array(["b", "a", "b"]), 3)
    np.testing.assert_array_equal(layout, [[1, 0], [-1, 2]])
    limits = [(float(np.quantile(roi[:, c], 0.25)), float(np.quantile(roi[:, c], 0.75))) for c in range(2)]
    colors = [(1.0, 0.0, 1.0), (0.0, 0.5, 0.25)]
    got = rr.roishow(roi, layout, level, limits, colors, fg, bg, overlay, 0.7)
    want = loop_roishow(roi, layout, level, limits, colors, fg, bg, overlay, 0.7)
    np.testing.assert_array_equal(got, want)
    lk = math.ceil(7 / (1 << level))
    assert got.shape == (2, 2 * lk, 2 * lk, 3) and not got[:, lk:, :lk].any()  # the empty cell
    plain = rr.roishow(roi, layout, level, limits, colors)
    if overlay == "none":
        np.testing.assert_array_equal(got, rr.roishow(roi, layout, level, limits, colors, None, None, "fill"))
    else:
        assert (got != rr.roishow(roi, layout, level, limits, colors, fg, bg, "none")).any()
        assert plain.shape == got.shape
    only_fg = rr.roishow(roi, layout, level, limits, colors, fg, None, overlay, 0.7)  # a dataset without bg
    np.testing.assert_array_equal(only_fg, loop_roishow(roi, layout, level, limits, colors, fg, None, overlay, 0.7))


def test_fg_goes_on_top_of_bg():
    roi = np.zeros((1, 1, 1, 4, 4), dtype=np.uint8)
    fg = np.zeros((1, 1, 4, 4), dtype=bool)
    bg = np.ones((1, 1, 4, 4), dtype=bool)
    fg[0, 0, 1:3, 1:3] = True
    got = rr.roishow(roi, np.zeros((1, 1), np.int32), 0, [(0.0, 1.0)], [(1.0, 1.0, 1.0)], fg, bg, "fill", 1.0)
    assert (got[0, 1:3, 1:3] == (0, 255, 0)).all() and (got[0, 0] == (255, 0, 0)).all()
    rim = rr.roishow(roi, np.zeros((1, 1), np.int32), 0, [(0.0, 1.0)], [(1.0, 1.0, 1.0)], fg, bg, "outline", 0.3)
    assert (rim[0, 0] == (255, 0, 0)).all() and (rim[0, 1, 1] == (0, 255, 0)).all()  # the cell's border counts as off
    big = np.ones((1, 1, 8, 8), dtype=bool)
    inner = rr.roishow(np.zeros((1, 1, 1, 8, 8), np.uint8), np.zeros((1, 1), np.int32), 0, [(0.0, 1.0)],
                       [(1.0, 1.0, 1.0)], None, big, "outline", 0.3)
    assert not inner[0, 1:-1, 1:-1].any() and inner[0, 0].all(axis=0)[0]


# ---- the layout -----------------------------------------------------------------------------------------------------


def reference_grouping(tags):
    """plot/image.py:16-23 written out: which mark lands in cell (row, column)."""
    names, counts = np.unique(tags, return_counts=True)
    grid = np.full((counts.max(), len(names)), -1, dtype=np.int32)
    for i, name in enumerate(names):  # groupby("tag") walks the sorted tags; a group keeps mark order
        group = np.nonzero(tags == name)[0]
        grid[:len(group), i] = group
    return grid, names


def test_layout_is_the_references_grouping():
    tags = np.array(["b", "a", "b", "", "b"])
    grid, names = reference_grouping(tags)
    assert names.tolist() == ["", "a", "b"]
    got = plot.montage_layout(tags, 5)
    assert got.dtype == np.int32 and got.shape == (3, 3)
    np.testing.assert_array_equal(got, grid)
    np.testing.assert_array_equal(got, [[3, 1, 0], [-1, -1, 2], [-1, -1, 4]])
    np.testing.assert_array_equal(got, rr.montage_layout(tags, 5))
    rng = np.random.default_rng(3)
    for m in (1, 2, 17, 96):
        tags = rng.choice(np.array(["x", "yy", "", "z0", "z1"]), size=m)
        got = plot.montage_layout(tags, m)
        np.testing.assert_array_equal(got, reference_grouping(tags)[0])
        np.testing.assert_array_equal(got, rr.montage_layout(tags, m))
        assert sorted(got[got >= 0].tolist()) == list(range(m))
        for col in got.T:  # ascending marks from the top, then only -1
            k = int((col >= 0).sum())
            assert (np.diff(col[:k]) > 0).all() and (col[k:] == -1).all()


def test_layout_of_a_chips_tags():
    tags = np.array([["p1", "", "p2"], ["", "p1", "p1"]])  # (mark_row, mark_col), stacked row-major
    got = plot.montage_layout(tags.reshape(-1), 6)
    np.testing.assert_array_equal(got, [[1, 0, 2], [3, 4, -1], [-1, 5, -1]])
    np.testing.assert_array_equal(got, reference_grouping(tags.reshape(-1))[0])


def test_untagged_grid_and_no_marks():
    np.testing.assert_array_equal(plot.montage_layout(None, 5), [[0, 1, 2], [3, 4, -1]])  # ceil(sqrt(5)) = 3
    np.testing.assert_array_equal(plot.montage_layout(None, 5, 2), [[0, 1], [2, 3], [4, -1]])
    np.testing.assert_array_equal(plot.montage_layout(None, 4), [[0, 1], [2, 3]])
    np.testing.assert_array_equal(plot.montage_layout(None, 3, 7), [[0, 1, 2, -1, -1, -1, -1]])
    for m in (1, 2, 9, 10, 2000):
        got = plot.montage_layout(None, m)
        assert got.shape[1] == math.ceil(math.sqrt(m)) and got.shape[0] == math.ceil(m / got.shape[1])
        np.testing.assert_array_equal(got, rr.montage_layout(None, m))
    for tags in (None, np.array([], dtype=str)):
        got = plot.montage_layout(tags, 0)
        assert got.shape == (0, 0) and got.dtype == np.int32
    for columns in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            plot.montage_layout(None, 5, columns)
    with pytest.raises(ValueError):
        plot.montage_layout(np.array(["a"]), 2)
    assert plot.montage_level(3, 3, 40) == 0 and plot.montage_level(45, 45, 100) == 3
    assert plot.montage_level(45, 45, 100) == rr.default_level(45, 45, 100)
    assert plot.montage_level(10 ** 4, 10 ** 4, 100) == 6


# ---- the rank ------------------------------------------------------------------------------------------------------


def test_percentile_rank():
    assert plot.percentile_rank(1, 0) == plot.percentile_rank(1, 50) == plot.percentile_rank(1, 100) == 0
    for n in (2, 7, 1000, 2 ** 31 + 3):
        assert plot.percentile_rank(n, 0) == 0 and plot.percentile_rank(n, 100) == n - 1
    n = 2 ** 33 + 5
    assert plot.percentile_rank(n, 99.8) == (n - 1) * 99800 // 100000 == 8572754726
    assert plot.percentile_rank(n, 99.999) == 8589848696 and isinstance(plot.percentile_rank(n, 99.999), int)
    assert plot.percentile_rank(n, 50) == 2 ** 32 + 2
    assert plot.percentile_rank(np.int64(n), np.float32(50)) == 2 ** 32 + 2
    for q in (-0.001, 100.001, float("nan")):
        with pytest.raises(ValueError):
            plot.percentile_rank(10, q)
    with pytest.raises(ValueError):
        plot.percentile_rank(0, 50)
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(400):
        n = int(rng.integers(1, 3000))
        q = round(float(rng.random()) * 100, 3)
        pos = q * (n - 1) / 100
        if abs(pos - round(pos)) <= 1e-6:
            continue
        v = rng.normal(size=n).astype(np.float32)
        k = plot.percentile_rank(n, q)
        assert k == rr.percentile_rank(n, q)
        assert np.sort(v)[k] == np.percentile(v, q, method="lower") == rr.percentile(v, q)
        checked += 1
    assert checked > 300


def test_the_oracles_percentile():
    v = np.array([3.0, np.nan, -np.inf, 1.0, np.inf, 2.0], dtype=np.float32)
    assert rr.percentile(v, 0) == -np.inf and rr.percentile(v, 100) == np.inf and rr.percentile(v, 50) == 2.0
    d = np.array([1.0, 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -23, 16777217.0])  # float64 through float32
    assert rr.percentile(d, 34) == 1.0 and rr.percentile(d, 67) == np.float32(1.0 + 2.0 ** -23)
    assert rr.percentile(d, 100) == 16777216.0 and rr.percentile(d, 100).dtype == np.float64
    with pytest.raises(ValueError):
        rr.percentile(np.full(4, np.nan), 50)
    u = np.array([[5, 1], [9, 9]], dtype=np.uint16)
    np.testing.assert_array_equal(rr.percentile_limits(u[None], 0, 100), [[1.0, 9.0]])


# ---- errors raised before the device is needed ------------------------------------------------------------------------


def test_argument_errors():
    import magnify_amd as mg

    roi = mg.DataArray(np.zeros((2, 1, 1, 4, 4), np.uint16), ("mark", "channel", "time", "roi_y", "roi_x"))
    xp = mg.Dataset({"roi": roi, "image": mg.DataArray(np.zeros((8, 8), np.uint16), ("im_y", "im_x"))})
    for kw in (dict(lo=-1), dict(hi=100.5), dict(lo=60, hi=40), dict(lo=float("nan")), dict(source="tile"), dict(source=None)):
        with pytest.raises(ValueError):
            plot.percentile_limits(xp, **kw)
    for kw in (dict(level=7), dict(level=-1), dict(level=1.0), dict(overlay="rim"), dict(alpha=1.01), dict(alpha=-0.5),
               dict(group_by="mark"), dict(columns=0), dict(columns=-2)):
        with pytest.raises(ValueError):
            plot.roishow(xp, **kw)
    no_roi = mg.Dataset({"image": mg.DataArray(np.zeros((8, 8), np.uint16), ("im_y", "im_x"))})
    with pytest.raises(AttributeError, match="Dataset must contain 'roi' data variable."):
        plot.roishow(no_roi)
    with pytest.raises(AttributeError, match="Dataset must contain 'roi' data variable."):
        plot.percentile_limits(no_roi, source="roi")
    with pytest.raises(AttributeError, match="Dataset must contain 'image' data variable."):
        plot.percentile_limits(mg.Dataset({"roi": roi}), source="image")


def test_the_binding_reads_the_new_entries_from_the_header():
    import ctypes

    p, i, l, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert nat.PROTOTYPES["mg_percentile_histogram"] == [p, i, i, l, i, l, l, i, i, i, p, i, p, p]
    assert nat.PROTOTYPES["mg_render_roi_montage"] == [p, i, l, l, l, i, i, i, i, i, p, i, i, p, p, p, l, l, p, l, l, i, d, p, p]
    lib = nat.lib()
    hist = np.zeros(256, dtype=np.uint64)
    pre = np.array([1, 1], dtype=np.uint32)

    def histogram(dtype=0, n0=0, s0=0, n1=1, s1=0, unit=4, shift=0, bits=8, pshift=0, prefixes=0, n_pre=0, dst=hist.ctypes.data):
        return lib.mg_percentile_histogram(0, dtype, n0, s0, n1, s1, unit, shift, bits, pshift, prefixes, n_pre, dst, 0)

    assert histogram() == 0 and histogram(dtype=1, shift=5, bits=11) == 0  # no units: legal, nothing launched
    for kw in (dict(dtype=4), dict(n0=-1), dict(n1=-1), dict(unit=-1), dict(s0=-1), dict(s1=-1), dict(bits=0), dict(bits=12),
               dict(shift=-1), dict(shift=1), dict(bits=7), dict(dtype=1, shift=6, bits=11), dict(dtype=2, shift=0, bits=10),
               dict(n_pre=5), dict(n_pre=-1), dict(dst=0), dict(n0=1),  # (data is null)
               dict(dtype=1, shift=0, bits=5, pshift=5, n_pre=1),  # no prefixes
               dict(dtype=1, shift=0, bits=5, pshift=6, prefixes=pre.ctypes.data, n_pre=1),
               dict(dtype=1, shift=0, bits=5, pshift=5, prefixes=pre.ctypes.data, n_pre=2),  # the same prefix twice
               dict(dtype=0, shift=0, bits=4, pshift=4, prefixes=np.array([16], np.uint32).ctypes.data, n_pre=1)):
        assert histogram(**kw) == -1, kw
    assert histogram(dtype=1, shift=0, bits=5, pshift=5, prefixes=pre.ctypes.data, n_pre=1) == 0
    assert not hist.any()
