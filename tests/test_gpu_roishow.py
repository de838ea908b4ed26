"""``plot.roishow`` on the device against its NumPy restatement (tests/roishow_ref.py), bit for bit: the montage
(mg_render_roi_montage) on windows that take every load path of the kernel, the overlays from per-timepoint and from
shared masks, views that are read where they lie, and ``plot.roishow`` on what the pipelines return."""
import numpy as np
import pytest

import plot_ref as pr
import roishow_ref as rr
from synth import draw_beads, draw_chip

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
COLORS = [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0)]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    magnify_amd.seed(2469)
    return magnify_amd


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


def narrow_limits(roi, level=0):
    """Per channel the 25 % and 75 % quantiles of its finite block means at ``level``: both clamps act (as
    ``narrow_limits`` of tests/test_gpu_plot.py)."""
    lim = []
    for c in range(roi.shape[1]):
        means = np.concatenate([np.divide(*pr.block_sums(w, level)).reshape(-1) for w in roi[:, c].reshape((-1,) + roi.shape[3:])])
        means = means[np.isfinite(means)]
        lo, hi = float(np.quantile(means, 0.25)), float(np.quantile(means, 0.75))
        lim.append((lo, hi if hi > lo else lo + 1.0))
    return lim


SCENES = {}


def scene(dtype, L, per_time=True):
    """(roi, fg, bg, layout, limits per level) of the 5-mark scene, made once per (dtype, L)."""
    key = (np.dtype(dtype).name, L, per_time)
    if key not in SCENES:
        roi, fg, bg, tags = rr.scene(dtype, L, per_time=per_time)
        layout = rr.montage_layout(tags, 5)
        assert layout.shape == (3, 3) and (layout == -1).sum() == 4  # three columns of unequal length
        SCENES[key] = (roi, fg, bg, layout, {})
    return SCENES[key]


def limits_of(sc, level):
    if level not in sc[4]:
        sc[4][level] = narrow_limits(sc[0], level)
    return sc[4][level]


# ---- 1. the kernel --------------------------------------------------------------------------------------------------

CASES = [(L, level) for L in (1, 7, 40) for level in (0, 1, 3)] + [(100, 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("L,level", CASES, ids=lambda v: str(v))
def test_montage_equals_the_restatement(mg, L, level, dtype):
    from magnify_amd import hotpath

    sc = scene(dtype, L)
    roi, fg, bg, layout, _ = sc
    limits = limits_of(sc, level)
    d_roi, d_fg, d_bg = dev(roi), dev(fg), dev(bg)
    assert L < 7 or ((fg & bg).any() and not fg[3].any() and bg[4].all() and (fg[:, 0] != fg[:, 1]).any())
    for overlay in ("fill", "outline", "none"):
        got = hotpath.render_roi_montage(d_roi, layout, level, limits, COLORS, d_fg, d_bg, overlay, 0.7).cpu().numpy()
        want = rr.roishow(roi, layout, level, limits, COLORS, fg, bg, overlay, 0.7)
        assert got.shape == want.shape and got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
    lk = -(L // -(1 << level))
    assert got.shape == (2, 3 * lk, 3 * lk, 3) and not got[:, lk:, :2 * lk].any()  # the empty cells
    if L >= 40 and level == 0:
        assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()
        plain = rr.roishow(roi, layout, level, limits, COLORS)
        np.testing.assert_array_equal(got, plain)
        rim = rr.roishow(roi, layout, level, limits, COLORS, fg, bg, "outline", 0.7)
        fill = rr.roishow(roi, layout, level, limits, COLORS, fg, bg, "fill", 0.7)
        assert (rim != plain).any() and (fill != plain).any()
        assert ((fill != plain).any(-1) & (rim == plain).all(-1)).any()  # the inside of a mask is left alone


def test_a_u16_window_row_that_starts_off_vector_alignment(mg):
    """L = 100 at level 3: 13 blocks a side, the last one 4 wide; from an odd element on, no row is 16-byte aligned."""
    from magnify_amd import hotpath

    roi, fg, bg, layout, _ = scene(np.uint16, 100)
    limits = limits_of(scene(np.uint16, 100), 3)
    shifted = dev(np.concatenate([np.zeros(3, np.uint16), roi.reshape(-1)]))[3:].view(roi.shape)
    assert shifted.data_ptr() % 16 == 6
    got = hotpath.render_roi_montage(shifted, layout, 3, limits, COLORS, dev(fg), dev(bg), "fill", 0.7).cpu().numpy()
    np.testing.assert_array_equal(got, rr.roishow(roi, layout, 3, limits, COLORS, fg, bg, "fill", 0.7))
    for level in (4, 6):  # several vectors per row of a block; one block per window
        lim = limits_of(scene(np.uint16, 100), level)
        got = hotpath.render_roi_montage(shifted, layout, level, lim, COLORS, dev(fg), dev(bg), "outline", 0.7).cpu().numpy()
        np.testing.assert_array_equal(got, rr.roishow(roi, layout, level, lim, COLORS, fg, bg, "outline", 0.7))


@pytest.mark.parametrize("level", [0, 1])
def test_masks_shared_by_all_timepoints_are_a_stride_0_view(mg, level):
    from magnify_amd import hotpath

    sc = scene(np.uint16, 40, per_time=False)
    roi, fg, bg, layout, _ = sc
    assert (fg[:, 0] == fg[:, 1]).all() and (bg[:, 0] == bg[:, 1]).all()
    view_fg, view_bg = dev(fg[:, 0])[:, None].expand(5, 2, 40, 40), dev(bg[:, 0])[:, None].expand(5, 2, 40, 40)
    assert view_fg.stride(1) == 0
    limits = limits_of(sc, level)
    got = hotpath.render_roi_montage(dev(roi), layout, level, limits, COLORS, view_fg, view_bg, "fill", 0.4).cpu().numpy()
    np.testing.assert_array_equal(got, rr.roishow(roi, layout, level, limits, COLORS, fg, bg, "fill", 0.4))
    only_bg = hotpath.render_roi_montage(dev(roi), layout, level, limits, COLORS, None, view_bg, "fill", 0.4).cpu().numpy()
    np.testing.assert_array_equal(only_bg, rr.roishow(roi, layout, level, limits, COLORS, None, bg, "fill", 0.4))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_channel_subset_view_is_read_where_it_lies(mg, dtype):
    from magnify_amd import hotpath

    rng = np.random.default_rng(41)
    big = rr.scene(dtype, 7, seed=1)[0]
    big = np.concatenate([big, big[:, ::-1] // 2 if np.dtype(dtype).kind == "u" else big[:, ::-1] * 0.5], axis=1)  # 4 channels
    rng.shuffle(big, axis=3)
    _, fg, bg, layout, _ = scene(dtype, 7)
    d_big = dev(big)
    view = d_big[:, 1:4:2]  # channels 1 and 3: not contiguous over marks
    assert not view.is_contiguous() and view.data_ptr() != d_big.data_ptr()
    host = big[:, 1:4:2]
    limits = narrow_limits(host, 1)
    for level in (0, 1):
        got = hotpath.render_roi_montage(view, layout, level, limits, COLORS, dev(fg), dev(bg), "outline", 0.7).cpu().numpy()
        np.testing.assert_array_equal(got, rr.roishow(host, layout, level, limits, COLORS, fg, bg, "outline", 0.7))


def test_an_untagged_grid_and_no_marks(mg):
    import torch

    from magnify_amd import hotpath

    sc = scene(np.uint16, 7)
    roi, fg, bg, _, _ = sc
    layout = rr.montage_layout(None, 5, 2)
    assert layout.shape == (3, 2)
    limits = limits_of(sc, 0)
    got = hotpath.render_roi_montage(dev(roi), layout, 0, limits, COLORS, dev(fg), dev(bg), "fill", 0.7).cpu().numpy()
    np.testing.assert_array_equal(got, rr.roishow(roi, layout, 0, limits, COLORS, fg, bg, "fill", 0.7))
    assert not got[:, 14:, 7:].any()
    empty = hotpath.render_roi_montage(torch.zeros((0, 2, 2, 7, 7), dtype=torch.uint16, device="cuda"),
                                       np.zeros((0, 0), np.int32), 0, limits, COLORS)
    assert tuple(empty.shape) == (2, 0, 0, 3) and empty.dtype == torch.uint8


# ---- 2. through the API -----------------------------------------------------------------------------------------------


def host_roi(xp):
    """(roi (M, C, T, L, L), fg, bg (M, T, L, L)) on the host, marks stacked row-major."""
    v = xp.data_vars["roi"]
    lead = ("mark",) if "mark" in v.dims else ("mark_row", "mark_col")
    for d in ("time", "channel"):
        if d not in v.dims:
            v = v.expand_dims(d, len(lead))
    roi = v.transpose(*lead, "channel", "time", "roi_y", "roi_x").values
    roi = roi.reshape((-1,) + roi.shape[len(lead):])

    def mask(name):
        c = xp.coords[name]
        has_time = "time" in c.dims
        a = c.transpose(*lead, "time", "roi_y", "roi_x").values
        a = a.reshape((-1,) + a.shape[len(lead):])
        if not has_time:
            a = a[:, None]
        return np.broadcast_to(a, (a.shape[0], roi.shape[2]) + a.shape[2:])

    return roi, mask("fg"), mask("bg")


def want_roishow(xp, layout, level, overlay, limits=None, alpha=0.7):
    roi, fg, bg = host_roi(xp)
    if limits is None:
        limits = [(float(roi[:, c].min()), float(roi[:, c].max())) for c in range(roi.shape[1])]
    return rr.roishow(roi, layout, level, limits, pr.default_colors(roi.shape[1]), fg, bg, overlay, alpha)


BEADS = np.array([[60, 60], [60, 190], [128, 128], [190, 70], [185, 185]])
BEAD_KW = dict(min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=10000)


def test_beads_roishow(mg, tmp_path):
    a = draw_beads((256, 256), BEADS)
    b = draw_beads((256, 256), BEADS, value=3000) + np.uint16(50)
    data = mg.DataArray(data=np.stack([a, b]), dims=("channel", "y", "x"), coords={"channel": ["red", "green"]})
    xp = mg.beads(data=data, **BEAD_KW)
    m = xp.sizes["mark"]
    assert m >= 2 and "tag" not in xp.coords
    rgb = mg.plot.roishow(xp)
    assert rgb.dims == ("time", "y", "x", "rgb") and rgb.dtype == np.uint8 and rgb.data.is_cuda
    layout = rr.montage_layout(None, m)
    np.testing.assert_array_equal(rgb.attrs["marks"], layout)
    L = xp.roi.shape[-1]
    assert rgb.attrs["level"] == 0 and rgb.attrs["cell"] == L and rgb.attrs["tags"] is None
    np.testing.assert_array_equal(rgb.values, want_roishow(xp, layout, 0, "fill"))
    centre = rgb.values[0, L // 2, L // 2]
    assert centre[1] > centre[0]  # the fg mask, in green, sits on the bead
    two = rr.montage_layout(None, m, 2)
    for level, overlay in ((1, "outline"), (0, None)):
        got = mg.plot.roishow(xp, level=level, overlay=overlay, columns=2)
        np.testing.assert_array_equal(got.attrs["marks"], two)
        np.testing.assert_array_equal(got.values, want_roishow(xp, two, level, overlay))
    lim = mg.plot.percentile_limits(xp, 1, 99.8, source="roi")
    got = mg.plot.roishow(xp, contrast_limits=lim, colors=[(1.0, 0.5, 0.0), (0.25, 0.25, 1.0)], overlay="none").values
    roi = host_roi(xp)[0]
    np.testing.assert_array_equal(got, rr.roishow(roi, layout, 0, lim, [(1.0, 0.5, 0.0), (0.25, 0.25, 1.0)]))
    path = tmp_path / "t0.png"
    mg.plot.write_png(path, rgb[0].values)
    np.testing.assert_array_equal(pr.decode_png(path.read_bytes()), rgb.values[0])


CHIP_KW = dict(shape=(3, 3), min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100, col_dist=100,
               num_iter=5000)
PINS = np.array([["p1", "", "p2"], ["p2", "p1", "p1"], ["", "p1", "p3"]])


@pytest.mark.parametrize("restore", [False, True], ids=["before_restore_format", "after_restore_format"])
def test_chip_roishow(mg, restore, tmp_path):
    pinlist = tmp_path / "pins.csv"
    pinlist.write_text("Indices,MutantID\n" + "".join(f'"({c + 1}, {r + 1})",{PINS[r, c] or "blank"}\n'
                                                       for r in range(3) for c in range(3)))
    data = mg.DataArray(data=draw_chip((3, 3), 20), dims=("y", "x"))
    mg.seed(77)
    kw = dict(CHIP_KW, pinlist=str(pinlist))
    if restore:
        xp = mg.microfluidic_chip(data=data, **kw)
        assert "mark_row" in xp.dims and "mark" not in xp.dims
    else:
        pipe = mg.microfluidic_chip_pipe(**kw)
        pipe.remove_pipe("restore_format")
        xp = pipe(data)
    tags = np.asarray(xp.coords["tag"].values).reshape(-1)
    np.testing.assert_array_equal(tags, PINS.reshape(-1))
    layout = rr.montage_layout(tags, 9)
    np.testing.assert_array_equal(layout, [[1, 0, 2, 8], [6, 4, 3, -1], [-1, 5, -1, -1], [-1, 7, -1, -1]])
    for level, overlay in ((0, "fill"), (1, "outline")):
        rgb = mg.plot.roishow(xp, level=level, overlay=overlay)
        np.testing.assert_array_equal(rgb.attrs["marks"], layout)
        assert rgb.attrs["tags"].tolist() == ["", "p1", "p2", "p3"]
        np.testing.assert_array_equal(rgb.values, want_roishow(xp, layout, level, overlay))
    grid = mg.plot.roishow(xp, level=0, group_by=None)
    np.testing.assert_array_equal(grid.attrs["marks"], np.arange(9).reshape(3, 3))
    assert grid.attrs["tags"] is None
    np.testing.assert_array_equal(grid.values, want_roishow(xp, np.arange(9, dtype=np.int32).reshape(3, 3), 0, "fill"))


def test_a_roi_only_dataset_and_one_without_masks(mg):
    roi, fg, bg, tags = rr.scene(np.uint16, 7)
    dims = ("mark", "channel", "time", "roi_y", "roi_x")
    xp = mg.Dataset({"roi": mg.DataArray(dev(roi), dims)}, coords={"tag": (("mark",), tags)})
    layout = rr.montage_layout(tags, 5)
    limits = [(float(roi[:, c].min()), float(roi[:, c].max())) for c in range(2)]
    rgb = mg.plot.roishow(xp)  # no image, no fg / bg: no overlay; the limits come from the roi
    np.testing.assert_array_equal(rgb.values, rr.roishow(roi, layout, 0, limits, COLORS))
    assert rgb.attrs["tags"].tolist() == ["", "a", "b"]
    host = mg.Dataset({"roi": mg.DataArray(roi[:, 0, 0], ("mark", "roi_y", "roi_x"))})  # on the host, no channel, no time
    got = mg.plot.roishow(host, level=1)
    one = [(float(roi[:, 0, 0].min()), float(roi[:, 0, 0].max()))]
    np.testing.assert_array_equal(got.values, rr.roishow(roi[:, :1, :1], rr.montage_layout(None, 5), 1, one, [(1.0, 1.0, 1.0)]))
    none = mg.Dataset({"roi": mg.DataArray(dev(roi[:0]), dims)})
    empty = mg.plot.roishow(none)
    assert empty.shape == (2, 0, 0, 3) and empty.attrs["marks"].shape == (0, 0)


def test_errors(mg):
    import torch

    from magnify_amd import _native as nat

    roi, fg, bg, tags = rr.scene(np.uint16, 7)
    dims = ("mark", "channel", "time", "roi_y", "roi_x")
    xp = mg.Dataset({"roi": mg.DataArray(dev(roi), dims)})
    for kw in (dict(level=7), dict(level=-1), dict(overlay="rim"), dict(alpha=1.01), dict(alpha=-0.5), dict(group_by="row"),
               dict(columns=0), dict(contrast_limits=[(0, 1)]), dict(contrast_limits=[0, 1]), dict(colors=[(1, 1, 1)]),
               dict(colors=[(1, 1), (1, 1)]), dict(colors=[(2.0, 0, 0), (0, 0, 0)])):
        with pytest.raises(ValueError):
            mg.plot.roishow(xp, **kw)
    many = mg.Dataset({"roi": mg.DataArray(torch.zeros((1, 17, 1, 4, 4), dtype=torch.uint8, device="cuda"), dims)})
    with pytest.raises(ValueError, match="at most 16 channels"):
        mg.plot.roishow(many)
    with pytest.raises(AttributeError, match="Dataset must contain 'roi' data variable."):
        mg.plot.roishow(mg.Dataset({"image": mg.DataArray(np.zeros((4, 4), np.uint8), ("im_y", "im_x"))}))
    with pytest.raises(ValueError):
        mg.plot.percentile_limits(xp, 50, 40, source="roi")
    with pytest.raises(ValueError):
        mg.plot.percentile_limits(xp, source="fg")
    # the entry point refuses what is outside the contract and writes nothing
    d_roi = torch.zeros((1, 1, 1, 4, 4), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 4, 4, 3), 77, dtype=torch.uint8, device="cuda")
    lay = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    lim, col = np.array([[0.0, 1.0]]), np.array([[1.0, 1.0, 1.0]])

    def render(dtype=0, sm=16, sc=16, st=16, m=1, n_c=1, n_t=1, L=4, level=0, layout=lay.data_ptr(), rows=1, cols=1, limits=lim,
               colors=col, bg=0, bm=0, bt=0, fg=0, fm=0, ft=0, overlay=0, alpha=0.5, src=d_roi.data_ptr(), dst=out.data_ptr()):
        return nat.lib().mg_render_roi_montage(src, dtype, sm, sc, st, m, n_c, n_t, L, level, layout, rows, cols,
                                               limits.ctypes.data, colors.ctypes.data, bg, bm, bt, fg, fm, ft, overlay, alpha,
                                               dst, 0)

    for kw in (dict(dtype=4), dict(n_c=0), dict(n_c=17), dict(n_t=0), dict(L=0), dict(L=40000), dict(level=7), dict(level=-1),
               dict(overlay=3), dict(alpha=1.5), dict(alpha=float("nan")), dict(sm=-1), dict(sc=-1), dict(st=-1), dict(bm=-1),
               dict(ft=-1), dict(src=0), dict(dst=0), dict(layout=0), dict(m=0), dict(m=-1), dict(rows=-1), dict(cols=-1),
               dict(colors=np.array([[1.5, 0.0, 0.0]])), dict(colors=np.array([[np.nan, 0.0, 0.0]]))):
        assert render(**kw) == -1, kw
    assert render(rows=0, src=0, layout=0, dst=0, m=0) == 0  # no cells: legal, nothing launched
    torch.cuda.synchronize()
    assert (out == 77).all()
