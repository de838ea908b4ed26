"""``magnify_amd.plot`` on the device against its NumPy restatement (tests/plot_ref.py), bit for bit everywhere: the
composite (mg_render_overview) on planes that take every path of the kernel, the label map (mg_roi_image_labels), the
overlays, and ``plot.overview`` / ``plot.roi_to_image_labels`` on what the pipelines return."""
import numpy as np
import pytest

import plot_ref as pr
from synth import draw_beads, draw_chip

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
# one-pixel planes, blocks larger than the plane, odd widths (u8 / u16 rows start anywhere in a 16-byte vector), ragged
# last blocks both ways, several workgroups
PLANES = [(1, 1), (1, 19), (19, 1), (37, 53), (130, 71), (300, 517)]
COLORS = [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0)]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    magnify_amd.seed(2468)
    return magnify_amd


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


def pixels(rng, shape, dtype):
    if np.dtype(dtype).kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    return (rng.random(shape) * 1e4 - 3e3).astype(dtype)


def narrow_limits(image, level=0):
    """Per channel the 25 % and 75 % quantiles of its finite block means at ``level``: both clamps act."""
    lim = []
    for chan in image:
        means = np.concatenate([np.divide(*pr.block_sums(plane, level)).reshape(-1) for plane in chan])
        means = means[np.isfinite(means)]
        lo, hi = float(np.quantile(means, 0.25)), float(np.quantile(means, 0.75))
        lim.append((lo, hi if hi > lo else lo + 1.0))
    return lim


# ---- 1. the composite ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("level", [0, 1, 3])
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_composite_equals_the_restatement(mg, plane, level, dtype):
    from magnify_amd import hotpath

    rng = np.random.default_rng(1000 * plane[0] + 10 * plane[1] + level)
    image = pixels(rng, (2, 2) + plane, dtype)
    limits = narrow_limits(image, level)
    got = hotpath.render_overview(dev(image), level, limits, COLORS).cpu().numpy()
    want = pr.overview(image, level, limits, COLORS)
    assert got.shape == want.shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)
    if want[..., 0].size >= 16:
        assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("level", [0, 1, 3])
def test_a_channel_and_time_view_is_read_where_it_lies(mg, level, dtype):
    from magnify_amd import hotpath

    rng = np.random.default_rng(11)
    big = pixels(rng, (3, 5, 37, 53), dtype)
    d_big = dev(big)
    view = d_big[1:3, 0:5:2]  # channels 1, 2 and timepoints 0, 2, 4: planes that are not neighbours
    assert not view.is_contiguous() and view.data_ptr() != d_big.data_ptr()
    host = big[1:3, 0:5:2]
    limits = narrow_limits(host, level)
    got = hotpath.render_overview(view, level, limits, COLORS).cpu().numpy()
    np.testing.assert_array_equal(got, pr.overview(host, level, limits, COLORS))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_flat_limit_gives_nothing_of_that_channel(mg, dtype):
    from magnify_amd import hotpath

    rng = np.random.default_rng(12)
    image = pixels(rng, (2, 2, 37, 53), dtype)
    limits = [(float(image[0, 0, 3, 3]), float(image[0, 0, 3, 3])), narrow_limits(image)[1]]  # hi == lo
    for level in (0, 1, 3):
        got = hotpath.render_overview(dev(image), level, limits, COLORS).cpu().numpy()
        np.testing.assert_array_equal(got, pr.overview(image, level, limits, COLORS))
        assert not got[..., 0].any() and not got[..., 2].any() and got[..., 1].any()  # channel 0 is the magenta one


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_and_infinity_in_a_float_plane(mg, dtype):
    from magnify_amd import hotpath

    rng = np.random.default_rng(13)
    image = pixels(rng, (2, 2, 37, 53), dtype)
    image[0, 0, 5, 7], image[0, 0, 20, 40], image[0, 1, 9, 9] = np.nan, np.inf, -np.inf
    image[1, 1, 30, 16], image[1, 1, 30, 17] = np.inf, -np.inf  # one block at level 1: their sum is NaN
    limits = narrow_limits(image)
    for level in (0, 1, 3):
        got = hotpath.render_overview(dev(image), level, limits, COLORS).cpu().numpy()
        want = pr.overview(image, level, limits, COLORS)
        np.testing.assert_array_equal(got, want)
    level0 = pr.overview(image, 0, limits, COLORS)
    assert level0[0, 5, 7, 0] == 0 and level0[0, 20, 40, 0] == 255 and level0[1, 9, 9, 0] == 0


def test_three_channels_and_levels_up_to_six(mg):
    from magnify_amd import hotpath

    rng = np.random.default_rng(14)
    image = pixels(rng, (3, 1, 130, 71), np.uint16)
    limits, colors = narrow_limits(image), pr.default_colors(3)
    for level in (2, 4, 5, 6):
        got = hotpath.render_overview(dev(image), level, limits, colors).cpu().numpy()
        np.testing.assert_array_equal(got, pr.overview(image, level, limits, colors))


# ---- 2. the label map ----------------------------------------------------------------------------------------------------

H = W = 96


@pytest.fixture(scope="module")
def labelled():
    """The 96 x 96 scene with L = 40 (plot_ref.scene): host masks, origins and the label maps of levels 0 and 2."""
    x, y, fg = pr.scene()
    origin = pr.origins(x, y, fg.shape[-1], H, W)
    return x, y, fg, origin, {k: pr.image_labels(fg, origin, k, H, W) for k in (0, 2)}


@pytest.mark.parametrize("level", [0, 2])
def test_labels_of_masks_that_differ_per_timepoint(mg, labelled, level):
    from magnify_amd import hotpath

    _, _, fg, origin, want = labelled
    assert (fg[:, 0] != fg[:, 1]).any() and not fg[4].any()
    got = hotpath.image_labels(dev(fg), origin, level, H, W)
    assert got.dtype == __import__("torch").int32
    np.testing.assert_array_equal(got.cpu().numpy(), want[level])
    again = hotpath.image_labels(dev(fg), origin, level, H, W)  # the same bits on every call
    np.testing.assert_array_equal(again.cpu().numpy(), want[level])
    # the origins as a host array of another integer type, as a device tensor, and as a view of a wider table
    wide = np.zeros(origin.shape[:2] + (3,), dtype=np.int32)
    wide[..., :2] = origin
    for form in (origin.astype(np.int64), dev(origin.astype(np.int16)), dev(wide)[..., :2]):
        np.testing.assert_array_equal(hotpath.image_labels(dev(fg), form, level, H, W).cpu().numpy(), want[level])


@pytest.mark.parametrize("level", [0, 2])
def test_labels_of_the_stride_0_time_view(mg, labelled, level):
    from magnify_amd import hotpath

    _, _, fg, origin, _ = labelled
    m, _, L, _ = fg.shape
    view = dev(fg[:, 0])[:, None].expand(m, 3, L, L)  # what the untracked bead path returns
    assert view.stride(1) == 0
    origin3 = np.ascontiguousarray(np.repeat(origin[:, :1], 3, axis=1))
    origin3[:, 2] = origin[:, 1]  # the same masks at other places
    got = hotpath.image_labels(view, origin3, level, H, W).cpu().numpy()
    np.testing.assert_array_equal(got, pr.image_labels(np.repeat(fg[:, :1], 3, axis=1), origin3, level, H, W))
    assert (got[0] == got[1]).all() and (got[0] != got[2]).any()


def test_no_markers_is_legal(mg):
    import torch

    from magnify_amd import hotpath

    for level in (0, 2):
        got = hotpath.image_labels(torch.zeros((0, 2, 40, 40), dtype=torch.bool, device="cuda"),
                                   np.zeros((0, 2, 2), dtype=np.int32), level, H, W)
        assert tuple(got.shape) == (2, H >> level, W >> level) and not got.any()


# ---- 3. the overlays -----------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def overlay_scene(labelled):
    rng = np.random.default_rng(21)
    image = pixels(rng, (2, 2, H, W), np.uint16)
    valid = np.ones((5, 2), dtype=bool)
    valid[1, 1] = False  # one marker, at one timepoint only
    return image, narrow_limits(image), valid


@pytest.mark.parametrize("color_by", ["mark", "valid"])
@pytest.mark.parametrize("overlay", ["fill", "outline", "none"])
@pytest.mark.parametrize("level", [0, 2])
def test_overlays_equal_the_restatement(mg, labelled, overlay_scene, level, overlay, color_by):
    from magnify_amd import hotpath

    _, _, fg, origin, want_labels = labelled
    image, limits, valid = overlay_scene
    table = pr.color_table(5, 2, color_by, valid)
    labels = hotpath.image_labels(dev(fg), origin, level, H, W)
    got = hotpath.render_overview(dev(image), level, limits, COLORS, labels, dev(table), overlay, 0.7).cpu().numpy()
    want = pr.overview(image, level, limits, COLORS, want_labels[level], table, overlay, 0.7)
    np.testing.assert_array_equal(got, want)
    plain = pr.overview(image, level, limits, COLORS)
    if overlay == "none":
        np.testing.assert_array_equal(got, plain)
    else:
        changed = (got != plain).any(axis=-1)
        assert changed.any() and not changed[want_labels[level] == 0].any()
        if overlay == "outline":
            assert (~changed[want_labels[level] > 0]).any()  # the inside of a mask is left alone
    if color_by == "valid" and overlay == "outline":
        rim = changed & (want_labels[level] == 2)
        assert (got[0][rim[0]] == (0, 255, 0)).all() and (got[1][rim[1]] == (255, 0, 0)).all()


# ---- 4. through the API --------------------------------------------------------------------------------------------------


def host_parts(xp):
    """(image (C, T, H, W), fg (M, T, L, L), x, y, valid (M, T)) on the host of a dataset before or after
    restore_format, marks stacked row-major."""
    v = xp.data_vars["image"]
    for d in ("time", "channel"):
        if d not in v.dims:
            v = v.expand_dims(d)
    image = v.transpose("channel", "time", "im_y", "im_x").values
    n_t = image.shape[1]

    def marks(name, tail):
        v = xp.coords[name]
        lead = ("mark",) if "mark" in v.dims else ("mark_row", "mark_col")
        has_time = "time" in v.dims
        a = v.transpose(*lead, "time", *tail).values
        a = a.reshape((-1,) + a.shape[len(lead):])
        if not has_time:
            a = a[:, None]
        return np.broadcast_to(a, (a.shape[0], n_t) + a.shape[2:])

    return image, marks("fg", ("roi_y", "roi_x")), marks("x", ()), marks("y", ()), marks("valid", ())


def want_overview(xp, level, overlay, color_by="mark", alpha=0.7):
    image, fg, x, y, valid = host_parts(xp)
    h, w = image.shape[2:]
    limits = [(float(image[c].min()), float(image[c].max())) for c in range(image.shape[0])]
    origin = pr.origins(x, y, fg.shape[-1], h, w)
    labels = pr.image_labels(fg, origin, level, h, w)
    table = pr.color_table(len(fg), image.shape[1], color_by, valid)
    return pr.overview(image, level, limits, pr.default_colors(image.shape[0]), labels, table, overlay, alpha), labels


BEADS = np.array([[60, 60], [60, 190], [128, 128], [190, 70], [185, 185]])
BEAD_KW = dict(min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=10000)


def test_beads_overview(mg):
    data = mg.DataArray(data=draw_beads((256, 256), BEADS), dims=("y", "x"))
    xp = mg.beads(data=data, **BEAD_KW)
    assert xp.sizes["mark"] == 5
    rgb = mg.plot.overview(xp, level=0, overlay="fill")
    assert rgb.dims == ("time", "y", "x", "rgb") and rgb.dtype == np.uint8 and rgb.data.is_cuda
    want, labels = want_overview(xp, 0, "fill")
    np.testing.assert_array_equal(rgb.values, want)
    np.testing.assert_array_equal(mg.plot.roi_to_image_labels(xp).values, labels)
    got = rgb.values[0]
    for cx, cy in zip(xp.x.values.reshape(-1), xp.y.values.reshape(-1)):
        r, g, b = got[int(cy), int(cx)]
        assert not r == g == b  # the pixel at every found bead's centre is not grey
    assert (got[0, 0] == got[0, 0, 0]).all()  # (the background is)
    for overlay in ("outline", None):
        np.testing.assert_array_equal(mg.plot.overview(xp, level=1, overlay=overlay).values, want_overview(xp, 1, overlay)[0])
    assert mg.plot.overview(xp).attrs["level"] == 0  # 256 x 256: the default level


def test_tracked_beads_overview_follows_the_beads(mg):
    planes = np.stack([draw_beads((256, 256), BEADS + 3 * t) for t in range(3)])
    data = mg.DataArray(data=planes, dims=("time", "y", "x"))
    xp = mg.beads(data=data, track="ncc", max_drift=8, **BEAD_KW)
    assert xp.sizes["mark"] == 5 and xp.valid.values.all()
    rgb = mg.plot.overview(xp, level=0, overlay="fill").values
    want, labels = want_overview(xp, 0, "fill")
    np.testing.assert_array_equal(rgb, want)
    got = mg.plot.roi_to_image_labels(xp).values
    np.testing.assert_array_equal(got, labels)
    order = np.argmin(np.linalg.norm(np.stack([xp.y.values[:, 0], xp.x.values[:, 0]], axis=1)[:, None] - BEADS[None], axis=2),
                      axis=1)
    for i in range(5):  # timepoint 2's overlay sits on timepoint 2's positions
        centre = np.argwhere(got[2] == i + 1).mean(axis=0)
        assert np.abs(centre - (BEADS[order[i]] + 6)).max() <= 1.5 and np.abs(centre - BEADS[order[i]]).max() > 4
        cy, cx = BEADS[order[i]] + 6
        r, g, b = rgb[2, cy, cx]
        assert not r == g == b
    np.testing.assert_array_equal(mg.plot.overview(xp, level=0, overlay="outline", color_by="valid").values,
                                  want_overview(xp, 0, "outline", "valid")[0])


CHIP_KW = dict(shape=(3, 3), min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100, col_dist=100,
               num_iter=5000)


@pytest.mark.parametrize("restore", [False, True], ids=["before_restore_format", "after_restore_format"])
def test_chip_overview(mg, restore):
    data = mg.DataArray(data=draw_chip((3, 3), 20), dims=("y", "x"))
    mg.seed(77)
    if restore:
        xp = mg.microfluidic_chip(data=data, **CHIP_KW)
        assert "mark_row" in xp.dims and "mark" not in xp.dims
    else:
        pipe = mg.microfluidic_chip_pipe(**CHIP_KW)
        pipe.remove_pipe("restore_format")
        xp = pipe(data)
        assert xp.sizes["mark"] == 9
    for level, overlay in ((0, "fill"), (1, "outline")):
        rgb = mg.plot.overview(xp, level=level, overlay=overlay).values
        want, labels = want_overview(xp, level, overlay)
        np.testing.assert_array_equal(rgb, want)
        np.testing.assert_array_equal(mg.plot.roi_to_image_labels(xp, level=level).values, labels)
        assert set(np.unique(labels).tolist()) == set(range(10))  # all nine buttons, in stacked mark order
    assert labels[0, 100 >> 1, 100 >> 1] == 1 and labels[0, 300 >> 1, 200 >> 1] == 8


def test_an_image_without_rois_gets_no_overlay(mg):
    rng = np.random.default_rng(31)
    tiles = pixels(rng, (2, 130, 71), np.uint16)
    xp = mg.image(data=mg.DataArray(data=tiles, dims=("channel", "y", "x"), coords={"channel": ["a", "b"]}), overlap=0)
    assert "roi" not in xp
    rgb = mg.plot.overview(xp)
    image = tiles[:, None]
    limits = [(float(image[c].min()), float(image[c].max())) for c in range(2)]
    np.testing.assert_array_equal(rgb.values, pr.overview(image, 0, limits, COLORS))
    lim, cols = [(100.0, 50000.0), (2000.0, 2000.0)], [(1.0, 0.5, 0.0), (0.25, 0.25, 1.0)]
    got = mg.plot.overview(xp, level=2, contrast_limits=lim, colors=cols).values
    np.testing.assert_array_equal(got, pr.overview(image, 2, lim, cols))
    host = mg.Dataset({"image": mg.DataArray(tiles[0], ("im_y", "im_x"))})  # an image on the host, no channel, no time
    np.testing.assert_array_equal(mg.plot.overview(host, level=1).values,
                                  pr.overview(image[:1], 1, limits[:1], [(1.0, 1.0, 1.0)]))
    with pytest.raises(AttributeError):
        mg.plot.roi_to_image_labels(xp)


def test_errors(mg):
    import torch

    from magnify_amd import _native as nat

    xp = mg.image(data=mg.DataArray(data=np.arange(64 * 64, dtype=np.uint16).reshape(64, 64), dims=("y", "x")), overlap=0)
    for kw in (dict(level=7), dict(level=-1), dict(overlay="rim"), dict(color_by="tag"), dict(alpha=1.01), dict(alpha=-0.5),
               dict(contrast_limits=[(0, 1), (0, 1)]), dict(contrast_limits=[0, 1]), dict(colors=[(1, 1, 1), (1, 0, 0)]),
               dict(colors=[(1, 1)]), dict(colors=[(2.0, 0, 0)])):
        with pytest.raises(ValueError):
            mg.plot.overview(xp, **kw)
    with pytest.raises(AttributeError, match="Dataset must contain 'image' data variable."):
        mg.plot.overview(mg.Dataset({"tile": mg.DataArray(np.zeros((4, 4), np.uint8), ("tile_y", "tile_x"))}))
    bad = mg.Dataset({"image": mg.DataArray(np.full((8, 8), np.nan, dtype=np.float32), ("im_y", "im_x"))})
    with pytest.raises(ValueError, match="not finite"):
        mg.plot.overview(bad)
    # the entry points refuse what is outside the contract and write nothing
    image = torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 8, 8, 3), 77, dtype=torch.uint8, device="cuda")
    lim, col = np.array([[0.0, 1.0]]), np.array([[1.0, 1.0, 1.0]])
    lab = torch.full((1, 8, 8), 5, dtype=torch.int32, device="cuda")
    tab = torch.zeros((1, 1, 3), dtype=torch.uint8, device="cuda")

    def render(dtype=0, n_c=1, n_t=1, h=8, w=8, level=0, limits=lim, colors=col, labels=0, table=0, n_marks=0, overlay=0,
               alpha=0.5, cs=64, ts=64, img=image.data_ptr(), dst=out.data_ptr()):
        return nat.lib().mg_render_overview(img, dtype, cs, ts, n_c, n_t, h, w, level, limits.ctypes.data, colors.ctypes.data,
                                            labels, table, n_marks, overlay, alpha, dst, 0)

    for kw in (dict(dtype=4), dict(n_c=0), dict(n_c=17), dict(n_t=0), dict(h=0), dict(w=0), dict(level=7), dict(level=-1),
               dict(overlay=3), dict(alpha=1.5), dict(alpha=float("nan")), dict(cs=-1), dict(ts=-1), dict(img=0), dict(dst=0),
               dict(colors=np.array([[1.5, 0.0, 0.0]])), dict(colors=np.array([[np.nan, 0.0, 0.0]])),
               dict(overlay=1), dict(overlay=2, labels=lab.data_ptr()), dict(overlay=2, labels=lab.data_ptr(), table=tab.data_ptr())):
        assert render(**kw) == -1, kw

    def label(m=1, n_t=1, L=4, level=0, h=8, w=8, fg=tab.data_ptr(), origin=lab.data_ptr(), dst=lab.data_ptr(), sm=16, st=0):
        return nat.lib().mg_roi_image_labels(fg, sm, st, origin, m, n_t, L, level, h, w, dst, 0)

    for kw in (dict(m=-1), dict(n_t=0), dict(L=0), dict(level=7), dict(h=0), dict(w=0), dict(fg=0), dict(origin=0), dict(dst=0),
               dict(sm=-1), dict(st=-1)):
        assert label(**kw) == -1, kw
    assert label(m=0, fg=0, origin=0) == 0
    torch.cuda.synchronize()
    assert (out == 77).all() and (lab == 5).all()
