"""``magnify_amd.plot`` without a GPU: the NumPy restatement (tests/plot_ref.py) against plain loops and against the
reference's own label loop written out as the reference writes it (plot/image.py:160-166); the PNG writer; the default
level; the host side of plot.py (window origins, defaults, the binding).

tests/test_gpu_plot.py holds the kernels to the same restatement bit for bit."""
import ctypes
import zlib

import numpy as np
import pytest

import plot_ref as pr


scene = pr.scene


def reference_labels(fg, tblr, shape):
    """plot/image.py:157-168, written out as the reference writes it."""
    img_labels = np.zeros((fg.shape[1],) + shape, dtype=np.int32)
    for i in range(fg.shape[0]):
        for j in range(fg.shape[1]):
            mask = fg[i, j]
            top, bottom, left, right = tblr[i, j]
            img_labels[j, top:bottom, left:right] = (i + 1) * mask + img_labels[j, top:bottom, left:right] * (1 - mask)
    return img_labels


def test_level0_labels_are_the_references_overwrite():
    h = w = 96
    x, y, fg = scene()
    L = fg.shape[-1]
    xs, ys = x.astype(int), y.astype(int)
    tblr = np.array([[pr.bounding_box(xs[i, t], ys[i, t], L, w, h) for t in range(fg.shape[1])] for i in range(len(fg))])
    origin = pr.origins(x, y, L, h, w)
    np.testing.assert_array_equal(origin, tblr[..., [0, 2]])
    assert (tblr[0, 0, [0, 2]] == 0).all() and tblr[3, 0, 3] == w  # pushed back at the corner and at the edge
    assert (tblr[..., 1] - tblr[..., 0] == L).all() and (tblr[..., 3] - tblr[..., 2] == L).all()
    got = pr.image_labels(fg, origin, 0, h, w)
    want = reference_labels(fg, tblr, (h, w))
    np.testing.assert_array_equal(got, want)
    assert ((got == 2).any() and (got == 3).any() and not (got == 5).any())
    both = np.zeros((h, w), dtype=int)  # the overlap of markers 1 and 2 went to the larger index
    for i in (1, 2):
        t, _, l, _ = tblr[i, 0]
        both[t:t + L, l:l + L] += fg[i, 0]
    t, _, l, _ = tblr[3, 0]
    both[t:t + L, l:l + L][fg[3, 0]] = 0  # (marker 3's speckles reach into that overlap: they win there)
    assert (both == 2).any() and (got[0][both == 2] == 3).all()
    assert (got[0] != got[1]).any()


@pytest.mark.parametrize("level", [1, 2, 3])
def test_level_k_labels_are_the_block_maximum(level):
    h, w = 96, 90  # (90: a ragged last block)
    x, y, fg = scene(1)
    x = np.minimum(x, w - 1)
    origin = pr.origins(x, y, fg.shape[-1], h, w)
    full = pr.image_labels(fg, origin, 0, h, w)
    s = 1 << level
    hk, wk = -(h // -s), -(w // -s)
    pad = np.zeros((full.shape[0], hk * s, wk * s), dtype=np.int32)
    pad[:, :h, :w] = full
    want = pad.reshape(-1, hk, s, wk, s).max(axis=(2, 4))
    np.testing.assert_array_equal(pr.image_labels(fg, origin, level, h, w), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("shape,level", [((1, 1), 3), ((19, 1), 1), ((37, 53), 0), ((37, 53), 1), ((37, 53), 3)])
def test_block_means_equal_a_plain_double_loop(dtype, shape, level):
    rng = np.random.default_rng(5)
    h, w = shape
    plane = (rng.integers(0, 256 if dtype == np.uint8 else 60000, size=shape).astype(dtype) if np.dtype(dtype).kind == "u"
             else (rng.random(shape) * 1e4 - 3e3).astype(dtype))
    total, n = pr.block_sums(plane, level)
    s = 1 << level
    for Y in range(-(h // -s)):
        for X in range(-(w // -s)):
            acc, cnt = 0.0, 0
            for r in range(Y * s, min(Y * s + s, h)):
                for k in range(X * s, min(X * s + s, w)):
                    acc, cnt = acc + float(plane[r, k]), cnt + 1
            assert total[Y, X] == acc and n[Y, X] == cnt
            assert total[Y, X] / n[Y, X] == acc / cnt


def test_composite_of_one_pixel_by_hand():
    image = np.array([[[[10.0, 30.0], [50.0, 70.0]]], [[[0.0, 4.0], [np.nan, np.inf]]]])  # (2, 1, 2, 2)
    out = pr.overview(image, 0, [(20.0, 60.0), (0.0, 8.0)], [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0)])
    #           below lo -> 0       0.25                0.75               above hi -> 1
    np.testing.assert_array_equal(out[0, :, :, 0], [[0, int(255 * 0.25 + 0.5)], [int(255 * 0.75 + 0.5), 255]])
    np.testing.assert_array_equal(out[0, :, :, 1], [[0, 128], [0, 255]])  # 0, 0.5, NaN -> 0, inf -> 1
    flat = pr.overview(image, 0, [(20.0, 20.0), (0.0, 8.0)], [(1.0, 1.0, 1.0), (0.0, 0.0, 0.0)])
    assert not flat.any()  # hi == lo: nothing of that channel
    mean = pr.overview(image[:1], 1, [(0.0, 80.0)], [(1.0, 1.0, 1.0)])
    assert mean.shape == (1, 1, 1, 3) and (mean == int(255 * 0.5 + 0.5)).all()  # (10 + 30 + 50 + 70) / 4 = 40
    lab = np.array([[[1, 0], [0, 0]]], dtype=np.int32)
    tab = pr.color_table(1, 1)
    filled = pr.overview(image, 0, [(20.0, 60.0), (0.0, 8.0)], [(1, 0, 1), (0, 1, 0)], lab, tab, "fill", 0.5)
    np.testing.assert_array_equal(filled[0, 0, 0], np.floor(255 * (0.5 * tab[0, 0] / 255.0) + 0.5).astype(np.uint8))
    np.testing.assert_array_equal(filled[0, 1:], out[0, 1:])
    outline = pr.overview(image, 0, [(20.0, 60.0), (0.0, 8.0)], [(1, 0, 1), (0, 1, 0)], lab, tab, "outline")
    np.testing.assert_array_equal(outline[0, 0, 0], tab[0, 0])


def test_outline_marks_the_rim_only():
    lab = np.zeros((1, 9, 9), dtype=np.int32)
    lab[0, 2:7, 2:7] = 1
    lab[0, 0:2, 7:9] = 2  # at the picture's corner: outside counts as 0, so all of it is rim
    tab = pr.color_table(2, 1)
    image = np.zeros((1, 1, 9, 9), dtype=np.uint8)
    out = pr.overview(image, 0, [(0.0, 1.0)], [(1.0, 1.0, 1.0)], lab, tab, "outline")
    painted = out[0].any(axis=-1)
    want = np.zeros((9, 9), dtype=bool)
    want[2:7, 2:7] = True
    want[3:6, 3:6] = False
    want[0:2, 7:9] = True
    np.testing.assert_array_equal(painted, want)
    valid = np.array([[True], [False]])
    tab = pr.color_table(2, 1, "valid", valid)
    np.testing.assert_array_equal(tab[:, 0], [[0, 255, 0], [255, 0, 0]])


def test_write_png_round_trip(tmp_path):
    from magnify_amd import plot

    rng = np.random.default_rng(2)
    for shape in [(1, 1, 3), (7, 5, 3), (64, 131, 3)]:
        rgb = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = tmp_path / f"p{shape[1]}.png"
        plot.write_png(str(path), rgb)
        data = path.read_bytes()
        np.testing.assert_array_equal(pr.decode_png(data), rgb)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(str(path)) as im:
            assert im.mode == "RGB"
            np.testing.assert_array_equal(np.asarray(im), rgb)
    assert zlib.crc32(b"IEND") & 0xFFFFFFFF == int.from_bytes(data[-4:], "big")
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            plot.write_png(str(tmp_path / "bad.png"), bad)


def test_default_level():
    from magnify_amd import plot

    for fn in (pr.default_level, plot.default_level):
        assert fn(1024, 1024) == 0 and fn(4096, 4096) == 2 and fn(70000, 70000) == 6
        assert fn(1025, 1024) == 1 and fn(1, 1) == 0 and fn(2048, 512) == 0


def test_host_side_matches_the_restatement():
    from magnify_amd import plot, utils

    rng = np.random.default_rng(3)
    for L, h, w in [(40, 96, 96), (41, 50, 120), (72, 72, 300)]:
        x, y = rng.integers(0, w, size=(30, 2)), rng.integers(0, h, size=(30, 2))
        got = np.stack([utils.window_origin(y, L, h), utils.window_origin(x, L, w)], axis=-1)
        np.testing.assert_array_equal(got, pr.origins(x, y, L, h, w))
        for i in range(30):
            top, bottom, left, right = utils.bounding_box(int(x[i, 0]), int(y[i, 0]), L, w, h)
            assert (got[i, 0] == (top, left)).all() and bottom - top == L and right - left == L
    for n in (1, 2, 3, 7):
        assert plot.default_colors(n) == pr.default_colors(n)
    np.testing.assert_array_equal(np.asarray(plot.MARK_COLORS, dtype=np.uint8), pr.MARK_COLORS)
    assert plot.default_colors(1) == [(1.0, 1.0, 1.0)] and plot.default_colors(2) == [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0)]


def test_public_names_and_binding():
    import magnify_amd as mg
    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    assert "plot" in mg.__all__ and mg.plot.overview and mg.plot.roi_to_image_labels and mg.plot.write_png
    a = nat.PROTOTYPES["mg_roi_image_labels"]
    assert len(a) == 12 and a[1] is ctypes.c_int64 and a[2] is ctypes.c_int64
    b = nat.PROTOTYPES["mg_render_overview"]
    assert len(b) == 18 and b[2] is ctypes.c_int64 and b[3] is ctypes.c_int64 and b[15] is ctypes.c_double
    for name in ("mg_roi_image_labels", "mg_render_overview"):
        assert nat.RESTYPES[name] is ctypes.c_int and hasattr(nat.lib(), name)
    # (read from the header: its values)
    assert (hotpath.OVERVIEW_MAX_LEVEL, hotpath.OVERVIEW_MAX_CHANNELS, hotpath.PERCENTILE_MAX_PREFIXES) == (6, 16, 4)
    assert mg.plot.MAX_LEVEL == 6 and (nat.MG_U8, nat.MG_U16, nat.MG_F32, nat.MG_F64) == (0, 1, 2, 3)
    assert (nat.MG_NO_EDGE, nat.MG_SCORE_SKIPPED) == (100.0, -2.0)


def test_argument_errors_need_no_gpu():
    import magnify_amd as mg

    ds = mg.Dataset({"image": mg.DataArray(np.zeros((4, 4), np.uint8), ("im_y", "im_x"))})
    for kw in (dict(level=7), dict(level=-1), dict(level=1.5), dict(overlay="rim"), dict(color_by="tag"), dict(alpha=1.5),
               dict(alpha=-0.1)):
        with pytest.raises(ValueError):
            mg.plot.overview(ds, **kw)
    with pytest.raises(AttributeError, match="must contain 'image'"):
        mg.plot.overview(mg.Dataset({"tile": mg.DataArray(np.zeros((4, 4), np.uint8), ("tile_y", "tile_x"))}))
    with pytest.raises(ValueError):
        mg.plot.roi_to_image_labels(ds, level=9)
