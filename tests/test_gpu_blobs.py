"""Blobs on the device: mg_blob_labels / mg_blob_select / mg_blob_fill_holes through ``magnify_amd.blobs``, exactly equal
to the NumPy + scipy oracle (tests/blobs_ref.py) on random masks either side of both percolation points at every size
round the tile, on every dtype and polarity, on planes built to break the tile and seam passes (tests/blobs_cases.py), and
``find_blobs`` end to end through ``mg.blobs``.  No launch of the family is capped, so there is no walk to take twice."""
import numpy as np
import pytest
import torch

pytest.importorskip("scipy")

import blobs_cases as bc  # noqa: E402
import blobs_ref as br  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import magnify_amd

    magnify_amd.hotpath = __import__("magnify_amd.hotpath", fromlist=["x"])
    magnify_amd.hotpath.require_gpu()
    return magnify_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def check_label(mg, plane, threshold, below=False, connectivity=8, what=None, **kw):
    """label() of a host plane against the oracle: the map, the count and the statistics, exactly."""
    want_l, want_k, want_s = br.label(plane, threshold, below, connectivity)
    got = mg.blobs.label(dev(plane), threshold, below=below, connectivity=connectivity, **kw)
    tag = (what, plane.shape, str(plane.dtype), threshold, below, connectivity)
    assert got["count"] == want_k, tag
    assert got["labels"].dtype == torch.int32 and got["stats"].dtype == torch.int64 and got["stats"].shape == (want_k, 8), tag
    assert np.array_equal(host(got["labels"]), want_l), tag
    assert np.array_equal(host(got["stats"]), want_s), tag
    return got, (want_l, want_k, want_s)


def check_mask(mg, mask, connectivity, what=None, **kw):
    return check_label(mg, mask.astype(np.uint8), 0, False, connectivity, what, **kw)


def seam_shapes(mg):
    """(h, w) pairs in which every size round the tile occurs as a height and as a width, paired as
    test_gpu_background.py::seam_shapes pairs them, and one plane of several tiles both ways."""
    th, tw = mg.blobs.TILE_H, mg.blobs.TILE_W
    hs = sorted({1, 2, th - 1, th, th + 1, 2 * th + 1})
    ws = sorted({1, 31, 32, 33, tw - 1, tw, tw + 1, 2 * tw + 1, 3 * tw + 5}, reverse=True)
    pairs = [(h, ws[i % len(ws)]) for i, h in enumerate(hs)] + [(hs[i % len(hs)], w) for i, w in enumerate(ws)]
    pairs += [(h, ws[(i + len(ws) // 2) % len(ws)]) for i, h in enumerate(hs)]
    return sorted(set(pairs)) + [(2 * th + 1, 3 * tw + 5)]


def random_mask(shape=None, p=0.41, seed=7):
    return np.random.default_rng(seed).random(shape) < p


# ---- label -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("p", [0.05, 0.41, 0.59, 0.95])
def test_random_masks_at_every_size_round_the_tile(mg, p, connectivity):
    rng = np.random.default_rng(int(100 * p) + connectivity)
    for h, w in seam_shapes(mg):
        check_mask(mg, rng.random((h, w)) < p, connectivity, p)


@pytest.mark.parametrize("p", [0.41, 0.59])
def test_hundreds_of_tiles_at_the_percolation_points(mg, p):
    """22 x 15 tiles: components that run through hundreds of workgroups' tiles on every XCD, so that the seam pass's
    unions do meet each other; the same call three times gives the same bits."""
    mask = random_mask((22 * mg.blobs.TILE_H - 5, 15 * mg.blobs.TILE_W - 9), p, seed=21)
    for c in (4, 8):
        first, _ = check_mask(mg, mask, c, "many tiles")
        for _ in range(2):
            again = mg.blobs.label(dev(mask.astype(np.uint8)), 0, connectivity=c)
            assert torch.equal(again["labels"], first["labels"]) and torch.equal(again["stats"], first["stats"])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
def test_dtypes_polarity_nan_and_infinities(mg, dtype):
    rng = np.random.default_rng(11)
    h, w = 2 * mg.blobs.TILE_H + 1, 3 * mg.blobs.TILE_W + 5
    if np.dtype(dtype).kind == "u":
        plane = rng.integers(0, 256, size=(h, w)).astype(dtype)
        thresholds = [100.25, 140.5]
    else:
        plane = rng.normal(0.0, 1.0, size=(h, w)).astype(dtype)
        plane[rng.random((h, w)) < 0.05] = np.nan
        plane[rng.random((h, w)) < 0.02] = np.inf
        plane[rng.random((h, w)) < 0.02] = -np.inf
        thresholds = [-0.2304, 0.3701]
    for t in thresholds:
        for below in (False, True):
            for connectivity in (4, 8):
                check_label(mg, plane, t, below, connectivity)
            mask = mg.blobs.threshold_mask(dev(plane), t, below=below)  # the mask alone, as fill_holes takes it
            assert mask.dtype == torch.uint8 and np.array_equal(host(mask), br.on_mask(plane, t, below).astype(np.uint8))
    if np.dtype(dtype).kind == "f":  # NaN is off in both polarities
        on = host(mg.blobs.label(dev(plane), 0.0)["labels"]) >= 0
        off = host(mg.blobs.label(dev(plane), 0.0, below=True)["labels"]) >= 0
        assert not (on | off)[np.isnan(plane)].any() and (on | off)[~np.isnan(plane) & (plane != 0)].all()
    else:  # a pixel equal to an integer threshold is off both ways
        on = host(mg.blobs.label(dev(plane), 100)["labels"]) >= 0
        off = host(mg.blobs.label(dev(plane), 100, below=True)["labels"]) >= 0
        assert np.array_equal(on | off, plane != 100)


def test_structured_planes(mg):
    th, tw = mg.blobs.TILE_H, mg.blobs.TILE_W
    h, w = bc.structured_shape(th, tw)
    for c in (4, 8):
        got, _ = check_mask(mg, np.ones((h, w), dtype=bool), c, "all on")
        s = host(got["stats"])
        assert got["count"] == 1 and s.tolist() == [[h * w, w * h * (h - 1) // 2, h * w * (w - 1) // 2, 0, 0, h - 1, w - 1, 0]]
        got, _ = check_mask(mg, np.zeros((h, w), dtype=bool), c, "all off")
        assert got["count"] == 0 and (host(got["labels"]) == -1).all()
        got, _ = check_mask(mg, bc.corners_and_tile_corner(h, w, th, tw), c, "corners")
        assert got["count"] == 5  # the four round the tile corner are one component either way
        assert check_mask(mg, bc.pair(h, w, (th - 1, tw - 1), (th, tw)), c, "diagonal")[0]["count"] == (1 if c == 8 else 2)
        assert check_mask(mg, bc.pair(h, w, (th - 1, tw), (th, tw - 1)), c, "anti-diagonal")[0]["count"] == (1 if c == 8 else 2)
        m, path = bc.spiral(h, w)
        got, _ = check_mask(mg, m, c, "spiral")
        assert got["count"] == 1 and int(got["stats"][0, 7]) == 0 and int(got["stats"][0, 0]) == len(path)
        m[path[len(path) // 2]] = False
        assert check_mask(mg, m, c, "cut spiral")[0]["count"] == 2
        assert check_mask(mg, bc.comb(h, w), c, "comb")[0]["count"] == 1
        us, n = bc.nested_us(h, w)
        assert check_mask(mg, us, c, "nested U")[0]["count"] == n


def test_checkerboard_capacity_and_the_call_after_an_overflow(mg):
    h, w = bc.structured_shape(mg.blobs.TILE_H, mg.blobs.TILE_W)
    cb = bc.checkerboard(h, w)
    assert check_mask(mg, cb, 8, "checkerboard")[0]["count"] == 1
    k = (h * w + 1) // 2
    assert check_mask(mg, cb, 4, "checkerboard", max_components=k)[0]["count"] == k
    with pytest.raises(ValueError, match="max_components"):
        mg.blobs.label(dev(cb.astype(np.uint8)), 0, connectivity=4, max_components=k - 1)
    # the next call on the same workspace is exact again
    check_mask(mg, random_mask((h, w)), 4, "after the overflow", max_components=k - 1)
    check_mask(mg, random_mask((h, w)), 8, "after the overflow", max_components=k - 1)


def test_state_same_bits_twice_and_small_after_large(mg):
    th, tw = mg.blobs.TILE_H, mg.blobs.TILE_W
    big = random_mask((4 * th + 3, 5 * tw + 7), 0.59, seed=1)
    a, _ = check_mask(mg, big, 8, "first")
    b, _ = check_mask(mg, big, 8, "second")
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["stats"], b["stats"])
    for shape in [(th + 1, tw + 1), (3, 5), (1, 1)]:
        check_mask(mg, random_mask(shape, 0.59, seed=2), 8, "small after large")
    check_mask(mg, big, 4, "large again")


# ---- select ----------------------------------------------------------------------------------------------------------

def check_select(mg, mask, connectivity=8, **kw):
    got, (want_l, _, want_s) = check_mask(mg, mask, connectivity)
    out_l, out_s, out_t = br.select(want_l, want_s, **kw)
    sel = mg.blobs.select(got["labels"], got["stats"], **kw)
    assert sel["count"] == len(out_t), kw
    assert np.array_equal(host(sel["labels"]), out_l), kw
    assert np.array_equal(host(sel["stats"]), out_s) and np.array_equal(host(sel["table"]), out_t), kw
    assert sel["table"].dtype == torch.int32 and sel["labels"] is got["labels"]
    return sel


def test_select(mg):
    th, tw = mg.blobs.TILE_H, mg.blobs.TILE_W
    h, w = 2 * th + 5, 2 * tw + 9
    m = np.zeros((h, w), dtype=bool)
    m[0:4, 10:20] = True             # touches the top
    m[20:30, 0:3] = True             # the left
    m[h - 2:h, 40:70] = True         # the bottom
    m[30:40, w - 5:w] = True         # the right
    m[th - 3:th + 4, tw - 5:tw + 6] = True  # inside, over a tile corner: 77 pixels
    m[10:12, 30:33] = True           # inside: 6 pixels
    m[50, 100] = True                # inside: 1 pixel
    for kw in [dict(), dict(min_area=2), dict(min_area=7), dict(max_area=6), dict(min_area=2, max_area=40),
               dict(clear_border=True), dict(clear_border=True, min_area=2, max_area=76), dict(min_area=1000),
               dict(min_area=0)]:
        sel = check_select(mg, m, **kw)
        if kw == dict(min_area=1000):
            assert sel["count"] == 0 and set(host(sel["labels"]).reshape(-1).tolist()) == {-2, -1}
        if kw in (dict(), dict(min_area=0)):
            assert sel["count"] == 7 and (host(sel["labels"]) >= -1).all()
        if kw == dict(clear_border=True):
            assert sel["count"] == 3
    for p in (0.41, 0.59):
        for kw in [dict(min_area=3), dict(clear_border=True), dict(min_area=2, max_area=30, clear_border=True)]:
            check_select(mg, random_mask((h, w), p, seed=5), 4, **kw)
            check_select(mg, random_mask((h, w), p, seed=6), 8, **kw)


# ---- fill_holes ------------------------------------------------------------------------------------------------------

def check_fill(mg, mask, connectivity=8):
    want = br.fill_holes(mask)
    got = host(mg.blobs.fill_holes(dev(mask.astype(np.uint8))))
    assert got.dtype == np.uint8 and np.array_equal(got != 0, want) and got.max(initial=0) <= 1
    got_l = mg.blobs.label(dev(got), 0, connectivity=connectivity)
    want_l, want_k, want_s = br.label_mask(want, connectivity)
    assert got_l["count"] == want_k and np.array_equal(host(got_l["labels"]), want_l)
    assert np.array_equal(host(got_l["stats"]), want_s)
    return want


def test_fill_holes(mg):
    th, tw = mg.blobs.TILE_H, mg.blobs.TILE_W
    h, w = 2 * th + 7, 2 * tw + 11
    ring = bc.ellipse((h, w), 30, 60, 20, 14, 0.4) & ~bc.ellipse((h, w), 30, 60, 15, 9, 0.4)
    assert check_fill(mg, ring).sum() > ring.sum() + 100
    island = ring | bc.ellipse((h, w), 30, 60, 4, 3, 0.0)
    assert br.label_mask(island, 8)[1] == 2 and br.label_mask(check_fill(mg, island), 8)[1] == 1
    open_ring = np.zeros((h, w), dtype=bool)   # a ring whose hole reaches the frame: not filled
    open_ring[0:20, 5] = open_ring[0:20, 25] = True
    open_ring[19, 5:26] = True
    assert np.array_equal(check_fill(mg, open_ring), open_ring)
    gap = np.zeros((h, w), dtype=bool)         # a hole joined to the outside only by a diagonal gap: filled
    gap[10:20, 10:20] = True
    gap[11:19, 11:19] = False
    gap[10, 10] = False
    assert not gap[10, 10] and check_fill(mg, gap)[11:19, 11:19].all() and not check_fill(mg, gap)[10, 10]
    wide = np.zeros((h, w), dtype=bool)        # a hole spanning tiles
    wide[3:h - 3, 3:w - 3] = True
    wide[6:h - 6, 6:w - 6] = False
    assert check_fill(mg, wide)[6:h - 6, 6:w - 6].all()
    for seed in range(3):
        for c in (4, 8):
            check_fill(mg, random_mask((h, w), 0.59, seed=seed), c)
    check_fill(mg, np.zeros((h, w), dtype=bool))
    check_fill(mg, np.ones((h, w), dtype=bool))


def test_otsu_level_is_the_oracles(mg):
    plane, _, _ = bc.scene(3)
    u8, k, lo, hi = br.otsu_plane(plane)
    got = mg.blobs.to_uint8(dev(plane))
    assert np.array_equal(host(got), u8) and mg.blobs.otsu_level(got) == k


# ---- end to end ------------------------------------------------------------------------------------------------------

NAMES = ("x", "y", "valid", "clipped", "area", "bbox_top", "bbox_left", "bbox_bottom", "bbox_right", "x_centroid", "y_centroid")


def compare(xp, want):
    m = len(want["table"])
    assert xp.roi.sizes["mark"] == m
    assert np.array_equal(np.asarray(xp.roi.values).reshape(want["roi"].shape), want["roi"])
    for name in ("fg", "bg") + NAMES:
        got = np.asarray(xp[name].values)
        assert np.array_equal(got.reshape(want[name].shape), want[name]), name
    assert xp.attrs["blob_threshold"] == want["blob_threshold"] or (m == 0 and np.isnan(want["blob_threshold"]))
    assert xp.attrs["blob_components"] == want["blob_components"]


def inputs(mg, seed=0):
    """The scene as (y, x), as (channel, time, y, x) with 2 channels x 3 timepoints, and as float32: (DataArray, host
    image (C, T, H, W), search channel) of each."""
    plane, masks, ring = bc.scene(seed)
    rng = np.random.default_rng(100 + seed)
    stack = np.stack([rng.integers(0, 4000, size=(3,) + plane.shape).astype(np.uint16),
                      np.stack([plane, plane // 2, (plane // 3) + 7])])
    return {"plane": (mg.DataArray(plane, ("y", "x")), plane[None, None], None, 0),
            "stack": (mg.DataArray(data=stack, dims=("channel", "time", "y", "x"), coords={"channel": ["noise", "cells"]}),
                      stack, "cells", 1),
            "float32": (mg.DataArray(plane.astype(np.float32), ("y", "x")), plane.astype(np.float32)[None, None], None, 0)}, ring


@pytest.mark.parametrize("form", ["plane", "stack", "float32"])
def test_scene_end_to_end(mg, form):
    forms, ring = inputs(mg)
    data, image, channel, ch = forms[form]
    xp = mg.blobs(data, overlap=0, search_channel=channel)
    want = br.component(image, search_channel=ch)
    assert len(want["table"]) == bc.SCENE_BLOBS
    compare(xp, want)
    area = np.asarray(xp.area.values)
    assert not want["clipped"].any()
    fg_sum = np.asarray(xp.fg.sum(dim=["roi_x", "roi_y"]).values).reshape(len(area), -1)
    assert np.array_equal(fg_sum, np.repeat(area[:, None], fg_sum.shape[1], axis=1))
    # (the reductions take the dataset with all its dimensions: the same pipeline before restore_format)
    pipe = mg.blobs_pipe(overlap=0, search_channel=channel)
    pipe.remove_pipe("restore_format")
    full = pipe(data)
    assert full.roi.dims == ("mark", "channel", "time", "roi_y", "roi_x") and full.fg.dims == ("mark", "time", "roi_y", "roi_x")
    assert np.array_equal(np.asarray(full.roi.values), want["roi"]) and np.array_equal(np.asarray(full.fg.values), want["fg"])
    count, _, _ = mg.reduce.masked_stats(full, "fg")
    count = host(count.data).reshape(len(area), -1)
    assert np.array_equal(count, np.repeat(area[:, None], count.shape[1], axis=1))
    # fill_holes: the ring becomes its filled ellipse
    at = bc.mark_of(want["labels"], ring)
    filled_want = br.component(image, search_channel=ch, fill=True)
    filled = mg.blobs(data, overlap=0, search_channel=channel, fill_holes=True)
    compare(filled, filled_want)
    assert np.asarray(filled.area.values)[at] > area[at] + 50 and len(filled_want["table"]) == 12
    # a small roi_length: clipped / not valid on the blobs that do not fit, and on those only
    L = 24
    small_want = br.component(image, search_channel=ch, roi_length=L)
    small = mg.blobs(data, overlap=0, search_channel=channel, roi_length=L)
    compare(small, small_want)
    clipped = np.asarray(small.clipped.values)
    sides = np.maximum(want["bbox_bottom"] - want["bbox_top"], want["bbox_right"] - want["bbox_left"]) + 1
    assert clipped.any() and not clipped.all() and clipped[sides > L].all() and sides[clipped].min() > sides[~clipped].min()
    assert np.array_equal(np.asarray(small.valid.values).reshape(12, -1), np.repeat(~clipped[:, None], image.shape[1], axis=1))


def wrap(mg, form, image):
    """A host image (C, T, H, W) as the DataArray of ``form``, as ``inputs`` makes them."""
    if form == "stack":
        return mg.DataArray(data=image, dims=("channel", "time", "y", "x"), coords={"channel": ["noise", "cells"]})
    return mg.DataArray(image[0, 0], ("y", "x"))


SAME_MARKS = ("fg", "bg") + NAMES  # everything but the pixels themselves


@pytest.mark.parametrize("form", ["plane", "stack", "float32"])
def test_dark_polarity_on_the_inverted_scene_gives_the_same_marks(mg, form):
    """65535 - v mirrors the uint8 bins of the scene exactly (the oracle's maps of the two are the same bits), so the
    dark marks of the inverted scene are the bright marks of the scene, value for value."""
    forms, _ = inputs(mg)
    data, image, channel, ch = forms[form]
    inverted = (65535 - image).astype(image.dtype)
    bright = mg.blobs(data, overlap=0, search_channel=channel)
    dark = mg.blobs(wrap(mg, form, inverted), overlap=0, search_channel=channel, polarity="dark")
    compare(dark, br.component(inverted, search_channel=ch, polarity="dark"))
    assert dark.roi.sizes["mark"] == bright.roi.sizes["mark"] == 12
    for name in SAME_MARKS:
        assert dark[name].dims == bright[name].dims, name
        assert np.array_equal(np.asarray(dark[name].values), np.asarray(bright[name].values)), name
    assert dark.attrs["blob_components"] == bright.attrs["blob_components"]
    # and a number as the threshold, both ways
    by_number = []
    for polarity, img, t in (("bright", image, 800), ("dark", inverted, 65535 - 800)):
        xp = mg.blobs(wrap(mg, form, img), overlap=0, search_channel=channel, threshold=t, polarity=polarity)
        compare(xp, br.component(img, search_channel=ch, threshold=t, polarity=polarity))
        assert xp.roi.sizes["mark"] == 12 and xp.attrs["blob_threshold"] == t
        by_number.append(xp)
    for name in SAME_MARKS:  # v > 800 is 65535 - v < 64735
        assert np.array_equal(np.asarray(by_number[0][name].values), np.asarray(by_number[1][name].values)), name


@pytest.mark.parametrize("form", ["plane", "stack", "float32"])
def test_flat_plane_gives_no_marks(mg, form):
    """The plane that decides -- time 0 of the search channel -- is flat; in the stack the other planes are not."""
    if form == "stack":
        flat = np.random.default_rng(9).integers(0, 4000, size=(2, 3, 64, 80)).astype(np.uint16)
        flat[1, 0] = 7
        channel, ch = "cells", 1
    else:
        flat = np.full((1, 1, 64, 80), 7, dtype=np.float32 if form == "float32" else np.uint16)
        channel, ch = None, 0
    xp = mg.blobs(wrap(mg, form, flat), overlap=0, search_channel=channel)
    want = br.component(flat, search_channel=ch)
    assert xp.roi.sizes["mark"] == 0 and len(want["table"]) == 0 and xp.attrs["blob_components"] == 0
    assert np.isnan(xp.attrs["blob_threshold"])
    for name in ("fg", "bg") + NAMES:
        assert np.asarray(xp[name].values).size == 0, name
    assert np.asarray(xp.roi.values).size == 0
    # everything rejected by the selection is as empty
    forms, _ = inputs(mg, seed=2)
    data, image, channel, ch = forms[form]
    none = mg.blobs(data, overlap=0, search_channel=channel, min_area=5000)
    compare(none, br.component(image, search_channel=ch, min_area=5000))
    assert none.roi.sizes["mark"] == 0 and none.attrs["blob_components"] >= 12


def test_windows_that_cannot_be_are_refused(mg):
    big = np.zeros((300, 400), dtype=np.uint16)
    big[20:280, 30:60] = 1000
    with pytest.raises(ValueError, match="max_area or roi_length"):
        mg.blobs(mg.DataArray(big, ("y", "x")), overlap=0)
    small = np.zeros((20, 400), dtype=np.uint16)
    small[2:18, 30:60] = 1000
    with pytest.raises(ValueError, match="max_area or roi_length"):
        mg.blobs(mg.DataArray(small, ("y", "x")), overlap=0)


def test_smooth_is_the_blurred_plane_at_its_own_otsu_level(mg):
    plane, _, _ = bc.scene(4)
    xp = mg.blobs(mg.DataArray(plane, ("y", "x")), overlap=0, smooth=True)
    assert xp.roi.sizes["mark"] == 12
    blurred = mg.blobs.to_uint8(dev(plane), smooth=True)
    assert not torch.equal(blurred, mg.blobs.to_uint8(dev(plane)))
    k = mg.blobs.otsu_level(blurred)
    found = mg.blobs.label(blurred, k + 0.5)
    kept = mg.blobs.select(found["labels"], found["stats"], min_area=20)
    labels = host(kept["labels"])
    assert xp.attrs["blob_components"] == found["count"] and kept["count"] == 12
    assert np.array_equal(np.asarray(xp.area.values), host(kept["stats"])[:, 0])
    L = xp.roi.sizes["roi_y"]
    fg = np.asarray(xp.fg.values).reshape(12, L, L)
    for i, (row, col, _) in enumerate(host(kept["table"]).tolist()):
        top, bottom, left, right = mg.utils.bounding_box(col, row, L, plane.shape[1], plane.shape[0])
        assert np.array_equal(fg[i], labels[top:bottom, left:right] == i), i


def test_save_load_and_overview(mg, tmp_path):
    forms, _ = inputs(mg)
    data, image, channel, ch = forms["stack"]
    xp = mg.blobs(data, overlap=0, search_channel=channel)
    mg.save(tmp_path / "blobs.nc", xp)
    back = mg.load(tmp_path / "blobs.nc")
    for name in ("roi", "fg", "bg") + NAMES:
        assert back[name].dims == xp[name].dims, name
        assert np.array_equal(np.asarray(back[name].values), np.asarray(xp[name].values)), name
    assert back.attrs["blob_components"] == xp.attrs["blob_components"]
    assert back.attrs["blob_threshold"] == xp.attrs["blob_threshold"]
    picture = mg.plot.overview(xp)
    values = host(picture.data) if isinstance(picture.data, torch.Tensor) else np.asarray(picture.values)
    assert values.dtype == np.uint8 and values.shape[-1] == 3 and values.shape[0] == 3 and values.max() > 0
