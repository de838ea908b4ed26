"""What the window features share on the host: the per-marker int32 table a kernel reads (``hotpath._marker_table_view``),
one timepoint of a dataset (``_dataset.time_pick`` / ``roi_windows``), a caller's array per marker, a bead's own pixels,
the origin of a marker's window, "a finite number" and the limits of the 1/16-pixel geometry.  Shapes, strides and
indices only: nothing here needs a device."""
import math

import numpy as np
import pytest
import torch

import magnify_amd as mg
from magnify_amd import _dataset, hotpath, utils
from magnify_amd import _native as nat

M, T = 3, 3


# ---- hotpath._marker_table_view --------------------------------------------------------------------------------------------

def table(k, m=M, t=T, extra=0):
    return torch.arange(m * t * (k + extra), dtype=torch.int32).reshape(m, t, k + extra)


@pytest.mark.parametrize("k", [2, 3])
def test_marker_table_view_hands_tables_on_where_they_lie(k):
    view = lambda x, m=M: hotpath._marker_table_view("rows", x, m, T, k, "cpu")  # noqa: E731
    full = table(k)
    got, sm, st = view(full)
    assert got.data_ptr() == full.data_ptr() and (sm, st) == (T * k, k)
    got, sm, st = view(full[:, 0])  # (M, k): one row for all timepoints
    assert got.shape == (M, 1, k) and got.data_ptr() == full.data_ptr() and (sm, st) == (T * k, 0)
    one = table(k, t=1)
    got, sm, st = view(one.expand(M, T, k))  # expanded along time: not copied, stride 0
    assert got.data_ptr() == one.data_ptr() and (sm, st) == (k, 0)
    big = table(k, extra=1)
    got, sm, st = view(big[:, :, :k])  # rows of a wider table: read in place
    assert got.data_ptr() == big.data_ptr() and (sm, st) == (T * (k + 1), k + 1)
    wide = table(2 * k)
    got, sm, st = view(wide[..., ::2])  # an inner stride of 2: copied
    assert got.data_ptr() != wide.data_ptr() and (sm, st) == (T * k, k)
    assert torch.equal(got, wide[..., ::2])
    got, sm, st = view(full[:1], 1)  # one marker: its stride only ever multiplies 0
    assert got.data_ptr() == full.data_ptr() and (sm, st) == (0, k)
    got, sm, st = view(full.numpy().astype(np.int64))  # a host array of another integer type is converted
    assert got.dtype == torch.int32 and torch.equal(got, full) and (sm, st) == (T * k, k)


@pytest.mark.parametrize("k", [2, 3])
def test_marker_table_view_refusals(k):
    with pytest.raises(TypeError, match="rows"):
        hotpath._marker_table_view("rows", table(k).to(torch.int64), M, T, k, "cpu")
    for shape in [(k,), (M, T, k, 1), (M + 1, T, k), (M, 2, k), (M, T, k + 1)]:
        with pytest.raises(ValueError, match="rows"):
            hotpath._marker_table_view("rows", torch.zeros(shape, dtype=torch.int32), M, T, k, "cpu")
        with pytest.raises(ValueError, match="rows"):
            hotpath._marker_table_view("rows", np.zeros(shape, dtype=np.int32), M, T, k, "cpu")


def test_mask_view_of_no_mask():
    assert hotpath._mask_view("no mask", None, M, T, 5) == (None, 0, 0)
    mask = torch.ones((M, T, 5, 5), dtype=torch.bool)
    got, sm, st = hotpath._mask_view("a mask", mask, M, T, 5)
    assert got.dtype == torch.uint8 and got.data_ptr() == mask.data_ptr() and (sm, st) == (T * 25, 25)


# ---- one timepoint ---------------------------------------------------------------------------------------------------------

def host_tensor(var, dims, as_mask=False):
    """``_dataset.device_tensor`` without the upload."""
    data = torch.from_numpy(np.ascontiguousarray(var.transpose(*[d for d in dims if d in var.dims]).values))
    if "time" in dims and "time" not in var.dims:
        data = data.unsqueeze([d for d in dims if d in var.dims or d == "time"].index("time"))
    return data


def dataset(L=4, h=30, w=40, chip=False):
    rng = np.random.default_rng(5)
    coords = {"fg": (("mark", "time", "roi_y", "roi_x"), rng.random((M, T, L, L)) > 0.5),
              "bg": (("mark", "time", "roi_y", "roi_x"), rng.random((M, T, L, L)) > 0.5),
              "drawn": (("mark", "roi_y", "roi_x"), rng.random((M, L, L)) > 0.5),
              "x": (("mark", "time"), rng.uniform(0, w, (M, T))), "y": (("mark", "time"), rng.uniform(0, h, (M, T)))}
    if chip:
        coords["tag"] = (("mark",), np.array(["a"] * M))
    return mg.Dataset({"roi": mg.DataArray(rng.integers(0, 999, (M, 2, T, L, L)).astype(np.uint16), _dataset.ROI_DIMS),
                       "image": mg.DataArray(np.zeros((2, T, h, w), dtype=np.uint16), ("channel", "time", "im_y", "im_x"))},
                      coords=coords)


@pytest.mark.parametrize("time", [None, 0, 1, 2, -1])
def test_time_pick_selects_what_the_written_out_slices_selected(time, monkeypatch):
    monkeypatch.setattr(_dataset, "device_tensor", host_tensor)
    ds = dataset()
    roi, fg, drawn = ds.data_vars["roi"].values, ds.coords["fg"].values, ds.coords["drawn"].values
    if time is None:
        assert _dataset.time_pick(time) is None
        want_roi, want_fg = roi, fg
    else:
        assert _dataset.time_pick(time) == (slice(time, time + 1) if time != -1 else slice(-1, None))
        want_roi = ds.data_vars["roi"].isel(time=slice(time, time + 1) if time != -1 else slice(-1, None)).values
        want_fg = ds.coords["fg"].isel(time=slice(time, time + 1) if time != -1 else slice(-1, None)).values
        assert want_roi.shape[2] == 1 and want_fg.shape[1] == 1
    got_roi, got_fg = _dataset.roi_windows(ds, "fg", time)  # a mask per timepoint
    np.testing.assert_array_equal(got_roi.numpy(), want_roi)
    np.testing.assert_array_equal(got_fg.numpy(), want_fg)
    got_roi, got_drawn = _dataset.roi_windows(ds, ds.coords["drawn"], time)  # one mask for all: never sliced
    np.testing.assert_array_equal(got_roi.numpy(), want_roi)
    np.testing.assert_array_equal(got_drawn.numpy(), drawn[:, None])
    got_roi, none = _dataset.roi_windows(ds, None, time)  # every pixel
    np.testing.assert_array_equal(got_roi.numpy(), want_roi)
    assert none is None
    x, y = ds.coords["x"].values, ds.coords["y"].values
    if time is not None:
        x, y = (x[:, time:time + 1], y[:, time:time + 1]) if time != -1 else (x[:, -1:], y[:, -1:])
    got_y, got_x, top, left = _dataset.marker_windows(ds, 4, time, "a test", "centre")
    np.testing.assert_array_equal(got_x, x)
    np.testing.assert_array_equal(got_y, y)
    assert top.shape == left.shape == x.shape


@pytest.mark.parametrize("time", [None, 1, -1])
def test_roi_windows_own_mask(time, monkeypatch):
    monkeypatch.setattr(_dataset, "device_tensor", host_tensor)
    ds = dataset()
    own = ds.coords["fg"].values | ds.coords["bg"].values
    _, got = _dataset.roi_windows(ds, "own", time)
    np.testing.assert_array_equal(got.numpy().astype(bool), own if time is None else own[:, [time]])
    assert _dataset.roi_windows(dataset(chip=True), "own", time)[1] is None  # a chip: every pixel
    with pytest.raises(KeyError):
        _dataset.roi_windows(ds, "no_such_mask", time)
    ds["roi"] = mg.DataArray(ds.data_vars["roi"].values.astype(np.int32), _dataset.ROI_DIMS)
    with pytest.raises(TypeError):  # not a pixel type of the hot path
        _dataset.roi_windows(ds, None, time)


# ---- own_mask --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_own_mask(dtype):
    rng = np.random.default_rng(6)
    fg, bg = (torch.from_numpy(rng.random((M, T, 5, 5)) > 0.6).to(dtype) for _ in range(2))
    got = _dataset.own_mask(fg, bg)  # a mask per timepoint
    assert got.dtype == torch.uint8 and got.shape == (M, T, 5, 5)
    assert torch.equal(got.bool(), fg.bool() | bg.bool())
    for shared in ((fg[:, :1], bg[:, :1]), (fg[:, :1].expand(M, T, 5, 5), bg[:, 1:2])):  # one drawn mask for all timepoints
        got = _dataset.own_mask(*shared)
        assert got.dtype == torch.uint8 and got.shape == (M, 1, 5, 5)
        assert torch.equal(got.bool(), shared[0][:, :1].bool() | shared[1][:, :1].bool())
    got = _dataset.own_mask(fg[:, :1], bg)  # only one of the two is shared
    assert got.shape == (M, T, 5, 5) and torch.equal(got.bool(), fg[:, :1].bool() | bg.bool())


# ---- per_marker ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3])
def test_per_marker(k):
    rng = np.random.default_rng(7)
    full = rng.uniform(-5, 5, (M, T, k))
    for value, want in ((full[:, 0], full[:, :1]), (full[:, :1], full[:, :1]), (full, full), (full.tolist(), full),
                        (mg.DataArray(full.transpose(1, 0, 2), ("time", "mark", "component")), full),
                        (mg.DataArray(full[:, 0], ("mark", "component")), full[:, :1])):
        got = _dataset.per_marker("caller", value, M, T, k, "centre")
        assert got.dtype == np.float64 and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
    assert _dataset.per_marker("caller", np.zeros((0, k)), 0, T, k, "centre").shape == (0, 1, k)
    bad = [np.zeros((M + 1, k)), np.zeros((M, 2, k)), np.zeros((M, T, k + 1)), np.zeros((M, k - 1)), np.zeros(k),
           np.zeros((M, T, k, 1))]
    for value in (np.nan, np.inf, -np.inf):
        bad.append(full.copy())
        bad[-1][1, 2, 0] = value
    for value in bad:
        with pytest.raises(ValueError, match="caller: circle="):
            _dataset.per_marker("caller", value, M, T, k, "circle")


# ---- window_origin ---------------------------------------------------------------------------------------------------------

def test_window_origin_is_bounding_box_for_arrays():
    cases = [(size, L, c) for size in range(1, 14) for L in range(1, size + 1) for c in range(-4, size + 4)]
    assert len(cases) == 1547
    for size in range(1, 14):
        for L in range(1, size + 1):
            c = np.arange(-4, size + 4)
            got = utils.window_origin(c, L, size)
            assert got.shape == c.shape and got.dtype == np.int64
            for ci, g in zip(c.tolist(), got.tolist()):
                top, bottom, left, right = utils.bounding_box(ci, ci, L, size, size)
                assert g == top == left and bottom - top == L and 0 <= top <= size - L, (size, L, ci)
    c = np.array([[0, 7], [39, 20]], dtype=np.int32)  # any shape, any integer type
    np.testing.assert_array_equal(utils.window_origin(c, 8, 40), [[0, 3], [32, 16]])


# ---- number ----------------------------------------------------------------------------------------------------------------

def test_number():
    assert utils.number("a width", np.float32(2)) == 2.0 and type(utils.number("a width", np.float32(2))) is float
    assert utils.number("a width", 3) == 3.0 and utils.number("a width", np.int64(-4)) == -4.0
    assert utils.number("a width", 0.25) == 0.25
    for bad in (True, np.True_, "1", None, math.nan, math.inf, -math.inf, np.float32("nan"), 1j, [1.0]):
        with pytest.raises(ValueError, match="a width"):
            utils.number("a width", bad)


# ---- the limits of the 1/16-pixel geometry, as the header states them ------------------------------------------------------

def test_header_limits():
    from magnify_amd import profile

    assert nat.DEFINES["MG_PROFILE_SUBPIXEL"] == 16
    assert nat.DEFINES["MG_PROFILE_CENTRE_MIN"] == -1024 * 16
    assert nat.DEFINES["MG_PROFILE_CENTRE_MAX"] == 2048 * 16
    assert nat.DEFINES["MG_PROFILE_MAX_EDGE"] == math.isqrt(2**31 - 1) == 46340
    assert nat.DEFINES["MG_REFINE_MAX_RADIUS"] == 1024 * 16
    assert (profile.CENTRE_MIN, profile.CENTRE_MAX, profile.MAX_EDGE) == (-16384, 32768, 46340)
    np.testing.assert_array_equal(profile.quantised([0.03125, 0.09375, -1e300, 1e300, 2.53]), [0, 2, -2**30, 2**30, 40])
    assert profile.quantised([1.0]).dtype == np.int32
