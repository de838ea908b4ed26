"""What of the masked ROI statistics can be held to account without a GPU: the oracle against NumPy's own nan-reductions,
the restated linear interpolation against ``np.nanquantile`` bit for bit, the new host reductions of ``DataArray``,
``where`` on host arrays (unchanged), and the C entry points' declaration and export."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import roistats_ref as ref

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_window(dtype, L, rng, nan_share=0.2):
    v = ref.full_range(dtype, (L, L), rng)
    if np.dtype(dtype).kind == "f":
        v[rng.random((L, L)) < nan_share] = np.nan
    return v


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_agrees_with_numpy(dtype):
    rng = np.random.default_rng(3)
    q = (0, 0.1, 0.5, 0.998, 1)
    for L in (1, 2, 5, 12):
        for kind in ref.MASK_KINDS:
            v, m = random_window(dtype, L, rng), ref.make_mask(kind, L, rng)
            rec = ref.window(v, m, q)
            v64 = np.where(m, v.astype(np.float64), np.nan)
            assert rec["n"] == np.count_nonzero(~np.isnan(v64))
            if rec["n"] == 0:
                assert np.isnan(rec["min"]) and np.isnan(rec["max"]) and np.isnan(rec["order"]).all()
                assert rec["sum"] == 0 and rec["m2"] == 0
                continue
            assert rec["min"] == np.nanmin(v64) and rec["max"] == np.nanmax(v64)
            np.testing.assert_allclose(float(rec["sum"]), np.nansum(v64), rtol=1e-13)
            np.testing.assert_allclose(float(rec["m2"]) / rec["n"], np.nanvar(v64), rtol=1e-9, atol=0)
            np.testing.assert_allclose(np.sqrt(float(rec["m2"]) / rec["n"]), np.nanstd(v64), rtol=1e-9)
            np.testing.assert_array_equal(rec["quantile"], np.nanquantile(v64, q))
            # the order statistics are the neighbours np.nanquantile interpolates between
            np.testing.assert_array_equal(ref.interpolate(rec["n"], rec["order"], q), rec["quantile"])
            assert rec["order"][0, 0] == rec["min"] and rec["order"][-1, 1] == rec["max"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolation_is_nanquantile_bit_for_bit(dtype):
    """``reduce.interpolate_quantiles`` (the formula the device results go through, here on NumPy arrays) on random
    windows with NaNs, random and edge fractions."""
    from magnify_amd import reduce

    rng = np.random.default_rng(7)
    for trial in range(400):
        L = int(rng.integers(1, 9))
        v, m = random_window(dtype, L, rng), rng.random((L, L)) < rng.random()
        q = np.concatenate([rng.random(4), rng.choice([0.0, 0.5, 1.0, 0.998, 0.01], 2)])
        rec = ref.window(v, m, q)
        got = reduce.interpolate_quantiles(np.int32(rec["n"]), rec["order"], q)
        assert got.dtype == np.float64
        assert np.array_equal(got, rec["quantile"], equal_nan=True), (trial, rec["n"], q)


def test_host_reductions_of_dataarray():
    import magnify_amd as mg

    rng = np.random.default_rng(9)
    v = rng.standard_normal((3, 4, 5, 5))
    v[rng.random(v.shape) < 0.3] = np.nan
    v[0, 0] = np.nan
    arr = mg.DataArray(v, ("mark", "time", "roi_y", "roi_x"), coords={"mark": np.arange(3)})
    dim, axes = ["roi_x", "roi_y"], (-1, -2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.testing.assert_array_equal(arr.std(dim=dim).values, np.nanstd(v, axis=axes))
        np.testing.assert_array_equal(arr.std(dim=dim, ddof=1).values, np.nanstd(v, axis=axes, ddof=1))
        np.testing.assert_array_equal(arr.var(dim=dim, ddof=1).values, np.nanvar(v, axis=axes, ddof=1))
        np.testing.assert_array_equal(arr.var().values, np.nanvar(v))
        got = arr.quantile([0.1, 0.9], dim=dim)
        assert got.dims == ("quantile", "mark", "time") and "mark" in got.coords
        np.testing.assert_array_equal(got.values, np.nanquantile(v, [0.1, 0.9], axis=axes))
        np.testing.assert_array_equal(got.coords["quantile"].values, [0.1, 0.9])
        assert arr.quantile(0.5, dim="roi_x").dims == ("mark", "time", "roi_y")
        np.testing.assert_array_equal(arr.quantile(0.5, dim="roi_x").values, np.nanquantile(v, 0.5, axis=-1))
        np.testing.assert_array_equal(arr.quantile(0.25).values, np.nanquantile(v, 0.25))
    cnt = arr.count(dim=dim)
    assert cnt.dims == ("mark", "time")
    np.testing.assert_array_equal(cnt.values, (~np.isnan(v)).sum(axis=axes))
    assert cnt.values[0, 0] == 0 and arr.count().item() == (~np.isnan(v)).sum()
    ints = mg.DataArray(np.arange(24, dtype=np.uint16).reshape(2, 3, 4), ("a", "b", "c"))
    np.testing.assert_array_equal(ints.count(dim="c").values, np.full((2, 3), 4))
    np.testing.assert_array_equal(ints.std(dim="c").values, np.std(ints.values.astype(np.float64), axis=-1))


def test_where_on_host_arrays_is_unchanged():
    """Same dtype, same bytes, a NumPy array at once (no lazy operand) -- for a mask by DataArray and by name, with
    broadcasting over a missing channel dimension and with a cond dimension the array does not have."""
    import magnify_amd as mg

    rng = np.random.default_rng(10)
    roi = rng.integers(0, 65536, (3, 2, 2, 4, 4)).astype(np.uint16)
    fg = rng.random((3, 2, 4, 4)) < 0.5
    ds = mg.Dataset({"roi": mg.DataArray(roi, ("mark", "channel", "time", "roi_y", "roi_x"))},
                    coords={"fg": (("mark", "time", "roi_y", "roi_x"), fg)})
    want = np.where(fg[:, None], roi.astype(np.float64), np.nan)
    for got in (ds.roi.where(ds.fg), ds.roi.where("fg"), ds.where(ds.fg).roi, ds.where("fg").roi):
        assert isinstance(got.raw, np.ndarray) and got.dtype == np.float64 and got.dims == ds.roi.dims
        assert got.values.tobytes() == want.tobytes()
    np.testing.assert_array_equal(ds.roi.where(ds.fg).mean(dim=["roi_x", "roi_y"]).values, np.nanmean(want, axis=(-1, -2)))
    wider = mg.DataArray(rng.random((3, 5)) < 0.5, ("mark", "extra"))
    got = mg.DataArray(roi[:, 0, 0, 0, 0], ("mark",)).where(wider)
    assert got.dims == ("mark", "extra")
    np.testing.assert_array_equal(got.values, np.where(wider.values, roi[:, 0, 0, 0, 0].astype(np.float64)[:, None], np.nan))


def test_entry_points_are_declared_and_exported():
    from magnify_amd import _native, hotpath

    with open(os.path.join(ROOT, "include", "magnify_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+mg_roi_masked_stats\s*\(", header) and "mg_roi_masked_stats_keys_in_lds" in header
    assert len(_native.PROTOTYPES["mg_roi_masked_stats"]) == 15
    assert _native.PROTOTYPES["mg_roi_masked_stats_keys_in_lds"] == [ctypes.c_int, ctypes.c_int]
    assert (hotpath.ROISTATS_MAX_Q, hotpath.ROISTATS_LDS_KEY_BYTES) == (16, 49152)  # (read from the header: its values)
    lib = _native.lib()
    assert lib.mg_roi_masked_stats and lib.mg_roi_masked_stats_keys_in_lds
    # the query needs no device: which side of the LDS budget a window falls on, and what it refuses
    budget = hotpath.ROISTATS_LDS_KEY_BYTES
    for dtype, key_bytes in ((np.uint8, 4), (np.uint16, 4), (np.float32, 4), (np.float64, 8)):
        for L in (1, 64, 78, 79, 100, 110, 111, 200):
            assert hotpath.masked_stats_keys_in_lds(dtype, L) == (L * L * key_bytes <= budget)
    assert lib.mg_roi_masked_stats_keys_in_lds(9, 10) == -1 and lib.mg_roi_masked_stats_keys_in_lds(1, 0) == -1
    # refusals that are decided before anything is launched (no device needed: nothing is launched)
    q = np.array([0.5], dtype=np.float64)
    args = lambda **kw: [kw.get("roi", 16), kw.get("dtype", 1), kw.get("mask", 16), 49, 0, kw.get("m", 1), 1, 1,  # noqa: E731
                         kw.get("L", 7), kw.get("q", q.ctypes.data), kw.get("n_q", 1), 16, 16, kw.get("order", 16), None]
    for bad in (dict(roi=None), dict(mask=None), dict(dtype=7), dict(m=-1), dict(L=0), dict(n_q=17), dict(n_q=-1),
                dict(q=None), dict(order=None), dict(q=np.array([-0.1]).ctypes.data), dict(q=np.array([1.1]).ctypes.data),
                dict(q=np.array([np.nan]).ctypes.data)):
        assert lib.mg_roi_masked_stats(*args(**bad)) == -1, bad
    assert lib.mg_roi_masked_stats(*args(m=0)) == 0
