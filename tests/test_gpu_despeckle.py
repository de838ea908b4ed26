"""Hot-pixel removal on the device: mg_despeckle_planes / mg_outlier_votes through ``magnify_amd.despeckle``, equal by
value to the NumPy oracle (tests/despeckle_ref.py; NaN equal to NaN), the refusals, and ``despeckle=`` end to end."""

import numpy as np
import pytest
import torch

import despeckle_ref as sr
from synth import draw_beads, draw_chip

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
TESTS = ("bright", "dark", "both")


@pytest.fixture(scope="module")
def mg():
    import magnify_amd

    magnify_amd.hotpath = __import__("magnify_amd.hotpath", fromlist=["x"])
    magnify_amd.hotpath.require_gpu()
    magnify_amd.seed(1234)
    return magnify_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def top_of(dtype):
    dtype = np.dtype(dtype)
    return np.iinfo(dtype).max if dtype.kind == "u" else np.finfo(dtype).max


def check(mg, block, k, which, threshold, med=None, label=None, defects=None):
    """One call on a host block (N, H, W) against the oracle: the planes and the counts.  -> (out, counts) of the device."""
    d = dev(block)
    if which == "all":
        got = host(mg.despeckle.median(d, k))
        assert sr.same(got, sr.median(block, k) if med is None else med), (label, k, which)
        return got, None
    want, want_counts = sr.remove(block, k, which, threshold, defects=defects, med=med)
    out, counts = mg.despeckle.remove_outliers(d, threshold, k, which, defects=defects)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == block.shape[:-2]
    assert sr.same(host(out), want), (label, k, which, threshold)
    np.testing.assert_array_equal(host(counts), want_counts, err_msg=str((label, k, which, threshold)))
    return host(out), host(counts)


# ---- shapes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_radii_and_tests(mg, dtype):
    rng = np.random.default_rng(41)
    tile = mg.despeckle.TILE
    for h, w in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53), (tile, tile + 1), (2 * tile + 1, tile - 1), (64, 257)):
        block3, threshold = sr.random_planes(rng, dtype, (3, h, w))
        for k in (1, 2):
            med3 = sr.median(block3, k)
            for n in (1, 3):
                for which in TESTS + ("all",):
                    _, counts = check(mg, block3[:n], k, which, threshold, med3[:n], (dtype.__name__, n, h, w))
                    if which == "both" and n == 3 and h * w > 1000:  # some specks pass, not all of them
                        assert 0 < counts.sum() < sr.flags(block3, k, "both", 0.6 * threshold, med3).sum()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_plane_never_sees_its_neighbour_in_memory(mg, dtype):
    """The last rows of plane 0 are at the top of the range and plane 1 is constant: a halo that ran on into the next
    (or back into the last) plane would find outliers in plane 1."""
    rng = np.random.default_rng(42)
    tile = mg.despeckle.TILE
    for h, w in ((1, 1), (5, 7), (tile, tile), (tile + 3, 2 * tile + 1)):
        block = np.empty((2, h, w), dtype=dtype)
        block[0] = sr.random_planes(rng, dtype, (h, w))[0]
        block[0, -2:] = top_of(dtype)
        block[1] = 7
        for k in (1, 2):
            for which in TESTS:
                out, counts = check(mg, block, k, which, 0.0, label=(dtype.__name__, h, w))
                assert counts[1] == 0 and sr.same(out[1], block[1])


# ---- values ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_integer_range_and_fractional_thresholds(mg, dtype):
    rng = np.random.default_rng(43)
    top = int(top_of(dtype))
    block = (rng.integers(0, 2, size=(2, 37, 53)) * top).astype(dtype)  # only 0 and the maximum
    for k in (1, 2):
        med = sr.median(block, k)
        for which in TESTS:
            for threshold in (0, 0.5, top - 0.5, top):
                out, counts = check(mg, block, k, which, threshold, med, dtype.__name__)
                if threshold == top:
                    assert counts.sum() == 0  # a difference of exactly the range is not above it
                elif which == "both":
                    assert counts.sum() == (block != med).sum()  # every pixel off its median, none that equals it
    flat = np.full((1, 9, 9), top, dtype=dtype)
    flat[0, 4, 4] = 0
    assert check(mg, flat, 1, "dark", top - 0.5)[1].tolist() == [1]
    assert check(mg, flat, 1, "dark", float(top))[1].tolist() == [0]
    assert check(mg, flat, 1, "bright", 0)[1].tolist() == [0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_specials(mg, dtype):
    rng = np.random.default_rng(44)
    nan, inf = np.nan, np.inf
    block = rng.normal(-100.0, 50.0, size=(2, 41, 45)).astype(dtype)  # negative values
    block[0, 5, 5] = nan            # a NaN pixel among numbers
    block[0, 10:14, 10:14] = nan    # windows more than half NaN (k = 1: the inner 2 x 2; k = 2: around its centre)
    block[0, 20, 20] = inf          # +inf over a finite median
    block[0, 28:33, 28:33] = inf    # +inf where the median is +inf
    block[0, 36, 8] = -inf          # -inf under "dark"
    block[1, 0, 0] = nan            # the corner counts four times in its own window
    block[1, 40, 44] = inf
    block[1, 3:6, 30:36] = -inf
    block[1, 20, 3] = -0.0
    for k in (1, 2):
        med = sr.median(block, k)
        assert np.isnan(med[0, 11, 11]) and med[0, 30, 30] == inf and np.isfinite(med[0, 20, 20])
        for which in TESTS + ("all",):
            for threshold in (0.0, 10.5):
                out, _ = check(mg, block, k, which, threshold, med, dtype.__name__)
                if which == "all":
                    continue
                assert np.isnan(out[0, 5, 5]) and np.isnan(out[0, 10:14, 10:14]).all() and np.isnan(out[1, 0, 0])  # NaN stays
                assert (out[0, 29:32, 29:32] == inf).all()  # inf - inf is no outlier
                assert np.isfinite(out[0, 20, 20]) == (which != "dark")
                assert np.isfinite(out[0, 36, 8]) == (which != "bright")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties(mg, dtype):
    yy, xx = np.mgrid[0:23, 0:70]
    for values in ((5, 5), (3, 200), (0, int(min(top_of(dtype), 65535)))):
        board = np.where((yy + xx) & 1, values[1], values[0]).astype(dtype)
        block = np.stack([board, board[:, ::-1], np.full_like(board, values[1])])
        for k in (1, 2):
            med = sr.median(block, k)
            for which in ("both", "all"):
                check(mg, block, k, which, 0.0, med, (dtype.__name__, values))
    out, counts = check(mg, np.full((2, 9, 9), 5, dtype=dtype), 2, "both", 0.0)
    assert counts.tolist() == [0, 0]


# ---- the defect map --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_defect_map(mg, dtype):
    rng = np.random.default_rng(45)
    tile = mg.despeckle.TILE
    h, w = tile + 5, 2 * tile + 3
    block, threshold = sr.random_planes(rng, dtype, (3, h, w))
    if np.dtype(dtype).kind == "f":
        block[1, 7, 9] = np.nan
    none = np.zeros((h, w), dtype=bool)
    some = np.where(rng.random((h, w)) < 0.05, rng.integers(1, 256, size=(h, w)), 0).astype(np.uint8)
    some[7, 9] = 1
    for k in (1, 2):
        med = sr.median(block, k)
        out, counts = check(mg, block, k, "dark", threshold, med, dtype.__name__, defects=none)
        assert sr.same(out, block) and counts.tolist() == [0, 0, 0]
        for given in (some, some != 0, dev(some), dev(some != 0)):
            out, counts = mg.despeckle.remove_outliers(dev(block), 0, k, "bright", defects=given)
            out = host(out)
            assert sr.same(out[:, some != 0], med[:, some != 0]) and sr.same(out[:, some == 0], block[:, some == 0])
            assert host(counts).tolist() == [int((some != 0).sum())] * 3
        check(mg, block, k, "both", threshold, med, dtype.__name__, defects=some)


# ---- votes -----------------------------------------------------------------------------------------------------------

def test_votes_of_known_specks(mg):
    tile = mg.despeckle.TILE
    h, w = tile + 6, tile + 9
    rng = np.random.default_rng(46)
    block = (1000 + rng.integers(0, 8, size=(5, h, w))).astype(np.uint16)
    specks = {(0, 0): [0, 1, 2, 3, 4], (3, 4): [0, 2, 4], (tile - 1, tile): [1, 3], (tile, tile - 1): [2],
              (h - 1, w - 1): [0, 1, 2], (20, 20): [0, 1, 2, 3]}
    table = np.zeros((h, w), dtype=np.int32)
    for (y, x), planes in specks.items():
        block[planes, y, x] = 9000
        table[y, x] = len(planes)
    for k in (1, 2):
        got = mg.despeckle.outlier_votes(dev(block), 500, k, "bright")
        assert got.dtype == torch.int32 and tuple(got.shape) == (h, w)
        np.testing.assert_array_equal(host(got), table)
        np.testing.assert_array_equal(host(got), sr.votes(block, k, "bright", 500))
        assert host(mg.despeckle.outlier_votes(dev(block), 500, k, "dark")).sum() == 0
        for fraction, need in ((0.5, 3), (1.0, 5), (0.2, 1)):
            got = mg.despeckle.defect_map(dev(block), 500, k, "bright", fraction)
            assert got.dtype == torch.bool
            np.testing.assert_array_equal(host(got), table >= need)
            np.testing.assert_array_equal(host(got), sr.defect_map(block, k, "bright", 500, fraction))
        one = mg.despeckle.outlier_votes(dev(block[3:4]), 500, k, "bright")  # n = 1
        np.testing.assert_array_equal(host(one), sr.votes(block[3:4], k, "bright", 500))
        assert host(one).sum() == 3
    lead = dev(block[:4].reshape(2, 2, h, w))  # every leading dimension counts planes
    np.testing.assert_array_equal(host(mg.despeckle.outlier_votes(lead, 500)), sr.votes(block[:4], 1, "bright", 500))


@pytest.mark.parametrize("dtype", DTYPES)
def test_votes_of_random_planes(mg, dtype):
    rng = np.random.default_rng(47)
    tile = mg.despeckle.TILE
    for n, h, w in ((4, 3, 5), (6, tile + 1, 2 * tile + 5)):
        block, threshold = sr.random_planes(rng, dtype, (n, h, w), specks=0.05)
        for k in (1, 2):
            med = sr.median(block, k)
            for which in TESTS:
                got = host(mg.despeckle.outlier_votes(dev(block), 0.6 * threshold, k, which))
                np.testing.assert_array_equal(got, sr.votes(block, k, which, 0.6 * threshold, med))
    # the entry zeroes its table itself: a buffer full of sevens comes back as the votes
    nat = mg.hotpath.nat
    d, dirty = dev(block), torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    assert nat.lib().mg_outlier_votes(d.data_ptr(), nat.dtype_code(d.dtype), n, h, w, 1, 2, float(threshold), dirty.data_ptr(),
                                      mg.hotpath._stream()) == 0
    np.testing.assert_array_equal(host(dirty), sr.votes(block, 1, "both", threshold))


# ---- large indices ---------------------------------------------------------------------------------------------------

def test_more_planes_than_a_grid_dimension(mg):
    gen = torch.Generator(device="cuda").manual_seed(5)
    block = torch.randint(0, 256, (70_000, 3, 3), dtype=torch.uint8, device="cuda", generator=gen)
    on_host = host(block)
    for k, which in ((1, "both"), (2, "bright")):
        want, want_counts = sr.remove(on_host, k, which, 20.5)
        out, counts = mg.despeckle.remove_outliers(block, 20.5, k, which)
        assert np.array_equal(host(out), want)
        np.testing.assert_array_equal(host(counts), want_counts)
        assert want_counts[-1000:].sum() > 0
    votes = mg.despeckle.outlier_votes(block, 20.5, 1, "both")
    np.testing.assert_array_equal(host(votes), sr.votes(on_host, 1, "both", 20.5))


def test_a_block_above_two_to_the_31_pixels(mg):
    n, size = 129, 4096
    assert n * size * size > 2 ** 31
    gen = torch.Generator(device="cuda").manual_seed(6)
    block = torch.randint(0, 256, (n, size, size), dtype=torch.uint8, device="cuda", generator=gen)
    out, counts = mg.despeckle.remove_outliers(block, 60.5, 1, "both")
    for i in (0, n - 1):
        plane = host(block[i])
        want, want_count = sr.remove(plane, 1, "both", 60.5, med=sr.median_banded(plane, 1))
        assert np.array_equal(host(out[i]), want), i
        assert int(counts[i].item()) == int(want_count) > 0, i
    assert int(counts.min().item()) > 0
    del block, out
    torch.cuda.empty_cache()


# ---- refusals and empties --------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(mg, monkeypatch):
    calls = []
    real = mg.hotpath._call
    monkeypatch.setattr(mg.hotpath, "_call", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    ds = mg.despeckle
    good = torch.zeros((2, 8, 9), dtype=torch.uint8, device="cuda")
    for fn in (lambda: ds.remove_outliers(good, -1), lambda: ds.remove_outliers(good, float("nan")),
               lambda: ds.remove_outliers(good, float("inf")), lambda: ds.remove_outliers(good, True),
               lambda: ds.remove_outliers(good, 5, 0), lambda: ds.remove_outliers(good, 5, 3),
               lambda: ds.remove_outliers(good, 5, 1, "all"), lambda: ds.remove_outliers(good, 5, 1, "hot"),
               lambda: ds.outlier_votes(good, 5, 1, "all"), lambda: ds.outlier_votes(good, -5),
               lambda: ds.defect_map(good, 5, 1, "bright", 0), lambda: ds.defect_map(good, 5, 1, "bright", 1.5),
               lambda: ds.median(good, 3), lambda: ds.median(good[0, 0]), lambda: ds.remove_outliers(good.cpu(), 5),
               lambda: ds.outlier_votes(good.cpu(), 5), lambda: ds.median(good.cpu()),
               lambda: ds.remove_outliers(good, 5, defects=np.zeros((9, 8), bool)),
               lambda: ds.remove_outliers(good, 5, defects=torch.zeros((2, 8, 9), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: ds.remove_outliers(good.to(torch.int32), 5), lambda: ds.median(good.to(torch.float16)),
               lambda: ds.outlier_votes(good.to(torch.int64), 5), lambda: ds.remove_outliers(np.zeros((2, 8, 9), np.uint8), 5),
               lambda: ds.remove_outliers(good, 5, defects=np.zeros((8, 9), np.float32))):
        with pytest.raises(TypeError):
            fn()
    # zero-size blocks give empty results
    for shape in ((2, 0, 8), (2, 8, 0), (0, 5, 5)):
        empty = torch.zeros(shape, dtype=torch.uint16, device="cuda")
        out, counts = ds.remove_outliers(empty, 5)
        assert tuple(out.shape) == shape and host(counts).tolist() == [0] * shape[0] and counts.dtype == torch.int64
        assert tuple(ds.median(empty, 2).shape) == shape
        votes = ds.outlier_votes(empty, 5)
        assert tuple(votes.shape) == shape[1:] and int(votes.sum().item()) == 0
    assert calls == []
    # the C entry points say MG_EINVAL themselves, and MG_OK with nothing written for an empty block
    nat = mg.hotpath.nat
    lib, s, u8 = nat.lib(), mg.hotpath._stream(), nat.MG_U8
    src, dst = good.data_ptr(), torch.full((2, 8, 9), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), 9, dtype=torch.int64, device="cuda")
    votes = torch.full((8, 9), 9, dtype=torch.int32, device="cuda")
    dmap = torch.ones((8, 9), dtype=torch.uint8, device="cuda")
    nan = float("nan")

    def planes(dtype=u8, n=2, h=8, w=9, k=1, which=0, threshold=1.0, defects=0, to=None):
        return lib.mg_despeckle_planes(src, dst.data_ptr() if to is None else to, dtype, n, h, w, k, which, threshold, defects,
                                       counts.data_ptr(), s)

    for bad in (dict(dtype=99), dict(which=4), dict(which=-1), dict(k=0), dict(k=3), dict(threshold=-1.0), dict(threshold=nan),
                dict(to=src), dict(to=0), dict(n=-1), dict(h=-1), dict(which=4, defects=dmap.data_ptr())):
        assert planes(**bad) == -1, bad
    assert lib.mg_outlier_votes(src, u8, 2, 8, 9, 1, 3, 1.0, votes.data_ptr(), s) == -1  # ALL has no votes
    assert lib.mg_outlier_votes(src, u8, 2, 8, 9, 1, 0, -1.0, votes.data_ptr(), s) == -1
    assert lib.mg_outlier_votes(src, u8, 2, 8, 9, 3, 0, 1.0, votes.data_ptr(), s) == -1
    assert lib.mg_outlier_votes(src, u8, 2, 8, 9, 1, 0, 1.0, 0, s) == -1
    for empty in (dict(n=0), dict(h=0), dict(w=0)):
        assert planes(**empty) == 0, empty
    assert lib.mg_outlier_votes(src, u8, 0, 8, 9, 1, 0, 1.0, votes.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (host(dst) == 9).all() and (host(counts) == 9).all() and (host(votes) == 9).all()
    # a threshold that plays no part may be anything; ALL counts every pixel; the entry zeroes the counts itself
    assert planes(which=3, threshold=-1.0) == 0
    assert host(counts).tolist() == [72, 72]
    assert planes(threshold=nan, defects=dmap.data_ptr()) == 0
    assert host(counts).tolist() == [72, 72] and (host(dst) == 0).all()


# ---- the component ---------------------------------------------------------------------------------------------------

HOT = [(50, 50), (50, 150), (150, 50), (150, 150), (30, 70), (70, 30)]  # in every 200 x 200 tile: background


@pytest.fixture(scope="module")
def chip_stack():
    """(clean, hot, transient position): a 3 x 3 chip cut into 2 x 2 tiles, two timepoints; six hot pixels at the same
    place in every tile plane and one speck in a single plane."""
    img = draw_chip((3, 3), 20, value=200)
    assert img.shape == (400, 400)
    tiles = img.reshape(2, 200, 2, 200).transpose(0, 2, 1, 3)
    clean = np.ascontiguousarray(np.stack([tiles, tiles])[None])  # (channel, time, tile_row, tile_col, tile_y, tile_x)
    hot = clean.copy()
    for y, x in HOT:
        assert (clean[..., y - 1:y + 2, x - 1:x + 2] == 0).all()
        hot[..., y, x] = 65535
    transient = (0, 1, 0, 1, 120, 40)
    assert (clean[transient[:4]][119:122, 39:42] == 0).all()
    hot[transient] = 65535
    return clean, hot, transient


DIMS = ("channel", "time", "tile_row", "tile_col", "tile_y", "tile_x")
CHIP = dict(shape=(3, 3), min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100, col_dist=100, num_iter=5000)


def test_sensor_scope_keeps_a_transient_speck(mg, chip_stack):
    clean, hot, transient = chip_stack
    planes = clean.size // (200 * 200)
    arr = mg.DataArray(hot, DIMS, coords={"channel": ["bf"]}, attrs={"name": "assay"})
    out = mg.components.get("remove_outliers")(threshold=1000, scope="sensor")(arr)
    assert isinstance(out, mg.DataArray) and out.dims == DIMS and list(out.coords["channel"].values) == ["bf"]
    assert out.attrs["name"] == "assay" and out.attrs["despeckle_defects"] == 6
    assert out.attrs["despeckle_replaced"] == 6 * planes
    want = clean.copy()
    want[transient] = 65535
    np.testing.assert_array_equal(out.values, want)
    out = mg.components.get("remove_outliers")(threshold=1000, scope="plane")(arr)
    assert out.attrs["despeckle_replaced"] == 6 * planes + 1 and "despeckle_defects" not in out.attrs
    np.testing.assert_array_equal(out.values, clean)
    # a Dataset keeps its other variables, coordinates, attributes and cache; the pages need not come last
    moved = np.ascontiguousarray(hot[0, 0, 0].transpose(1, 0, 2))  # (tile_y, tile_col, tile_x)
    ds = mg.Dataset({"tile": mg.DataArray(dev(moved), ("tile_y", "tile_col", "tile_x")),
                     "extra": mg.DataArray(np.arange(3), ("n",))}, coords={"tile_col": [10, 20]}, attrs={"name": "assay"})
    ds._cache["kept"] = 1
    got = mg.despeckle.remove_outliers_component(ds, 1000, radius=2, which="both")
    assert got.tile.dims == ("tile_y", "tile_col", "tile_x") and got.attrs["name"] == "assay" and got._cache["kept"] == 1
    assert list(got.coords["tile_col"].values) == [10, 20] and got.extra.values.tolist() == [0, 1, 2]
    assert got.attrs["despeckle_replaced"] == 12 and "despeckle_replaced" not in ds.attrs
    np.testing.assert_array_equal(got.tile.values, clean[0, 0, 0].transpose(1, 0, 2))


def test_chip_with_hot_pixels_equals_the_clean_chip(mg, chip_stack):
    clean, hot, _ = chip_stack
    mg.seed(4321)
    want = mg.microfluidic_chip(mg.DataArray(clean, DIMS), **CHIP)
    mg.seed(4321)
    got = mg.microfluidic_chip(mg.DataArray(hot, DIMS), despeckle=1000, **CHIP)
    assert got.attrs["despeckle_replaced"] == 49 and "despeckle_replaced" not in want.attrs
    assert want.sizes["mark_row"] == 3 and want.sizes["mark_col"] == 3 and want.sizes["time"] == 2
    for name in ("x", "y", "fg", "bg"):
        np.testing.assert_array_equal(got[name].values, want[name].values, err_msg=name)
    np.testing.assert_array_equal(got.roi.values, want.roi.values)
    mg.seed(4321)
    got = mg.microfluidic_chip(mg.DataArray(hot, DIMS), despeckle=1000, despeckle_scope="sensor", **CHIP)
    assert got.attrs["despeckle_replaced"] == 48 and got.attrs["despeckle_defects"] == 6


# ---- end to end, beads -----------------------------------------------------------------------------------------------

CENTRES = [[y, x] for y in (70, 190, 310, 430) for x in (100, 256, 412)]
SPECKS = [(10, 10), (130, 40), (130, 180), (250, 330), (250, 180), (370, 40), (370, 330), (490, 256), (20, 500), (130, 470),
          (250, 490), (500, 20), (370, 480), (130, 330), (250, 30), (10, 256), (490, 100), (490, 412), (130, 256), (310, 180)]
BEADS = dict(min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=20000)


def marks(xp):
    n = xp.roi.sizes["mark"]
    if n == 0:
        return np.zeros(0), np.zeros(0)
    return xp.y.values.reshape(n, -1)[:, 0].astype(np.float64), xp.x.values.reshape(n, -1)[:, 0].astype(np.float64)


def test_beads_below_a_hot_pixel_are_found_again(mg):
    clean = draw_beads((512, 512), CENTRES, 20, value=200)
    hot = clean.copy()
    assert len(SPECKS) == 20 and len(CENTRES) == 12
    for y, x in SPECKS:  # background, at least 40 pixels from the rim of any bead
        assert min(np.hypot(y - cy, x - cx) for cy, cx in CENTRES) >= 50
        hot[y, x] = 65535
    out, counts = mg.despeckle.remove_outliers(dev(hot), 1000)
    assert np.array_equal(host(out), clean) and int(counts.item()) == 20
    mg.seed(1234)
    want = mg.beads(mg.DataArray(clean, ("y", "x")), **BEADS)
    mg.seed(1234)
    got = mg.beads(mg.DataArray(hot, ("y", "x")), despeckle=1000, **BEADS)
    assert want.roi.sizes["mark"] == got.roi.sizes["mark"] == 12
    assert got.attrs["despeckle_replaced"] == 20
    np.testing.assert_array_equal(got.x.values, want.x.values)
    np.testing.assert_array_equal(got.y.values, want.y.values)
    np.testing.assert_array_equal(got.fg.sum(dim=["roi_x", "roi_y"]).values, want.fg.sum(dim=["roi_x", "roi_y"]).values)
    ys, xs = marks(want)
    for cy, cx in CENTRES:
        assert np.hypot(ys - cy, xs - cx).min() < 5
    # without it one pixel at 65535 sets the grey scale: floor(255 * 200 / 65535) = 0, every bead is gone
    mg.seed(1234)
    lost = mg.beads(mg.DataArray(hot, ("y", "x")), **BEADS)
    assert "despeckle_replaced" not in lost.attrs
    ys, xs = marks(lost)
    for cy, cx in CENTRES:
        assert len(ys) == 0 or np.hypot(ys - cy, xs - cx).min() > 10
