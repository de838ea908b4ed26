"""Depth stacks on the device: mg_depth_project / mg_depth_focus_totals / mg_depth_fuse through ``magnify_amd.depth``,
bit for bit against the NumPy oracle (tests/depth_ref.py) unless stated, the refusals, and ``depth=`` end to end."""

import numpy as np
import pytest
import torch

import depth_ref as dr
from synth import draw_beads
from tiffwrite import ome_xml, write_tiff

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


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


def check_project(mg, block, label):
    """max / mean / pick of a host block (N, Z, H, W) against the oracle."""
    n, z = block.shape[:2]
    d = dev(block)
    picks = np.array([(3 * i + 1) % z for i in range(n)])
    want = {"max": np.stack(dr.over_stacks(dr.project_max, block)), "mean": np.stack(dr.over_stacks(dr.project_mean, block)),
            "pick": np.stack([dr.project_pick(s, p) for s, p in zip(block, picks)])}
    for method in ("max", "mean", "pick"):
        got = host(mg.depth.project(d, method, picks if method == "pick" else None))
        assert dr.same(got, want[method]), (label, method)


# ---- project ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_project_shapes(mg, dtype):
    rng = np.random.default_rng(11)
    for z in (1, 2, 3, 7):
        for h, w in ((1, 1), (3, 5), (37, 53), (64, 257)):
            for n in (1, 3):
                check_project(mg, dr.random_stack(rng, dtype, (n, z, h, w)), (dtype.__name__, n, z, h, w))


def test_project_integer_means_and_the_top_of_the_range(mg):
    # Z = 2: 1.5 -> 2 and 2.5 -> 2; Z = 4: sums 2, 6, 10 -> 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    for dtype in (np.uint8, np.uint16):
        two = np.array([[[[1, 2, 0, 255]], [[2, 3, 1, 255]]]], dtype=dtype)
        assert host(mg.depth.project(dev(two), "mean")).tolist() == [[[2, 2, 0, 255]]]
        four = np.array([[[[1, 2, 3]], [[1, 2, 3]], [[0, 1, 2]], [[0, 1, 2]]]], dtype=dtype)
        assert host(mg.depth.project(dev(four), "mean")).tolist() == [[[0, 2, 2]]]
        check_project(mg, two, "two")
        check_project(mg, four, "four")
    full = np.full((2, 255, 5, 7), 65535, dtype=np.uint16)
    full[1, 100, 2, 3] = 0
    check_project(mg, full, "u16 at 65535, Z = 255")
    assert host(mg.depth.project(dev(full), "mean"))[0].min() == 65535


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_project_float_specials(mg, dtype):
    rng = np.random.default_rng(12)
    block = dr.random_stack(rng, dtype, (3, 5, 9, 11)) - 30000
    block[0, 1, 2, 3] = np.nan
    block[0, 0, 4, 4] = np.nan
    block[1, 4, 0, 0] = np.nan
    block[1, 2, 1, 1], block[1, 3, 1, 2] = np.inf, -np.inf
    block[2, 0, 3, 3], block[2, 3, 3, 3] = np.inf, -np.inf  # both in one pixel: the mean is NaN
    block[:, :, 8, 10] = [-0.0, 0.0, -0.0, 0.0, -0.0]
    block[:, :, 8, 9] = -0.0
    block[:, :, 8, 8] = [0.0, -0.0, -0.0, 0.0, 0.0]
    check_project(mg, block, dtype.__name__)
    got = host(mg.depth.project(dev(block), "max"))
    assert np.isnan(got[0, 2, 3]) and np.isnan(got[0, 4, 4]) and np.isnan(got[1, 0, 0])
    assert np.signbit(got[0, 8, 10]) and np.signbit(got[0, 8, 9]) and not np.signbit(got[0, 8, 8])


@pytest.mark.parametrize("dtype", DTYPES)
def test_project_and_fuse_of_an_offset_view(mg, dtype):
    """A stack that starts 3 elements into a larger allocation: for uint8 / uint16 no slice starts on a dword."""
    rng = np.random.default_rng(13)
    block = dr.random_stack(rng, dtype, (2, 3, 7, 9))
    big = np.zeros(block.size + 8, dtype=dtype)
    big[3:3 + block.size] = block.ravel()
    view = dev(big)[3:3 + block.size].view(block.shape)
    assert view.data_ptr() % 4 != 0 or np.dtype(dtype).itemsize >= 4
    for method, fn in (("max", dr.project_max), ("mean", dr.project_mean)):
        assert dr.same(host(mg.depth.project(view, method)), np.stack(dr.over_stacks(fn, block))), method
    image, index = mg.depth.fuse(view, 3)
    want = dr.over_stacks(dr.fuse, block, 1)
    assert dr.same(host(image), np.stack([w[0] for w in want]))
    assert np.array_equal(host(index), np.stack([w[1] for w in want]))
    if dr.is_int(block):
        np.testing.assert_array_equal(host(mg.depth.focus_totals(view)), np.stack(dr.over_stacks(dr.focus_totals, block)))


# ---- fuse ------------------------------------------------------------------------------------------------------------

def check_fuse(mg, block, k, label):
    image, index = mg.depth.fuse(dev(block), 2 * k + 1)
    want = dr.over_stacks(dr.fuse, block, k)
    assert index.dtype == torch.uint8 and image.shape == index.shape == block.shape[:1] + block.shape[2:]
    assert np.array_equal(host(index), np.stack([w[1] for w in want])), label
    assert dr.same(host(image), np.stack([w[0] for w in want])), label


def fuse_planes(tile):
    return [(2, 5), (1, 1), (tile - 1, tile), (tile, tile), (tile + 1, tile), (tile, tile - 1), (tile, tile + 1),
            (2 * tile + 5, 3 * tile + 7)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fuse_windows_and_tile_edges(mg, dtype):
    rng = np.random.default_rng(21)
    tile = mg.depth.TILE
    for k in (1, 4, 15):
        for h, w in fuse_planes(tile):
            check_fuse(mg, dr.random_stack(rng, dtype, (2, 5, h, w)), k, (dtype.__name__, k, h, w))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fuse_depths(mg, dtype):
    rng = np.random.default_rng(22)
    tile = mg.depth.TILE
    for z, k, (h, w) in ((1, 4, (tile + 1, tile + 3)), (2, 1, (2, 5)), (2, 15, (tile + 1, tile - 1)), (255, 4, (tile + 3, tile + 1)),
                         (255, 1, (1, 1))):
        check_fuse(mg, dr.random_stack(rng, dtype, (1 if z == 255 else 3, z, h, w)), k, (dtype.__name__, z, k, h, w))


def test_fuse_checkerboard_at_the_uint32_bound(mg):
    yy, xx = np.mgrid[0:40, 0:45]
    board = (((yy + xx) & 1) * 65535).astype(np.uint16)
    block = np.stack([np.full_like(board, 7), board, board[::-1].copy()])[None]
    assert int(dr.window_measure(board, 15).max()) == 251_916_540
    check_fuse(mg, block, 15, "checkerboard")
    _, index = mg.depth.fuse(dev(block), 31)
    assert (host(index) >= 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fuse_all_equal_slices_and_no_index(mg, dtype):
    rng = np.random.default_rng(23)
    plane = dr.random_stack(rng, dtype, (mg.depth.TILE + 2, mg.depth.TILE + 5))
    block = np.stack([plane] * 4)[None]
    image, index = mg.depth.fuse(dev(block), 9)
    assert (host(index) == 0).all() and dr.same(host(image)[0], plane)
    flat = np.full((1, 3, 9, 9), 5, dtype=dtype)  # every measure 0: ties to z = 0
    assert (host(mg.depth.fuse(dev(flat), 3)[1]) == 0).all()
    block = dr.random_stack(rng, dtype, (2, 3, 19, 45))
    image, none = mg.depth.fuse(dev(block), 5, want_index=False)
    assert none is None and dr.same(host(image), np.stack([w[0] for w in dr.over_stacks(dr.fuse, block, 2)]))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_fuse_sharp_region_crossing_a_tile_border(mg, dtype):
    """Slice z is a ramp (ML = 0) except for a noisy patch 10 columns wide that moves right by 14 columns per slice, in
    slice 2 across the border between the first two tiles; the index map follows it."""
    rng = np.random.default_rng(24)
    tile = mg.depth.TILE
    h, w, nz = tile + tile // 2, 2 * tile + 8, 5
    yy, xx = np.mgrid[0:h, 0:w]
    block = np.empty((1, nz, h, w), dtype=dtype)
    for z in range(nz):
        s = (1000 + 3 * yy + 2 * xx).astype(np.float64)
        x0 = tile - 30 + 14 * z
        s[4:h - 4, x0:x0 + 10] += rng.integers(0, 4000, size=(h - 8, 10))
        block[0, z] = s.astype(dtype)
    check_fuse(mg, block, 2, dtype.__name__)
    _, index = mg.depth.fuse(dev(block), 5)
    index = host(index)[0]
    for z in range(nz):
        x0 = tile - 30 + 14 * z
        assert (index[10:h - 10, x0 + 5] == z).all()  # a column that only slice z's patch reaches (with its window)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fuse_float_nan_slice(mg, dtype):
    rng = np.random.default_rng(25)
    block = dr.random_stack(rng, dtype, (2, 4, mg.depth.TILE + 3, mg.depth.TILE + 9))
    block[0, 0] = np.nan  # a NaN measure never wins, not even in slice 0
    block[1, 2] = np.nan
    block[1, 1, 5, 7] = np.nan  # and one NaN pixel poisons its neighbourhood only
    check_fuse(mg, block, 2, dtype.__name__)
    _, index = mg.depth.fuse(dev(block), 5)
    index = host(index)
    assert (index[0] != 0).all() and (index[1] != 2).all()


# ---- focus totals and sharpest ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_focus_totals_integers_exact(mg, dtype):
    rng = np.random.default_rng(31)
    for n, z, h, w in ((1, 1, 1, 1), (2, 3, 3, 5), (3, 2, 37, 53), (1, 3, 64, 257), (2, 2, 300, 700)):
        block = dr.random_stack(rng, dtype, (n, z, h, w))
        got = mg.depth.focus_totals(dev(block))
        assert got.dtype == torch.int64 and tuple(got.shape) == (n, z)
        np.testing.assert_array_equal(host(got), np.stack(dr.over_stacks(dr.focus_totals, block)))
    # the entry zeroes its totals itself: a buffer full of sevens comes back as the sums
    nat = mg.hotpath.nat
    d, dirty = dev(block), torch.full((n, z), 7, dtype=torch.int64, device="cuda")
    assert nat.lib().mg_depth_focus_totals(d.data_ptr(), nat.dtype_code(d.dtype), n, z, h, w, dirty.data_ptr(),
                                           mg.hotpath._stream()) == 0
    np.testing.assert_array_equal(host(dirty), np.stack(dr.over_stacks(dr.focus_totals, block)))
    top = np.zeros((1, 1, 64, 64), dtype=dtype)
    top[0, 0, ::2, ::2] = np.iinfo(dtype).max
    top[0, 0, 1::2, 1::2] = np.iinfo(dtype).max
    np.testing.assert_array_equal(host(mg.depth.focus_totals(dev(top))), np.stack(dr.over_stacks(dr.focus_totals, top)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_focus_totals_floats_within_1e12(mg, dtype):
    """At most 2^12 non-negative float64 terms per slice: any summation order is within 2^12 * 2^-53 < 1e-12 relative of
    the correctly rounded sum (math.fsum)."""
    rng = np.random.default_rng(32)
    for n, z, h, w in ((1, 1, 1, 1), (2, 3, 3, 5), (3, 2, 37, 53), (2, 4, 64, 64), (1, 2, 15, 257)):
        assert h * w <= 2 ** 12
        block = dr.random_stack(rng, dtype, (n, z, h, w))
        got = mg.depth.focus_totals(dev(block))
        assert got.dtype == torch.float64
        want = np.stack(dr.over_stacks(dr.focus_totals, block))
        got = host(got)
        print(dtype.__name__, (n, z, h, w), "max relative error", float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
        assert np.all(np.abs(got - want) <= 1e-12 * want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharpest_picks_the_oracles_slice(mg, dtype):
    rng = np.random.default_rng(33)
    h, w = 37, 53
    base = rng.random((h, w))
    # slice totals scale with the amplitude -- gaps far above the float tolerance.  Integer totals are exact, so equal
    # slices tie and the lowest z wins; float totals of equal slices may differ in the last bits (no defined order of
    # summation), so the float stacks have no ties
    if np.dtype(dtype).kind == "u":
        amps = {0: [1, 8, 3, 8, 2], 1: [5, 1, 2, 3, 4], 2: [2, 2, 2, 2, 2]}
    else:
        amps = {0: [1, 8, 3, 7, 2], 1: [5, 1, 2, 3, 4], 2: [6, 2, 5, 3, 4]}
    scale = 25 if np.dtype(dtype) == np.uint8 else 1000
    block = np.stack([np.stack([(base * a * scale).astype(dtype) for a in amps[i]]) for i in range(3)])
    totals = np.stack(dr.over_stacks(dr.focus_totals, block))
    want = [dr.first_argmax(t) for t in totals]
    assert want == [1, 0, 0]
    image, chosen = mg.depth.sharpest(dev(block))
    assert host(chosen).tolist() == want and chosen.dtype == torch.int32
    assert dr.same(host(image), np.stack([block[i, want[i]] for i in range(3)]))
    lead = dev(block.reshape(3, 1, 5, h, w))  # leading dimensions are kept
    image, chosen = mg.depth.sharpest(lead)
    assert tuple(image.shape) == (3, 1, h, w) and host(chosen).tolist() == [[1], [0], [0]]


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(mg, monkeypatch):
    calls = []
    real = mg.hotpath._call
    monkeypatch.setattr(mg.hotpath, "_call", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    good = torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device="cuda")
    empty = torch.zeros((2, 0, 8, 8), dtype=torch.uint8, device="cuda")
    for fn in (lambda: mg.depth.project(empty, "max"), lambda: mg.depth.focus_totals(empty), lambda: mg.depth.fuse(empty),
               lambda: mg.depth.sharpest(empty),
               lambda: mg.depth.fuse(torch.zeros((1, 256, 2, 2), dtype=torch.uint8, device="cuda")),
               lambda: mg.depth.fuse(good, 1), lambda: mg.depth.fuse(good, 33), lambda: mg.depth.fuse(good, 4),
               lambda: mg.depth.project(good, "pick", [0, 3]), lambda: mg.depth.project(good, "pick", [-1, 0]),
               lambda: mg.depth.project(good, "pick", [0]), lambda: mg.depth.project(good, "pick"),
               lambda: mg.depth.project(good, "median"), lambda: mg.depth.project(good[0, 0], "max")):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: mg.depth.project(good.to(torch.int32), "max"), lambda: mg.depth.fuse(good.to(torch.float16)),
               lambda: mg.depth.focus_totals(good.to(torch.int64)), lambda: mg.depth.project(np.zeros((2, 3, 8, 8), np.uint8), "max")):
        with pytest.raises(TypeError):
            fn()
    assert calls == []
    # the C entry points say MG_EINVAL themselves
    nat = mg.hotpath.nat
    lib, s, u8 = nat.lib(), mg.hotpath._stream(), nat.MG_U8
    out = torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    assert lib.mg_depth_fuse(good.data_ptr(), u8, 2, 3, 8, 8, 0, out.data_ptr(), 0, s) == -1
    assert lib.mg_depth_fuse(good.data_ptr(), u8, 2, 3, 8, 8, 16, out.data_ptr(), 0, s) == -1
    assert lib.mg_depth_fuse(good.data_ptr(), u8, 2, 256, 8, 8, 1, out.data_ptr(), 0, s) == -1
    assert lib.mg_depth_project(good.data_ptr(), out.data_ptr(), u8, 2, 0, 8, 8, 0, 0, s) == -1
    assert lib.mg_depth_project(good.data_ptr(), out.data_ptr(), u8, 2, 3, 8, 8, 2, 0, s) == -1  # pick without indices
    assert lib.mg_depth_project(good.data_ptr(), out.data_ptr(), 99, 2, 3, 8, 8, 0, 0, s) == -1
    assert lib.mg_depth_project(good.data_ptr(), out.data_ptr(), u8, 0, 3, 8, 8, 0, 0, s) == 0   # no stack: nothing to do
    assert lib.mg_depth_focus_totals(good.data_ptr(), u8, 2, 3, 8, 8, 0, s) == -1
    # an empty plane is legal
    assert tuple(mg.depth.project(torch.zeros((2, 3, 0, 8), dtype=torch.uint8, device="cuda"), "max").shape) == (2, 0, 8)
    assert host(mg.depth.focus_totals(torch.zeros((2, 3, 0, 8), dtype=torch.uint8, device="cuda"))).tolist() == [[0] * 3] * 2


# ---- end to end ------------------------------------------------------------------------------------------------------

def box_blur(img, r):
    """Mean over the (2r + 1)^2 box (edge-padded), on the host."""
    p = np.pad(img.astype(np.float64), r, mode="edge")
    acc = np.zeros(img.shape, dtype=np.float64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            acc += p[dy:dy + img.shape[0], dx:dx + img.shape[1]]
    return np.rint(acc / (2 * r + 1) ** 2).astype(img.dtype)


POS = [[120, 100], [300, 160], [420, 90], [200, 400], [380, 380]]  # two halves of a 512 x 512 scene


@pytest.fixture(scope="module")
def scene():
    """Five slices: the left half is sharp in slice 1, the right half in slice 3, everything else box-blurred."""
    sharp = draw_beads((512, 512), POS)
    blurred = {r: box_blur(sharp, r) for r in (3, 5, 7)}
    radius = {"left": [3, 0, 3, 5, 7], "right": [7, 5, 3, 0, 3]}
    stack = np.empty((5, 512, 512), dtype=np.uint16)
    for z in range(5):
        left = sharp if radius["left"][z] == 0 else blurred[radius["left"][z]]
        right = sharp if radius["right"][z] == 0 else blurred[radius["right"][z]]
        stack[z, :, :256], stack[z, :, 256:] = left[:, :256], right[:, 256:]
    return sharp, stack


BEADS = dict(min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=5000)


def found_positions(xp):
    n = xp.roi.sizes["mark"]  # (a single timepoint is squeezed away by restore_format)
    ys, xs = xp.y.values.reshape(n, -1)[:, 0], xp.x.values.reshape(n, -1)[:, 0]
    return sorted((int(round(float(y) / 10)), int(round(float(x) / 10))) for y, x in zip(ys, xs))


def test_beads_on_a_depth_stack(mg, scene):
    sharp, stack = scene
    want = sorted((int(round(p[0] / 10)), int(round(p[1] / 10))) for p in POS)
    for dims in (("depth", "y", "x"), ("z", "y", "x")):
        for method in ("focus", "max"):
            xp = mg.beads(mg.DataArray(stack, dims), depth=method, **BEADS)
            assert xp.roi.sizes["mark"] == len(POS), (method, dims)
            assert found_positions(xp) == want, (method, dims)
            assert "depth" not in xp.sizes and "z" not in xp.sizes and xp.sizes.get("time", 1) == 1
            assert xp.attrs["depth_method"] == method and "depth_chosen" not in xp.attrs
    # on the rim of every bead (a disk's edge within 2 pixels) the fused image is the sharp slice of that half
    image, index = mg.depth.fuse(dev(stack), 9)
    image, index = host(image), host(index)
    mixed = box_blur(sharp, 2)
    rim = (mixed > 0) & (mixed < 1000)
    assert rim[:, :256].sum() > 500 and rim[:, 256:].sum() > 300
    assert (index[:, :256][rim[:, :256]] == 1).all() and (index[:, 256:][rim[:, 256:]] == 3).all()
    np.testing.assert_array_equal(image[rim], sharp[rim])
    # without depth=: the slices land on time, as before
    pipe = mg.beads_pipe(**BEADS)
    assert [n for n, _ in pipe.components][0] == "standardize_format"
    pipe.remove_pipe("restore_format")  # (which would give the stacked dimension its name back)
    xq = pipe(mg.DataArray(stack, ("depth", "y", "x")))
    assert xq.sizes["time"] == 5 and "depth" not in xq.sizes and "depth_method" not in xq.attrs
    assert xq.roi.sizes["mark"] >= 1  # found in slice 0, as before


def test_sharpest_and_mean_through_the_component(mg, scene):
    _, stack = scene
    two = np.stack([stack, stack[::-1]])  # (channel, depth, y, x): the sharpest slice is counted per stack
    arr = mg.DataArray(two, ("channel", "depth", "y", "x"), coords={"channel": ["a", "b"]})
    out = mg.components.get("project_depth")(method="sharpest")(arr)
    totals = [dr.focus_totals(s) for s in two]
    want = [dr.first_argmax(t) for t in totals]
    assert out.attrs["depth_chosen"] == want and out.attrs["depth_method"] == "sharpest"
    assert out.dims == ("channel", "y", "x") and list(out.coords["channel"].values) == ["a", "b"]
    np.testing.assert_array_equal(out.values, np.stack([two[i, want[i]] for i in range(2)]))
    xp = mg.beads(arr, depth="sharpest", search_channel="a", **BEADS)
    assert xp.attrs["depth_chosen"] == want and xp.sizes["channel"] == 2 and "depth" not in xp.sizes
    # a Dataset with tile, depth not in front of the pages' other dimensions
    ds = mg.Dataset({"tile": mg.DataArray(two.transpose(1, 0, 2, 3), ("depth", "channel", "tile_y", "tile_x"))},
                    coords={"channel": ["a", "b"], "depth": [0.0, 0.5, 1.0, 1.5, 2.0]}, attrs={"name": "assay"})
    got = mg.depth.project_depth(ds, method="mean")
    assert got.tile.dims == ("channel", "tile_y", "tile_x") and "depth" not in got.coords and got.attrs["name"] == "assay"
    np.testing.assert_array_equal(got.tile.values, np.stack(dr.over_stacks(dr.project_mean, two)))


def test_image_from_an_ome_z_file_equals_the_array(mg, scene, tmp_path):
    _, stack = scene
    path = tmp_path / "focal.ome.tif"
    write_tiff(path, list(stack), bigtiff=True, description=ome_xml(size_z=5, size_y=512, size_x=512))
    from_file = mg.image(str(path), overlap=0, depth="max")
    from_array = mg.image(mg.DataArray(stack, ("depth", "y", "x")), overlap=0, depth="max")
    np.testing.assert_array_equal(from_file.image.values, from_array.image.values)
    np.testing.assert_array_equal(np.squeeze(from_file.image.values), dr.project_max(stack))
    assert "depth" not in from_file.sizes and from_file.attrs["depth_method"] == "max"
    with pytest.raises(ValueError, match="Z dimension"):
        mg.image(str(path), overlap=0)
