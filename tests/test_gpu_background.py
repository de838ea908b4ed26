"""Background subtraction on the device: mg_background_planes through ``magnify_amd.background``, equal by value to the
NumPy oracle (tests/background_ref.py; NaN equal to NaN) at every seam of the kernels, the refusals, the component and
``background=`` end to end."""

import numpy as np
import pytest
import torch

import background_ref as br
import despeckle_ref as sr
from synth import draw_beads

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
RADII = [1, 2, 7, 32, 128]
MAX_H, MAX_W = 300, 400  # the largest plane of the seam tests


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


def random_planes(rng, dtype, shape):
    """Noise over the whole range of the integers; floats around -100, so there are negative values."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return rng.integers(0, int(top_of(dtype)) + 1, size=shape).astype(dtype)
    return rng.normal(-100.0, 50.0, size=shape).astype(dtype)


def check(mg, block, radius, smooth=0, label=None):
    """estimate and subtract of a host block (..., H, W) against the oracle.  -> (background, difference) of the oracle."""
    want_b = br.estimate(block, radius, smooth)
    want_d = br.minus(block, want_b)
    d = dev(block)
    got_b, got_d = host(mg.background.estimate(d, radius, smooth)), host(mg.background.subtract(d, radius, smooth))
    assert br.same(got_b, want_b), ("estimate", label, block.shape, radius, smooth)
    assert br.same(got_d, want_d), ("subtract", label, block.shape, radius, smooth)
    return want_b, want_d


def seam_shapes(mg, radius):
    """(h, w) pairs in which every seam size occurs as a height and as a width: the window's sizes and the sizes of the
    kernels' steps, one off either side.  Small against large, so that the oracle stays quick, and one plane of
    several steps both ways."""
    bg = mg.background
    sizes = {1, radius, radius + 1, 2 * radius, 2 * radius + 1, 2 * radius + 2, 4 * radius + 3,
             bg.COLS - 1, bg.COLS, bg.COLS + 1, bg.ROWS - 1, bg.ROWS, bg.ROWS + 1, 2 * bg.ROWS + 1,
             bg.SPAN - 1, bg.SPAN, bg.SPAN + 1}
    hs, ws = sorted(s for s in sizes if s <= MAX_H), sorted((s for s in sizes if s <= MAX_W), reverse=True)
    pairs = [(h, ws[i % len(ws)]) for i, h in enumerate(hs)] + [(hs[i % len(hs)], w) for i, w in enumerate(ws)]
    pairs += [(h, ws[(i + len(ws) // 2) % len(ws)]) for i, h in enumerate(hs)]  # and every height with a middling width
    return sorted(set(pairs)) + [(2 * bg.ROWS + 1, bg.SPAN + bg.COLS + 1)]


# ---- seams -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_planes_at_every_seam(mg, dtype, radius):
    rng = np.random.default_rng(51)
    shapes = seam_shapes(mg, radius)
    assert max(h for h, _ in shapes) <= MAX_H and max(w for _, w in shapes) <= MAX_W
    for h, w in shapes:
        n = 2 if h * w < 20000 else 1
        check(mg, random_planes(rng, dtype, (n, h, w)), radius, label=dtype.__name__)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_made_planes(mg, dtype, radius):
    bg = mg.background
    top = int(top_of(dtype)) if np.dtype(dtype).kind == "u" else 4096
    for h, w in ((1, 2 * radius + 2), (min(2 * radius + 1, MAX_H), 1), (bg.ROWS + 1, bg.COLS + 1),
                 (min(4 * radius + 3, 2 * bg.ROWS + 1), min(4 * radius + 3, bg.SPAN + 1))):
        cy, cx = h // 2, (2 * w) // 3
        flat = np.full((h, w), top // 2, dtype=dtype)
        bright, dark = flat.copy(), flat.copy()
        bright[cy, cx], dark[cy, cx] = top, 3
        yy, xx = np.mgrid[0:h, 0:w]
        ramp = ((yy * 3 + xx * 2) % (top + 1)).astype(dtype)  # monotone down and across (uint8: until its range ends)
        block = np.stack([flat, bright, dark, ramp, ramp[::-1, ::-1]])
        want_b, want_d = check(mg, block, radius, label=dtype.__name__)
        assert br.same(want_b[0], flat) and not want_d[0].any()
        if h > 1 or w > 1:
            assert br.same(want_b[1], flat) and want_d[1].sum() == top - top // 2  # the bright pixel is all that is left
        assert want_b[2, cy, cx] == 3 and (want_b[2] <= dark).all()  # the dark one is background: it is still there
        if radius < cy < h - 1 - radius and radius < cx < w - 1 - radius:
            assert br.same(want_b[2], dark) and not want_d[2].any()  # and nowhere else, where no border cuts its windows
        if dtype is not np.uint8:  # a ramp is its own opening, but for the far edges, where the windows are cut
            assert not want_d[3][:max(h - radius, 0), :max(w - radius, 0)].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_plane_never_sees_its_neighbour_in_memory(mg, dtype):
    rng = np.random.default_rng(52)
    bg = mg.background
    top = top_of(dtype)
    for radius in (2, 32):
        for h, w in ((1, 1), (5, 7), (bg.ROWS + 3, bg.COLS + 1)):
            block = np.empty((3, h, w), dtype=dtype)
            block[0], block[2] = 0, top
            block[1] = random_planes(rng, dtype, (h, w))
            want_b, _ = check(mg, block, radius, label=dtype.__name__)
            assert (want_b[0] == 0).all() and (want_b[2] == top).all()
            check(mg, block[::-1], radius, label=dtype.__name__)


# ---- values ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_integer_extremes(mg, dtype):
    rng = np.random.default_rng(53)
    top = int(top_of(dtype))
    block = (rng.integers(0, 2, size=(2, 67, 131)) * top).astype(dtype)  # only 0 and the maximum
    block[1, 20:50, 30:100] = top  # a field of the maximum that the windows fit into
    for radius in (1, 2, 7):
        want_b, want_d = check(mg, block, radius, label=dtype.__name__)
        assert (want_b[1] == top).any() and (want_d == top).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_specials(mg, dtype):
    rng = np.random.default_rng(54)
    nan, inf = np.nan, np.inf
    block = rng.normal(-100.0, 50.0, size=(3, 70, 90)).astype(dtype)
    block[0, 5, 5] = nan              # a NaN pixel among numbers
    block[0, 10:13, 10:13] = nan      # an island smaller than the windows of radius 2 and 7, as large as that of radius 1
    block[0, 20:55, 30:65] = nan      # an island larger than every window: windows with nothing left
    block[0, 60, 8] = inf
    block[0, 62:69, 70:85] = inf      # a field of +inf
    block[0, 3, 80] = -inf
    block[1, 0, 0] = nan              # the corners
    block[1, 69, 89] = -inf
    block[1, 30:40, 30:60] = 0.0
    block[1, 30:40, 30:60:2] = -0.0   # +-0 side by side
    one = dtype(1.0)
    block[2] = one
    block[2, ::2, ::3] = np.nextafter(one, dtype(2.0))   # neighbours one ulp apart
    block[2, 1::4, 1::5] = np.nextafter(one, dtype(0.0))
    block[2, 40:60, 40:60] = np.nextafter(one, dtype(2.0))
    for radius in (1, 2, 7):
        want_b, want_d = check(mg, block, radius, label=dtype.__name__)
        assert np.isnan(want_b[0, 37, 47]) and not np.isnan(want_b[0, 5, 5]) and np.isnan(want_d[0, 5, 5])
        assert (want_b[0] == inf).any() == (radius <= 3) and (want_b[2, 45:55, 45:55] > one).all()
    for radius in (32, 128):  # wider than the plane: every window holds the numbers of the whole plane
        check(mg, block, radius, label=dtype.__name__)
    check(mg, np.full((2, 9, 70), nan, dtype=dtype), 2, label="all NaN")


@pytest.mark.parametrize("dtype", DTYPES)
def test_smoothing_and_the_clamp(mg, dtype):
    rng = np.random.default_rng(55)
    bg = mg.background
    for h, w in ((1, 1), (5, 70), (bg.ROWS + 1, bg.COLS + 9)):
        block = random_planes(rng, dtype, (2, h, w))
        for smooth in (1, 2):
            med = sr.median(block, smooth)
            for radius in (3, 32):
                want_b, want_d = check(mg, block, radius, smooth, label=dtype.__name__)
                assert br.same(want_b, br.opening(med, radius))
                if h * w > 1000 and radius == 3:
                    above = want_b > block  # the background of the median is above the pixel: the clamp
                    assert 0.1 < above.mean() < 0.6 and not want_d[above].any()
    lead = random_planes(rng, dtype, (2, 3, 9, 11))  # every leading dimension counts planes
    got = mg.background.subtract(dev(lead), 2, 1)
    assert tuple(got.shape) == lead.shape and br.same(host(got), br.subtract(lead, 2, 1))


# ---- large indices ---------------------------------------------------------------------------------------------------

def test_more_planes_than_a_grid_dimension(mg):
    gen = torch.Generator(device="cuda").manual_seed(5)
    block = torch.randint(0, 256, (70_000, 3, 5), dtype=torch.uint8, device="cuda", generator=gen)
    on_host = host(block)
    for radius, smooth in ((1, 0), (2, 1)):
        want = br.subtract(on_host, radius, smooth)
        assert np.array_equal(host(mg.background.subtract(block, radius, smooth)), want)
        assert want[-1000:].any()
    assert np.array_equal(host(mg.background.estimate(block, 1)), br.estimate(on_host, 1))


def test_a_block_above_two_to_the_31_pixels(mg):
    n, size, radius = 33, 8192, 3
    assert n * size * size > 2 ** 31
    gen = torch.Generator(device="cuda").manual_seed(6)
    block = torch.randint(0, 256, (n, size, size), dtype=torch.uint8, device="cuda", generator=gen)
    assert mg.background.SCRATCH_LIMIT // (2 * size * size) < n  # the block goes to the entry in several groups
    out = mg.background.subtract(block, radius)
    for i in (0, n // 2, n - 1):
        plane = host(block[i])
        want = br.minus(plane, br.opening_by_shifts(plane, radius))
        assert want.any() and np.array_equal(host(out[i]), want), i
    del block, out
    torch.cuda.empty_cache()


# ---- refusals and empties --------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(mg, monkeypatch):
    calls = []
    real = mg.hotpath._call
    monkeypatch.setattr(mg.hotpath, "_call", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    bg = mg.background
    good = torch.zeros((2, 8, 9), dtype=torch.uint8, device="cuda")
    for fn in (bg.estimate, bg.subtract):
        for bad in (lambda: fn(good, 0), lambda: fn(good, 129), lambda: fn(good, True), lambda: fn(good, 2.5),
                    lambda: fn(good, -1), lambda: fn(good, "4"), lambda: fn(good, 4, 3), lambda: fn(good, 4, -1),
                    lambda: fn(good, 4, True), lambda: fn(good, 4, 1.0), lambda: fn(good[0, 0], 4),
                    lambda: fn(good.cpu(), 4)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: fn(good.to(torch.int32), 4), lambda: fn(good.to(torch.float16), 4),
                    lambda: fn(np.zeros((2, 8, 9), np.uint8), 4)):
            with pytest.raises(TypeError):
                bad()
        for shape in ((2, 0, 8), (2, 8, 0), (0, 5, 5)):  # zero-size blocks give empty results
            assert tuple(fn(torch.zeros(shape, dtype=torch.uint16, device="cuda"), 4, 1).shape) == shape
    image = mg.DataArray(good, ("channel", "im_y", "im_x"), coords={"channel": ["bf", "cy5"]})
    for bad in (lambda: bg.subtract_background(image, 4, channel="egfp"), lambda: bg.subtract_background(image, 0),
                lambda: bg.subtract_background(mg.Dataset({"tile": image}), 4),
                lambda: bg.subtract_background(mg.DataArray(good, ("channel", "a", "b")), 4)):
        with pytest.raises(ValueError):
            bad()
    assert calls == []
    # the C entry points say MG_EINVAL themselves, and MG_OK with nothing written for an empty block
    nat = mg.hotpath.nat
    lib, s, u8 = nat.lib(), mg.hotpath._stream(), nat.MG_U8
    src, filt = good.data_ptr(), torch.zeros((2, 8, 9), dtype=torch.uint8, device="cuda")
    dst = torch.full((2, 8, 9), 9, dtype=torch.uint8, device="cuda")
    need = lib.mg_background_scratch_bytes(u8, 2, 8, 9, 4)
    assert need == 2 * 2 * 8 * 9 and lib.mg_background_scratch_bytes(nat.MG_F64, 3, 8, 9, 128) == 2 * 3 * 8 * 9 * 8
    scratch = torch.full((need + 16,), 9, dtype=torch.uint8, device="cuda")
    for bad in (dict(dtype=99), dict(n=-1), dict(h=-1), dict(w=-1), dict(h=(1 << 30) + 1), dict(w=(1 << 20) + 1),
                dict(radius=0), dict(radius=129), dict(n=1 << 62)):
        args = dict(dtype=u8, n=2, h=8, w=9, radius=4)
        args.update(bad)
        assert lib.mg_background_scratch_bytes(*args.values()) == -1, bad
    for empty in (dict(n=0), dict(h=0), dict(w=0)):
        args = dict(dtype=u8, n=2, h=8, w=9, radius=4)
        args.update(empty)
        assert lib.mg_background_scratch_bytes(*args.values()) == 0, empty

    def planes(dtype=u8, n=2, h=8, w=9, radius=4, mode=1, source=src, filtered=0, to=None, work=None, size=need):
        return lib.mg_background_planes(source, filtered, dst.data_ptr() if to is None else to, dtype, n, h, w, radius, mode,
                                        scratch.data_ptr() if work is None else work, size, s)

    for bad in (dict(dtype=99), dict(mode=2), dict(mode=-1), dict(radius=0), dict(radius=129), dict(n=-1), dict(h=-1), dict(w=-1),
                dict(h=(1 << 30) + 1), dict(w=(1 << 20) + 1), dict(source=0), dict(to=0), dict(to=src), dict(work=0),
                dict(size=need - 1), dict(size=-1), dict(filtered=filt.data_ptr(), to=filt.data_ptr()), dict(work=src),
                dict(work=dst.data_ptr()), dict(dtype=nat.MG_U16, n=1, h=4, w=9, source=src + 1),
                dict(dtype=nat.MG_U16, n=1, h=4, w=9, work=scratch.data_ptr() + 1),
                dict(dtype=nat.MG_F32, n=1, h=2, w=9, to=dst.data_ptr() + 2),
                dict(dtype=nat.MG_U16, n=1, h=4, w=9, filtered=filt.data_ptr() + 1)):
        assert planes(**bad) == -1, bad
    for empty in (dict(n=0), dict(h=0), dict(w=0), dict(n=0, work=0, size=0)):
        assert planes(**empty) == 0, empty
    torch.cuda.synchronize()
    assert (host(dst) == 9).all() and (host(scratch) == 9).all()
    assert planes(filtered=filt.data_ptr(), size=need + 16) == 0  # more scratch than needed is fine
    torch.cuda.synchronize()
    assert (host(dst) == 0).all() and (host(scratch)[need:] == 9).all()


# ---- the component ---------------------------------------------------------------------------------------------------

def test_component_leaves_the_other_channels_alone(mg):
    rng = np.random.default_rng(56)
    image = random_planes(rng, np.uint16, (3, 2, 70, 90))
    ds = mg.Dataset({"image": mg.DataArray(dev(image), ("channel", "time", "im_y", "im_x")),
                     "extra": mg.DataArray(np.arange(3), ("n",))}, coords={"channel": ["bf", "cy5", "egfp"]},
                    attrs={"name": "assay"})
    ds._cache["kept"] = 1
    got = mg.components.get("subtract_background")(radius=5, channel="cy5")(ds)
    assert got.image.dims == ("channel", "time", "im_y", "im_x") and got.attrs["name"] == "assay" and got._cache["kept"] == 1
    assert got.attrs["background_radius"] == 5 and "background_radius" not in ds.attrs
    assert list(got.coords["channel"].values) == ["bf", "cy5", "egfp"] and got.extra.values.tolist() == [0, 1, 2]
    want = image.copy()
    want[1] = br.subtract(image[1], 5)
    np.testing.assert_array_equal(got.image.values, want)
    assert (want[1] != image[1]).any()
    np.testing.assert_array_equal(ds.image.values, image)  # the dataset that came in is as it was
    got = mg.background.subtract_background(ds, 5, smooth=1, channel=["egfp", "bf"])
    want = image.copy()
    want[[0, 2]] = br.subtract(image[[0, 2]], 5, 1)
    np.testing.assert_array_equal(got.image.values, want)
    np.testing.assert_array_equal(mg.background.subtract_background(ds, 5).image.values, br.subtract(image, 5))
    # a DataArray, the pages not last, a host array: every other dimension counts planes
    moved = np.ascontiguousarray(image[0].transpose(1, 0, 2))  # (y, time, x)
    arr = mg.DataArray(moved, ("y", "time", "x"), coords={"time": [10, 20]}, attrs={"name": "assay"})
    got = mg.background.subtract_background(arr, 5)
    assert isinstance(got, mg.DataArray) and got.dims == ("y", "time", "x") and list(got.coords["time"].values) == [10, 20]
    assert got.attrs == {"name": "assay", "background_radius": 5}
    np.testing.assert_array_equal(got.values, br.subtract(image[0], 5).transpose(1, 0, 2))


def test_image_pipeline_subtracts_after_the_stitch(mg):
    rng = np.random.default_rng(57)
    tiles = rng.integers(1000, 60000, size=(2, 2, 40, 50)).astype(np.uint16)
    data = mg.DataArray(data=tiles, dims=("row", "col", "y", "x"))
    plain = mg.image(data, overlap=6)
    assert "background_radius" not in plain.attrs
    got = mg.image(data, overlap=6, background=8)
    assert got.attrs["background_radius"] == 8 and got["image"].values.shape == plain["image"].values.shape == (68, 88)
    want = host(mg.background.subtract(dev(plain["image"].values), 8))
    np.testing.assert_array_equal(got["image"].values, want)
    np.testing.assert_array_equal(want, br.subtract(plain["image"].values, 8))
    assert (want != plain["image"].values).any()


# ---- end to end, beads -----------------------------------------------------------------------------------------------

CENTRES = [[y, x] for y in (70, 190, 310, 430) for x in (100, 256, 412)]  # 40 pixels and more from the borders and each other
BEADS = dict(min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=20000)
RADIUS = 16


def marks(xp):
    n = xp.roi.sizes["mark"]
    if n == 0:
        return np.zeros(0), np.zeros(0)
    return xp.y.values.reshape(n, -1)[:, 0].astype(np.float64), xp.x.values.reshape(n, -1)[:, 0].astype(np.float64)


def found(xp):
    ys, xs = marks(xp)
    return sum(1 for cy, cx in CENTRES if len(ys) and np.hypot(ys - cy, xs - cx).min() < 5)


def test_beads_on_a_ramp_are_found_again(mg):
    """Twelve disks of radius 10 and value 200 on 100 * clip(x, 0, W - 1 - 16): a background of up to 49 500 counts that
    varies along x only and is flat over the last 16 columns, so that P - B is the clean image exactly (checked with
    the oracle; the CPU restatement of the finder, oracle/ref_pipeline.py find_beads with these settings, finds all
    twelve beads in the clean image and none in the ramp, whose beads are 255 * 200 / 49 500 = 1 grey level)."""
    size = 512
    clean = draw_beads((size, size), CENTRES, 20, value=200)
    ramp = clean + (100 * np.clip(np.arange(size), 0, size - 1 - RADIUS)).astype(np.uint16)[None, :]
    assert ramp.dtype == np.uint16 and ramp.max() == 49500 and len(CENTRES) == 12
    assert np.array_equal(br.subtract(ramp, RADIUS), clean)
    assert np.array_equal(host(mg.background.subtract(dev(ramp), RADIUS)), clean)
    mg.seed(1234)
    want = mg.beads(mg.DataArray(clean, ("y", "x")), **BEADS)
    mg.seed(1234)
    got = mg.beads(mg.DataArray(ramp, ("y", "x")), background=RADIUS, **BEADS)
    assert want.roi.sizes["mark"] == got.roi.sizes["mark"] == 12
    assert got.attrs["background_radius"] == RADIUS and "background_radius" not in want.attrs
    np.testing.assert_array_equal(got.x.values, want.x.values)
    np.testing.assert_array_equal(got.y.values, want.y.values)
    np.testing.assert_array_equal(got.fg.sum(dim=["roi_x", "roi_y"]).values, want.fg.sum(dim=["roi_x", "roi_y"]).values)
    assert found(want) == found(got) == 12
    # without it the ramp takes the grey scale: the beads are about one grey level above it
    mg.seed(1234)
    lost = mg.beads(mg.DataArray(ramp, ("y", "x")), **BEADS)
    assert "background_radius" not in lost.attrs
    assert found(lost) < 12
