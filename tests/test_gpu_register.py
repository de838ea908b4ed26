"""``stitch(register="ncc")`` on the device against its NumPy restatement (tests/register_ref.py): the seam sums of
mg_seam_sums, the stitch of shifted tiles (shift with edge replication, then tests/blend_ref.py) and the component end
to end on tiles cut from one scene at jittered positions.

Tolerances.  Seam sums: integer pixels equal; float pixels |err| <= n * 2**-52 * sum|terms| per entry (any summation
order in float64; float32 products are exact in float64).  Registered stitch, as tests/test_gpu_blend.py: integers
equal, float64 8 * 2**-52 * max|contributing values|, float32 one ulp of the reference.

End to end (seeds picked with the restatement on the CPU): the scene of ``noisy_bead_image(1, ...)`` has one seam,
(1, 0) | (1, 1), that holds only a sliver of a bead; with independent noise per tile its best score is 0.49 (every other
seam: >= 0.99), so it falls just below ``min_score = 0.5`` and is left out -- the table is the expected one with or
without it.  With ``blend="linear"`` the image is the scene crop except where a band reads a pixel that the shift
replicated from the tile's edge (``_replicated``): those pixels are the restatement's, not the scene's."""
import numpy as np
import pytest

import blend_ref as br
import register_ref as rr
from synth import draw_beads, noisy_bead_image, random_bead_positions, vignette

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "uint16", "float32", "float64"]
CORRECTIONS = ["none", "flatfield", "shading"]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return magnify_amd


def _random_tiles(rng, dtype, shape):
    if np.dtype(dtype).kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    return rng.uniform(0.0, 4000.0, size=shape).astype(dtype)


# ---- a. seam sums ----------------------------------------------------------------------------------------------------


def _check_sums(planes, v, m, what):
    import torch

    from magnify_amd import register

    dev = torch.from_numpy(planes).cuda()
    sums, fixed = register.seam_sums(dev, v, m)
    again = register.seam_sums(dev, v, m)
    sums, fixed = sums.cpu().numpy(), fixed.cpu().numpy()
    assert sums.tobytes() == again[0].cpu().numpy().tobytes() and fixed.tobytes() == again[1].cpu().numpy().tobytes(), what
    integer = planes.dtype.kind == "u"
    assert sums.dtype == fixed.dtype == (np.int64 if integer else np.float64), what
    for p in range(planes.shape[0]):
        want_s, want_f, mag, fmag = rr.seam_sums(planes[p], v, m)
        assert sums[p].shape == want_s.shape and fixed[p].shape == want_f.shape, what
        if integer:
            np.testing.assert_array_equal(sums[p], want_s, err_msg=what)
            np.testing.assert_array_equal(fixed[p], want_f, err_msg=what)
        else:
            n = want_f[:, 0]
            np.testing.assert_array_equal(fixed[p][:, 0], n, err_msg=what)
            for got, want, scale, count in ((sums[p], want_s, mag, n[:, None, None, None]), (fixed[p], want_f, fmag, n[:, None])):
                bound = count * 2.0**-52 * scale
                err = np.abs(got - want)
                print(what, "plane", p, "max error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
                assert np.all(err <= bound), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_sums_equal_the_restatement(mg, dtype):
    rng = np.random.default_rng(DTYPES.index(dtype))
    for nr, nc in ((2, 2), (1, 3), (3, 1)):
        for v, m in ((8, 1), (9, 2), (16, 4)):
            _check_sums(_random_tiles(rng, dtype, (3, nr, nc, 40, 48)), v, m, f"{dtype} {nr}x{nc} v={v} m={m}")


@pytest.mark.parametrize("grid", [(1, 2, 1030, 40), (2, 1, 40, 1030)])
def test_seam_sums_of_a_patch_longer_than_a_strip(mg, grid):
    """The long side of the patch, 1022, is eight strips of a workgroup (128) less two positions."""
    nr, nc, ty, tx = grid
    _check_sums(_random_tiles(np.random.default_rng(7), "uint16", (1, nr, nc, ty, tx)), 16, 4, f"long {grid}")


# ---- b. registered stitch --------------------------------------------------------------------------------------------


def _fields(rng, corr, c, ty, tx):
    if corr == "flatfield":
        return rng.uniform(0.6, 1.4, size=(ty, tx)).astype(np.float32), 7.0
    if corr == "shading":
        return (rng.uniform(0.6, 1.4, size=(c, ty, tx)).astype(np.float32),
                rng.uniform(0.0, 20.0, size=(c, ty, tx)).astype(np.float32))
    return None, None


def _tables(rng, n_tables, nr, nc, clip):
    """Shift tables within [-clip, clip] that hold both extremes on both axes."""
    t = rng.integers(-clip, clip + 1, size=(n_tables, nr, nc, 2))
    flat = t.reshape(n_tables, -1, 2)
    flat[:, 0, :] = clip
    flat[:, -1, :] = -clip
    if nr * nc > 2:
        flat[:, 1, :] = (clip, -clip)
    return t.astype(np.int32)


class _Stitched:
    """The device side of one (tiles, correction): the per-tile values of the plain path (overlap 0 tile by tile, as
    tests/test_gpu_blend.py::_run takes them) and the stitch with any shifts / blend."""

    def __init__(self, tiles, corr, flat, dark):
        import torch

        from magnify_amd import hotpath, shading

        self.hotpath, self.shading, self.corr, self.flat, self.dark = hotpath, shading, corr, flat, dark
        c, t, nr, nc, ty, tx = tiles.shape
        self.dev = torch.from_numpy(tiles).cuda()
        if corr == "none":
            self.values = tiles
        elif corr == "flatfield":
            self.max2 = hotpath.flatfield_max(self.dev, flat, dark)
            per_tile, _ = hotpath.flatfield_stitch(self.dev.reshape(c * t * nr * nc, 1, 1, 1, ty, tx), 0, flat, dark,
                                                   max2=self.max2, want_minmax=False)
            self.values = per_tile.reshape(tiles.shape).cpu().numpy()
        else:
            self.fl, self.dk = torch.from_numpy(flat).cuda(), torch.from_numpy(dark).cuda()
            per_tile, _ = shading.apply_stitch(self.dev.reshape(c, t * nr * nc, 1, 1, ty, tx), 0, self.fl, self.dk,
                                               want_minmax=False)
            self.values = per_tile.reshape(tiles.shape).cpu().numpy()

    def stitch(self, v, blend=None, **kw):
        if self.corr == "none":
            image, minmax = self.hotpath.flatfield_stitch(self.dev, v, apply_flatfield=False, blend=blend, **kw)
        elif self.corr == "flatfield":
            image, minmax = self.hotpath.flatfield_stitch(self.dev, v, self.flat, self.dark, max2=self.max2, blend=blend, **kw)
        else:
            image, minmax = self.shading.apply_stitch(self.dev, v, self.fl, self.dk, blend=blend, **kw)
        return image.cpu().numpy(), minmax.cpu().numpy()


def _want(values, v, tables, blend):
    """Shift-then-blend_ref, table 0 for every plane or table t for timepoint t; and the moved tiles."""
    n_time = values.shape[1]
    moved = np.stack([rr.shift_tiles(values[:, t], tables[t if len(tables) > 1 else 0]) for t in range(n_time)], axis=1)
    return (br.plain(moved, v) if blend is None else br.blend(moved, v)), moved


def _check(values, v, tables, blend, got, minmax, what):
    want, moved = _want(values, v, tables, blend)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if want.dtype.kind == "u" or blend is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        if want.dtype == np.float64:
            bound = 8 * 2.0**-52 * br.contributing_max(moved, v)
        else:
            bound = np.spacing(np.abs(want)).astype(np.float64)
        print(what, "max error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), what
    planes = got.reshape(-1, got.shape[-2] * got.shape[-1])
    np.testing.assert_array_equal(minmax, np.stack([planes.min(axis=1), planes.max(axis=1)], axis=1).astype(np.float64),
                                  err_msg=what)


SMALL = [((3, 3), v) for v in (4, 5, 16)] + [((1, 3), 5), ((3, 1), 5)]


@pytest.mark.parametrize("corr", CORRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_grids_equal_shift_then_stitch(mg, dtype, corr):
    rng = np.random.default_rng(100 + DTYPES.index(dtype) * 10 + CORRECTIONS.index(corr))
    for (nr, nc), v in SMALL:
        tiles = _random_tiles(rng, dtype, (2, 2, nr, nc, 40, 48))
        st = _Stitched(tiles, corr, *_fields(rng, corr, 2, 40, 48))
        for n_tables in (1, 2):
            tables = _tables(rng, n_tables, nr, nc, v // 2)
            for blend in (None, "linear"):
                got, minmax = st.stitch(v, blend, shifts=tables if n_tables > 1 else tables[0])
                _check(st.values, v, tables, blend, got, minmax, f"{dtype} {corr} {nr}x{nc} v={v} tables={n_tables} {blend}")


@pytest.mark.parametrize("corr", CORRECTIONS)
def test_aligned_tiles_with_aligned_and_unaligned_shifts(mg, corr):
    """2 x 3 of 64 x 64 uint16, v = 16: every unshifted chunk is one aligned 16-byte vector; shifts that are multiples
    of 8 pixels keep that, the others do not."""
    rng = np.random.default_rng(164)
    tiles = _random_tiles(rng, "uint16", (2, 2, 2, 3, 64, 64))
    st = _Stitched(tiles, corr, *_fields(rng, corr, 2, 64, 64))
    table = np.array([[[0, 8], [8, -8], [-8, 0]], [[3, 8], [-8, 5], [-7, 1]]], dtype=np.int32)[None]
    for blend in (None, "linear"):
        got, minmax = st.stitch(16, blend, shifts=table[0])
        _check(st.values, 16, table, blend, got, minmax, f"aligned {corr} {blend}")


@pytest.mark.parametrize("corr", CORRECTIONS)
def test_wide_canvas_and_nine_planes(mg, corr):
    """2 x 3 of 256 x 1024 uint16, v = 102: 2766 columns (more than one workgroup column of 2048) and 9 planes (one
    more than a workgroup's 8), one table per timepoint."""
    rng = np.random.default_rng(202)
    tiles = _random_tiles(rng, "uint16", (3, 3, 2, 3, 256, 1024))
    st = _Stitched(tiles, corr, *_fields(rng, corr, 3, 256, 1024))
    tables = _tables(rng, 3, 2, 3, 51)
    for blend in (None, "linear"):
        got, minmax = st.stitch(102, blend, shifts=tables)
        assert got.shape == (3, 3, 308, 2766)
        _check(st.values, 102, tables, blend, got, minmax, f"wide {corr} {blend}")


@pytest.mark.parametrize("corr", CORRECTIONS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_a_zero_table_gives_the_bytes_of_the_existing_pass(mg, dtype, corr):
    rng = np.random.default_rng(5)
    tiles = _random_tiles(rng, dtype, (2, 2, 3, 3, 40, 48))
    st = _Stitched(tiles, corr, *_fields(rng, corr, 2, 40, 48))
    for blend in (None, "linear"):
        image, minmax = st.stitch(16, blend)
        for zero in (np.zeros((3, 3, 2), dtype=np.int32), np.zeros((2, 3, 3, 2), dtype=np.int32)):
            got, got_mm = st.stitch(16, blend, shifts=zero)
            assert got.tobytes() == image.tobytes() and got_mm.tobytes() == minmax.tobytes(), (dtype, corr, blend)


def test_shift_tables_are_checked(mg):
    import torch

    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    dev = torch.from_numpy(_random_tiles(np.random.default_rng(1), "uint16", (1, 2, 2, 2, 40, 48))).cuda()
    for bad in (np.full((2, 2, 2), 5, dtype=np.int32), np.zeros((3, 2, 2, 2), dtype=np.int32), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            hotpath.flatfield_stitch(dev, 8, apply_flatfield=False, shifts=bad)
    # the entry itself refuses a table outside [-clip, clip], n_tables not in {1, T} and a blend flag that is none
    image = torch.empty((1, 2, 64, 80), dtype=torch.uint16, device="cuda")
    table = torch.full((1, 2, 2, 2), 5, dtype=torch.int32, device="cuda")
    ok = torch.zeros((2, 2, 2, 2), dtype=torch.int32, device="cuda")
    call = lambda t, n_tables, blend: nat.lib().mg_flatfield_apply_stitch_shift(  # noqa: E731
        dev.data_ptr(), nat.MG_U16, 2, 2, 2, 40, 48, 8, 0, 1, 0.0, 0, 0, 1.0, 0, 0, 0, image.data_ptr(), 0, t.data_ptr(),
        n_tables, 2, blend, hotpath._stream())
    assert call(ok, 2, 0) == 0 and call(ok, 1, 1) == 0
    assert call(table, 1, 0) == -1 and call(ok, 3, 0) == -1 and call(ok, 1, 2) == -1


# ---- c - f. end to end -----------------------------------------------------------------------------------------------

R, CC, TY, TX, V, M, PAD = 3, 3, 96, 112, 24, 4, 8
HY, HX = TY - V, TX - V


@pytest.fixture(scope="module")
def jittered():
    """(scene, e, tiles cut at the jittered positions, the expected table, g): seeds as in tests/test_cpu_register.py."""
    rng = np.random.default_rng(11)
    scene, _ = noisy_bead_image(1, (R * HY + V + 2 * PAD, CC * HX + V + 2 * PAD), 40, r_lo=4, r_hi=8)
    e = rr.draw_errors(rng, R, CC, M)
    want, g = rr.expected_table(e)
    return scene, e, rr.cut_jittered(scene, R, CC, TY, TX, V, e, PAD), want, g


def _image(mg, tiles, dims=("row", "col", "y", "x"), **kw):
    return mg.image(mg.DataArray(data=tiles, dims=dims), overlap=V, **kw)


def _replicated(table, blend):
    """(R hy, Cc hx) bool: the pixels of the registered stitch that read a value the shift replicated from a tile's
    edge (none without blend: the kept part of a tile moved by at most clip stays inside it)."""
    nr, nc = table.shape[:2]
    inside = np.zeros((nr, nc, TY, TX))
    for r in range(nr):
        for c in range(nc):
            yy, xx = np.arange(TY) - table[r, c, 0], np.arange(TX) - table[r, c, 1]
            inside[r, c] = ((yy >= 0) & (yy < TY))[:, None] & ((xx >= 0) & (xx < TX))[None, :]
    return (br.plain(inside, V) if blend is None else br.blend(inside, V)) < 1 - 1e-12


def _per_tile_noise(rng, tiles):
    noisy = tiles.astype(np.float64) + rng.poisson(20, size=tiles.shape) + rng.normal(0, 3, size=tiles.shape)
    return np.clip(np.rint(noisy), 0, 65535).astype(np.uint16)


@pytest.mark.parametrize("blend", [None, "linear"])
def test_jittered_tiles_are_put_back_on_the_scene(mg, jittered, blend):
    scene, e, tiles, want, g = jittered
    out = _image(mg, tiles, register="ncc", max_shift=M, blend=blend)
    np.testing.assert_array_equal(out["tile_shift"].values, want[None])
    assert out["tile_shift"].dims == ("reg_time", "reg_row", "reg_col", "yx") and out["tile_shift"].values.dtype == np.int32
    assert out["seam_shift"].values.shape == (1, 12, 2) and out["seam_score"].values.shape == (1, 12)
    assert out["seam_score"].values.min() >= 0.99 and out.attrs["tile_shift_clipped"] == 0
    for s, (a, b) in enumerate(rr.seams(R, CC)):
        np.testing.assert_array_equal(out["seam_shift"].values[0, s], e[b] - e[a])
    crop = rr.scene_crop(scene, R, CC, TY, TX, V, PAD, e[0, 0], g)
    got = out["image"].values
    np.testing.assert_array_equal(got, rr.stitch(tiles, V, want, blend))
    replicated = _replicated(want, blend)
    assert not replicated.any() if blend is None else 0 < replicated.mean() < 0.05
    np.testing.assert_array_equal(got[~replicated], crop[~replicated])
    plain = _image(mg, tiles, blend=blend)
    assert "tile_shift" not in plain and (plain["image"].values != crop).any()


def test_per_tile_noise_and_a_pending_flatfield_give_the_same_table(mg, jittered):
    from magnify_amd import preprocess
    from magnify_amd.stitch import Stitcher

    _, _, tiles, want, _ = jittered
    noisy = _per_tile_noise(np.random.default_rng(11), tiles)
    np.testing.assert_array_equal(_image(mg, noisy, register="ncc", max_shift=M)["tile_shift"].values, want[None])
    vig = vignette((TY, TX))
    raw = np.clip(np.rint(tiles.astype(np.float64) * vig + 100), 0, 65535).astype(np.uint16)
    ds = preprocess.standardize_format(mg.DataArray(data=raw, dims=("row", "col", "y", "x")))
    ds = preprocess.flatfield_correct(ds, flatfield=vig, darkfield=100)
    lazy = ds.data_vars["tile"].raw
    ds = Stitcher(overlap=V, register="ncc", max_shift=M)(ds)
    np.testing.assert_array_equal(ds["tile_shift"].values, want[None])
    # the image: the corrected tiles (materialize: the overlap-0 path), shifted, then the plain stitch
    np.testing.assert_array_equal(ds["image"].values[0, 0], rr.stitch(lazy.materialize().cpu().numpy()[0, 0], V, want))


def test_featureless_tiles_stay_where_they_are(mg):
    """2 x 3: beads only under the first two tile columns, a constant background under the last, noise per tile."""
    nr, nc = 2, 3
    rng = np.random.default_rng(100)
    shape = (nr * HY + V + 2 * PAD, nc * HX + V + 2 * PAD)
    pos = random_bead_positions(rng, (shape[0], PAD + 2 * HX - 10), 25, 8)
    radii, values = rng.integers(4, 9, size=len(pos)), rng.integers(500, 4001, size=len(pos))
    beads = draw_beads(shape, pos, 2 * radii, values).astype(np.float64)
    scene = np.where(beads > 0, beads + 120.0, 120.0)
    e = rr.draw_errors(rng, nr, nc, M)
    tiles = _per_tile_noise(rng, rr.cut_jittered(scene, nr, nc, TY, TX, V, e, PAD))
    out = _image(mg, tiles, register="ncc", max_shift=M)
    shift, score = out["tile_shift"].values[0], out["seam_score"].values[0]
    touches_last = np.array([a[1] == 2 or b[1] == 2 for a, b in rr.seams(nr, nc)])
    assert (score[touches_last] < 0.5).all() and (score[touches_last] <= 0.1).all() and (score[~touches_last] >= 0.99).all()
    np.testing.assert_array_equal(shift[:, 2], 0)
    np.testing.assert_array_equal(shift[:, :2], rr.expected_table(e[:, :2])[0])
    np.testing.assert_array_equal(shift, rr.register(tiles, V, M)[0])


def test_two_timepoints(mg):
    from magnify_amd import preprocess
    from magnify_amd.stitch import Stitcher

    rng = np.random.default_rng(21)
    scene, _ = noisy_bead_image(1, (R * HY + V + 2 * PAD, CC * HX + V + 2 * PAD), 40, r_lo=4, r_hi=8)
    es = [rr.draw_errors(rng, R, CC, M) for _ in range(2)]
    tiles = np.stack([rr.cut_jittered(scene, R, CC, TY, TX, V, e, PAD) for e in es])
    tables = [rr.expected_table(e) for e in es]
    assert (tables[0][0] != tables[1][0]).any()
    dataset = lambda: preprocess.standardize_format(mg.DataArray(data=tiles, dims=("time", "row", "col", "y", "x")))  # noqa: E731
    each = Stitcher(overlap=V, register="ncc", max_shift=M, register_time="each")(dataset())
    assert each["tile_shift"].values.shape == (2, R, CC, 2) and each["seam_score"].values.shape == (2, 12)
    for t in range(2):
        np.testing.assert_array_equal(each["tile_shift"].values[t], tables[t][0])
        np.testing.assert_array_equal(each["image"].values[0, t],
                                      rr.scene_crop(scene, R, CC, TY, TX, V, PAD, es[t][0, 0], tables[t][1]))
    first = Stitcher(overlap=V, register="ncc", max_shift=M, register_time=0)(dataset())
    np.testing.assert_array_equal(first["tile_shift"].values, tables[0][0][None])
    np.testing.assert_array_equal(first["image"].values[0, 0], each["image"].values[0, 0])
    np.testing.assert_array_equal(first["image"].values[0, 1], rr.stitch(tiles[1], V, tables[0][0]))
    second = Stitcher(overlap=V, register="ncc", max_shift=M, register_time=1)(dataset())
    np.testing.assert_array_equal(second["tile_shift"].values, tables[1][0][None])


def test_a_single_tile_has_nothing_to_register(mg):
    one = _random_tiles(np.random.default_rng(3), "uint16", (1, 1, TY, TX))
    out = _image(mg, one, register="ncc", max_shift=M)
    np.testing.assert_array_equal(out["image"].values, br.plain(one, V))
    np.testing.assert_array_equal(out["tile_shift"].values, np.zeros((1, 1, 1, 2), dtype=np.int32))
    assert "seam_score" not in out


def test_the_results_survive_save_and_load(mg, jittered, tmp_path):
    _, _, tiles, want, _ = jittered
    out = _image(mg, tiles, register="ncc", max_shift=M)
    mg.save(tmp_path / "registered.nc", out)
    back = mg.load(tmp_path / "registered.nc")
    for name in ("tile_shift", "seam_shift", "seam_score", "image"):
        assert back[name].dims == out[name].dims, name
        np.testing.assert_array_equal(back[name].values, out[name].values, err_msg=name)
    assert back["tile_shift"].values.dtype == np.int32 and back["seam_score"].values.dtype == np.float64
    np.testing.assert_array_equal(back["tile_shift"].values, want[None])
    assert int(back.attrs["tile_shift_clipped"]) == 0


def test_register_channel_by_name(mg, jittered):
    """Two channels: "dapi" is a constant with noise of its own per tile (nothing to register), "egfp" the scene."""
    _, _, tiles, want, _ = jittered
    blank = _per_tile_noise(np.random.default_rng(3), np.full_like(tiles, 120))
    data = mg.DataArray(data=np.stack([blank, tiles]), dims=("channel", "row", "col", "y", "x"),
                        coords={"channel": ["dapi", "egfp"]})
    out = mg.image(data, overlap=V, register="ncc", max_shift=M, register_channel="egfp")
    np.testing.assert_array_equal(out["tile_shift"].values, want[None])
    by_index = mg.image(data, overlap=V, register="ncc", max_shift=M, register_channel=1)
    np.testing.assert_array_equal(by_index["image"].values, out["image"].values)
    np.testing.assert_array_equal(out["image"].values, rr.stitch(np.stack([blank, tiles]), V, want))  # both channels moved
    first = mg.image(data, overlap=V, register="ncc", max_shift=M)  # None: the first channel -- no seam scores
    assert (first["seam_score"].values < 0.5).all() and not first["tile_shift"].values.any()
    np.testing.assert_array_equal(first["image"].values, br.plain(np.stack([blank, tiles]), V))
    with pytest.raises(ValueError, match="register_channel"):
        mg.image(data, overlap=V, register="ncc", max_shift=M, register_channel="cy5")


@pytest.mark.parametrize("blend", [None, "linear"])
def test_a_pending_shading_correction(mg, jittered, blend):
    """``Stitcher`` on a ``LazyShading``: the table is that of the corrected tiles, the image the corrected tiles
    (``materialize``: the overlap-0 path) shifted and stitched."""
    import torch

    from magnify_amd import preprocess, shading
    from magnify_amd.stitch import Stitcher

    _, _, tiles, want, _ = jittered
    vig = vignette((TY, TX))
    raw = np.clip(np.rint(tiles.astype(np.float64) * vig + 100), 0, 65535).astype(np.uint16)
    ds = preprocess.standardize_format(mg.DataArray(data=raw, dims=("row", "col", "y", "x")))
    dev = preprocess.to_device(ds.data_vars["tile"].data)
    lazy = shading.LazyShading(dev, torch.from_numpy(vig[None]).cuda(), torch.full((1, TY, TX), 100.0, device="cuda"))
    ds.data_vars["tile"] = mg.DataArray(lazy, ds.data_vars["tile"].dims, name="tile")
    values = lazy.materialize().cpu().numpy()[0, 0]
    ds = Stitcher(overlap=V, blend=blend, register="ncc", max_shift=M)(ds)
    np.testing.assert_array_equal(ds["tile_shift"].values[0], rr.register(values, V, M)[0])
    np.testing.assert_array_equal(ds["tile_shift"].values, want[None])
    np.testing.assert_array_equal(ds["image"].values[0, 0], rr.stitch(values, V, want, blend))
