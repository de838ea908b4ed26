"""``stitch(blend="linear")`` without a GPU: the properties of its NumPy restatement (tests/blend_ref.py), the refusals
of ``Stitcher`` and the keyword on the public functions."""
import inspect

import numpy as np
import pytest

import blend_ref as br
import magnify_amd as mg
from magnify_amd import hotpath, preprocess
from magnify_amd.stitch import Stitcher

GRIDS = [(2, 3), (3, 3), (1, 2), (2, 1)]
TY, TX = 12, 16


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("v", [0, 1, 4, 5, TY // 2])
def test_tiles_of_one_scene_blend_to_the_plain_stitch(grid, v):
    R, C = grid
    rng = np.random.default_rng(100 * R + 10 * C + v)
    for dtype in (np.uint8, np.uint16):
        scene = rng.integers(0, np.iinfo(dtype).max + 1, size=(2, R * (TY - v) + v, C * (TX - v) + v)).astype(dtype)
        tiles = br.cut_tiles(scene, R, C, TY, TX, v)
        want = br.plain(tiles, v)
        c = v // 2
        np.testing.assert_array_equal(want, scene[:, c : c + want.shape[1], c : c + want.shape[2]])  # (plain is the scene)
        np.testing.assert_array_equal(br.blend(tiles, v), want)
    # floats: the two weights of a pixel sum to 1 only after rounding -- equal within the derived bound
    scene = rng.normal(size=(R * (TY - v) + v, C * (TX - v) + v))
    tiles = br.cut_tiles(scene, R, C, TY, TX, v)
    got, want = br.blend(tiles, v), br.plain(tiles, v)
    assert np.all(np.abs(got - want) <= 8 * 2.0**-52 * np.abs(want))


def test_two_constant_tiles_ramp_across_the_band():
    tiles = np.empty((1, 2, 12, 20), np.uint16)
    tiles[0, 0], tiles[0, 1] = 100, 300
    row = br.blend(tiles, 6)[0]
    seam = 20 - 6  # the kept width of the first tile
    assert row[seam - 4 : seam + 4].tolist() == [100, 117, 150, 183, 217, 250, 283, 300]
    assert set(row[: seam - 3].tolist()) == {100} and set(row[seam + 3 :].tolist()) == {300}
    col = br.blend(np.ascontiguousarray(tiles.transpose(1, 0, 3, 2)), 6)[:, 0]  # the same along y
    assert col[seam - 4 : seam + 4].tolist() == [100, 117, 150, 183, 217, 250, 283, 300]
    ramp = br.blend(tiles.astype(np.float64), 6)[0, seam - 3 : seam + 3]
    np.testing.assert_allclose(ramp, 100 + 200 * (np.arange(6) + 0.5) / 6, rtol=1e-15)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("v", [0, 1, 4, 5, TY // 2])
def test_random_tiles_differ_from_the_plain_stitch_exactly_in_the_bands(grid, v):
    R, C = grid
    rng = np.random.default_rng(7 + v)
    tiles = rng.normal(size=(R, C, TY, TX))  # (continuous values: a mix of two tiles is never the owner's value)
    got, want = br.blend(tiles, v), br.plain(tiles, v)
    bands = br.band_mask(R, C, TY, TX, v)
    hy, hx = TY - v, TX - v
    count = R * hy * C * hx - (R * hy - (R - 1) * v) * (C * hx - (C - 1) * v)  # all but the pixels outside every band
    assert bands.sum() == count and (v > 0 or count == 0)
    assert (hotpath.blend_bands(R, TY, v), hotpath.blend_bands(C, TX, v)) == (
        [(i * hy - v // 2, i * hy - v // 2 + v) for i in range(1, R)] if v else [],
        [(i * hx - v // 2, i * hx - v // 2 + v) for i in range(1, C)] if v else [])
    np.testing.assert_array_equal(got != want, bands)


def test_restatement_refuses_bands_that_would_meet():
    with pytest.raises(ValueError):
        br.blend(np.zeros((1, 2, 8, 8)), 5)


def _dataset(tiles):
    return preprocess.standardize_format(mg.DataArray(data=tiles, dims=("row", "col", "y", "x")))


def test_stitcher_refuses_unknown_modes_and_meeting_bands():
    with pytest.raises(ValueError, match="blend"):
        Stitcher(blend="cubic")
    with pytest.raises(ValueError, match="blend"):
        mg.components.get("stitch")(overlap=4, blend="cubic")
    with pytest.raises(ValueError, match="blend"):
        mg.image_pipe(blend=True)
    tiles = np.zeros((2, 2, 40, 40), np.uint16)
    with pytest.raises(ValueError, match="2 \\* overlap"):
        Stitcher(overlap=25, blend="linear")(_dataset(tiles))
    with pytest.raises(ValueError, match="blend"):
        hotpath.check_blend("linear", 21, 40, 48)
    assert hotpath.check_blend("linear", 20, 40, 48) == "linear" and hotpath.check_blend(None, 39, 40, 48) is None
    assert Stitcher(overlap=25).blend is None and Stitcher(overlap=20, blend="linear").blend == "linear"


def test_blend_is_a_keyword_of_the_public_functions():
    functions = [mg.components.get("stitch"), mg.microfluidic_chip, mg.microfluidic_chip_pipe, mg.mrbles, mg.mrbles_pipe,
                 mg.beads, mg.beads_pipe, mg.image, mg.image_pipe]
    for f in functions:
        p = inspect.signature(f).parameters
        assert "blend" in p and p["blend"].default is None, f
    from magnify_amd import shading, stack

    for f in (hotpath.flatfield_stitch, shading.apply_stitch, stack.StackProcessor.__init__, stack.process_stream):
        assert inspect.signature(f).parameters["blend"].default is None, f
    stitch = dict(mg.image_pipe(overlap=7, blend="linear").components)["stitch"]
    assert (stitch.overlap, stitch.blend) == (7, "linear")
    assert dict(mg.beads_pipe().components)["stitch"].blend is None
