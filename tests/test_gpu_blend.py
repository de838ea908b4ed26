"""``stitch(blend="linear")`` on the device against its NumPy restatement (tests/blend_ref.py) applied to the values the
plain pass writes for every tile -- taken from the plain path itself, ``blend=None`` with overlap 0 tile by tile (what
``LazyFlatfield.materialize`` / ``LazyShading.materialize`` do), which the golden tests pin.

Tolerances: integer pixels are equal.  float64: 8 * 2**-52 * max|contributing values| (seven float64 operations, with
or without fused multiply-add).  float32: one float32 ulp of the reference after the cast."""
import numpy as np
import pytest

import blend_ref as br
from synth import draw_chip, noisy_bead_image

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


def _fields(rng, corr, c, ty, tx):
    if corr == "flatfield":  # an image flat and a scalar dark
        return rng.uniform(0.6, 1.4, size=(ty, tx)).astype(np.float32), 7.0
    if corr == "shading":    # per-channel float32 fields
        return (rng.uniform(0.6, 1.4, size=(c, ty, tx)).astype(np.float32),
                rng.uniform(0.0, 20.0, size=(c, ty, tx)).astype(np.float32))
    return None, None


def _run(tiles, v, corr, flat, dark, blend):
    """(per-tile values of the plain path, the stitched image with ``blend``, its minmax) as host arrays."""
    import torch

    from magnify_amd import hotpath, shading

    c, t, nr, nc, ty, tx = tiles.shape
    dev = torch.from_numpy(tiles).cuda()
    if corr == "none":
        values = tiles
        image, minmax = hotpath.flatfield_stitch(dev, v, apply_flatfield=False, blend=blend)
    elif corr == "flatfield":
        max2 = hotpath.flatfield_max(dev, flat, dark)
        per_tile, _ = hotpath.flatfield_stitch(dev.reshape(c * t * nr * nc, 1, 1, 1, ty, tx), 0, flat, dark, max2=max2,
                                               want_minmax=False)
        values = per_tile.reshape(tiles.shape).cpu().numpy()
        image, minmax = hotpath.flatfield_stitch(dev, v, flat, dark, max2=max2, blend=blend)
    else:
        fl, dk = torch.from_numpy(flat).cuda(), torch.from_numpy(dark).cuda()
        per_tile, _ = shading.apply_stitch(dev.reshape(c, t * nr * nc, 1, 1, ty, tx), 0, fl, dk, want_minmax=False)
        values = per_tile.reshape(tiles.shape).cpu().numpy()
        image, minmax = shading.apply_stitch(dev, v, fl, dk, blend=blend)
    return values, image.cpu().numpy(), minmax.cpu().numpy()


def _check(values, v, got, minmax, what):
    want = br.blend(values, v)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if want.dtype.kind == "u":
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        if want.dtype == np.float64:
            bound = 8 * 2.0**-52 * br.contributing_max(values, v)
        else:
            bound = np.spacing(np.abs(want)).astype(np.float64)
        print(what, "max error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), what
    planes = got.reshape(-1, got.shape[-2] * got.shape[-1])
    np.testing.assert_array_equal(minmax, np.stack([planes.min(axis=1), planes.max(axis=1)], axis=1).astype(np.float64),
                                  err_msg=what)


# 3 x 3 of 40 x 48: four-tile corners, an odd overlap, 2 v == tile; 1 x 3 and 3 x 1: bands along one axis only
SMALL = [((3, 3), v) for v in (0, 1, 2, 5, 16, 20)] + [((1, 3), 5), ((3, 1), 5)]


@pytest.mark.parametrize("corr", CORRECTIONS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_grids_equal_the_restatement(mg, dtype, corr):
    rng = np.random.default_rng(DTYPES.index(dtype) * 10 + CORRECTIONS.index(corr))
    for (nr, nc), v in SMALL:
        tiles = _random_tiles(rng, dtype, (2, 1, nr, nc, 40, 48))
        flat, dark = _fields(rng, corr, 2, 40, 48)
        values, got, minmax = _run(tiles, v, corr, flat, dark, "linear")
        _check(values, v, got, minmax, f"{dtype} {corr} {nr}x{nc} v={v}")
        if v == 0:  # no bands: the plain stitch
            np.testing.assert_array_equal(got, _run(tiles, v, corr, flat, dark, None)[1])


@pytest.mark.parametrize("corr", CORRECTIONS)
def test_aligned_chunks_and_the_plain_path_unchanged(mg, corr):
    """2 x 3 of 64 x 64 uint16, v = 16: hx % 8 == 0 and clip % 8 == 0, every chunk one aligned 16-byte vector."""
    import torch

    from magnify_amd import hotpath

    rng = np.random.default_rng(64)
    tiles = _random_tiles(rng, "uint16", (2, 2, 2, 3, 64, 64))
    flat, dark = _fields(rng, corr, 2, 64, 64)
    values, got, minmax = _run(tiles, 16, corr, flat, dark, "linear")
    _check(values, 16, got, minmax, f"aligned {corr}")
    _, plain, plain_mm = _run(tiles, 16, corr, flat, dark, None)
    np.testing.assert_array_equal(plain, br.plain(values, 16))
    if corr != "shading":  # blend=None is the call without the keyword, byte for byte
        dev = torch.from_numpy(tiles).cuda()
        if corr == "none":
            image, mm = hotpath.flatfield_stitch(dev, 16, apply_flatfield=False)
        else:
            image, mm = hotpath.flatfield_stitch(dev, 16, flat, dark)
        assert image.cpu().numpy().tobytes() == plain.tobytes() and mm.cpu().numpy().tobytes() == plain_mm.tobytes()


@pytest.mark.parametrize("corr", CORRECTIONS)
def test_wide_canvas_and_nine_planes(mg, corr):
    """2 x 3 of 256 x 1024 uint16, v = 102: 2766 columns (more than one workgroup column of 2048) and 9 planes (one
    more than a workgroup's 8)."""
    rng = np.random.default_rng(102)
    tiles = _random_tiles(rng, "uint16", (3, 3, 2, 3, 256, 1024))
    flat, dark = _fields(rng, corr, 3, 256, 1024)
    values, got, minmax = _run(tiles, 102, corr, flat, dark, "linear")
    assert got.shape == (3, 3, 308, 2766)
    _check(values, 102, got, minmax, f"wide {corr}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_minmax_is_that_of_the_blended_image(mg, dtype):
    """The plane's maximum sits on a band pixel of its owner tile and the neighbour is lower there: the blended
    maximum is below the unblended one."""
    rng = np.random.default_rng(3)
    v, ty, tx = 16, 40, 48
    tiles = _random_tiles(rng, dtype, (1, 2, 3, 3, ty, tx))
    tiles = (tiles // 4 if tiles.dtype.kind == "u" else tiles / 4).astype(dtype)
    top = np.iinfo(dtype).max if tiles.dtype.kind == "u" else 1.0e6
    tiles[0, 0, 1, 1, 20, v // 2 + (tx - v) - 3] = top  # canvas column hx + (hx - 3): in the band before the seam at 2 hx
    tiles[0, 1, 0, 2, v // 2 + 2, 30] = top             # the other plane: outside every band, stays the maximum
    values, got, minmax = _run(tiles, v, "none", None, None, "linear")
    _check(values, v, got, minmax, f"minmax {dtype}")
    _, plain, plain_mm = _run(tiles, v, "none", None, None, None)
    assert plain_mm[0, 1] == top and minmax[0, 1] < top and minmax[1, 1] == top == plain_mm[1, 1]


def _image(mg, tiles, **kw):
    return mg.image(mg.DataArray(data=tiles, dims=("row", "col", "y", "x")), **kw)["image"].values


def test_image_pipeline_blends(mg):
    rng = np.random.default_rng(21)
    tiles = _random_tiles(rng, "uint16", (2, 3, 64, 72))
    got = _image(mg, tiles, overlap=16, blend="linear")
    np.testing.assert_array_equal(got, br.blend(tiles, 16))
    assert (got != _image(mg, tiles, overlap=16)).any()


def test_consistent_chip_tiles_blend_to_themselves(mg):
    canvas = draw_chip((10, 10), 20)  # 1100 x 1100
    tiles = br.cut_tiles(canvas, 2, 2, 558, 558, 16)
    plain = _image(mg, tiles, overlap=16)
    assert plain.shape == (1084, 1084)
    np.testing.assert_array_equal(_image(mg, tiles, overlap=16, blend="linear"), plain)


def test_process_stream_blends_like_the_component(mg, monkeypatch):
    import torch

    from magnify_amd import stack

    scene, _ = noisy_bead_image(5, (256, 256), 6, r_lo=6, r_hi=12)
    one = br.cut_tiles(scene, 2, 2, 136, 136, 16).astype(np.uint16)
    one += (np.arange(4, dtype=np.uint16).reshape(2, 2, 1, 1) * 50)  # tiles that disagree: the seams show
    block = np.stack([one, one[::-1, ::-1].copy()])[:, None]          # (T, C, rows, cols, ty, tx)
    made, real = [], stack.StackProcessor

    def recording(*args, **kw):  # (a function, not a subclass: a class would keep the processor alive in a reference
        made.append(real(*args, **kw))  # cycle, for the garbage collector to free from whatever thread it runs in)
        return made[-1]

    monkeypatch.setattr(stack, "StackProcessor", recording)
    outs = list(stack.process_stream(iter([torch.from_numpy(block)]), overlap=16, blend="linear", num_iter=2000,
                                     min_bead_diameter=10, max_bead_diameter=26))
    assert len(outs) == 1 and len(made) == 1 and made[0].blend == "linear"
    image = made[0].image.cpu().numpy()
    for t in range(2):
        want = _image(mg, block[t, 0], overlap=16, blend="linear")
        np.testing.assert_array_equal(image[t, 0], want)
        assert (want != _image(mg, block[t, 0], overlap=16)).any()
    del outs
    made.clear()  # the processor, its finder and the graphs it captured go here, on this thread
