"""``rotate``: the bilinear resampling kernel (mg_affine_bilinear) against its NumPy restatement (tests/rotate_ref.py,
itself held to scipy.ndimage.rotate by tests/test_cpu_rotate.py) bit for bit, the component's contract, and a tilted
chip through ``mg.microfluidic_chip(rotation=)``."""
import numpy as np
import pytest

pytest.importorskip("scipy")

import rotate_ref as rr  # noqa: E402
from synth import draw_chip  # noqa: E402

pytestmark = pytest.mark.gpu

ANGLES = [0.7, -3.25, 45, 90, 180, 200.5]
DTYPES = ["uint8", "uint16", "float32", "float64"]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    magnify_amd.seed(4321)
    return magnify_amd


def _rotate_on_device(image, angle, want_minmax=True):
    import torch

    from magnify_amd import hotpath

    out, minmax = hotpath.rotate_image(torch.from_numpy(image).cuda(), angle, want_minmax=want_minmax)
    return out.cpu().numpy(), None if minmax is None else minmax.cpu().numpy()


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=what)


# 1 x 1 and the one-pixel-wide planes (no horizontal / vertical neighbour); 37 x 53 and 130 x 71 (odd widths: u8 / u16
# rows start anywhere in a dword); 300 x 517: several workgroup tiles both ways with ragged edges
@pytest.mark.parametrize("shape", [(1, 1), (1, 19), (19, 1), (37, 53), (130, 71), (300, 517)])
def test_kernel_equals_restatement_bit_for_bit(mg, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for dtype in DTYPES:
        img = rr.random_image(rng, dtype, shape)
        for angle in ANGLES:
            got, minmax = _rotate_on_device(img[None, None], angle)
            want = rr.rotate(img, angle)
            _same_bits(got[0, 0], want, f"{dtype} {shape} {angle}")
            np.testing.assert_array_equal(minmax, [[want.min(), want.max()]], err_msg=f"{dtype} {shape} {angle}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_planes_rotate_independently_with_their_minmax(mg, dtype):
    rng = np.random.default_rng(5)
    stack = rr.random_image(rng, dtype, (2, 3, 37, 53))
    stack[1, 2] = stack[1, 2] // 3 + 1  # (a plane with another range)
    stack[0, 1, 10:20] = 0
    got, minmax = _rotate_on_device(stack, -3.25)
    want = rr.rotate(stack, -3.25)
    _same_bits(got, want, dtype)
    planes = want.reshape(6, -1)
    np.testing.assert_array_equal(minmax, np.stack([planes.min(axis=1), planes.max(axis=1)], axis=1).astype(np.float64))
    again, none = _rotate_on_device(stack, -3.25, want_minmax=False)  # the d_minmax = NULL path
    assert none is None
    _same_bits(again, want, dtype)


def test_float_nan_propagates_into_the_minmax(mg):
    img = rr.random_image(np.random.default_rng(2), "float32", (20, 31))
    img[9, 14] = np.nan
    got, minmax = _rotate_on_device(img[None, None], 0.7)
    want = rr.rotate(img, 0.7)
    assert np.isnan(want).any()
    _same_bits(got[0, 0], want, "nan")
    assert np.isnan(minmax).all()  # as np.min / np.max


def _tiles(rng):
    return rng.integers(0, 60000, size=(2, 2, 40, 40)).astype(np.uint16)


def test_image_pipeline_rotates(mg):
    data = mg.DataArray(data=_tiles(np.random.default_rng(11)), dims=("row", "col", "y", "x"))
    plain = mg.image(data, overlap=5)["image"].values
    assert plain.shape == (70, 70)
    turned = mg.image(data, overlap=5, rotation=7.5)["image"].values
    _same_bits(turned, rr.rotate(plain, 7.5), "image pipeline")


def _stitched(mg, tiles):
    pipe = mg.image_pipe(overlap=5)
    for name in ("rotate", "drop", "restore_format"):
        pipe.remove_pipe(name)
    return pipe(mg.DataArray(data=tiles, dims=("row", "col", "y", "x")))


def test_component_cache_and_errors(mg):
    from magnify_amd import find, preprocess

    tiles = _tiles(np.random.default_rng(12))
    ds = _stitched(mg, tiles)
    before = ds.data_vars["image"].data
    ptr, cache = before.data_ptr(), ds._cache["image_minmax"]
    for turns in (0, 360, -720.0):  # whole turns: the same object, the same memory, the same cache
        out = preprocess.rotate(ds, rotation=turns)
        assert out is ds and out.data_vars["image"].data.data_ptr() == ptr and ds._cache["image_minmax"] is cache
    plain = before.cpu().numpy()
    with pytest.raises(ValueError):
        preprocess.rotate(ds, rotation=float("nan"))
    with pytest.raises(ValueError):
        preprocess.rotate(ds, rotation=float("inf"))
    with pytest.raises(AttributeError):  # before stitch: no image yet
        preprocess.rotate(preprocess.standardize_format(mg.DataArray(data=tiles, dims=("row", "col", "y", "x"))),
                          rotation=5)
    assert ds.data_vars["image"].data.data_ptr() == ptr  # (the refusals left the dataset alone)

    out = preprocess.rotate(ds, rotation=-12.5)
    image = find._image_tensor(out)
    want = rr.rotate(plain, -12.5)
    assert out.data_vars["image"].dims == ("channel", "time", "im_y", "im_x") and image.dtype == before.dtype
    _same_bits(image.cpu().numpy(), want, "component")
    assert image.data_ptr() != ptr
    minmax = find._plane_minmax(out, image, (0, 0))  # the finders' cached min / max is the rotated plane's
    assert minmax is not None
    np.testing.assert_array_equal(minmax.cpu().numpy(), [[want.min(), want.max()]])

    host = _stitched(mg, tiles)
    host["image"] = mg.DataArray(plain.copy(), ("channel", "time", "im_y", "im_x"))  # a host-resident image
    _same_bits(find._image_tensor(preprocess.rotate(host, rotation=-12.5)).cpu().numpy(), want, "host image")


def test_tilted_chip_is_found_after_rotating_it_back(mg):
    """The 10 x 10 chip of test_gpu_chip_api.test_ten_by_ten_chip mounted 4 degrees off, with that test's arguments
    and assertions.  Without the rotation the buttons are found where they are: the reference's chip path
    (oracle/ref_pipeline.find_centers + find_rois) on this tilted image puts button [4, 3] at x 397.0, y 511.0 and
    button [0, 0] at x 70, y 133 -- outside the 5 px / 5 % windows below; 4 degrees was enough, and every button stays
    68 px or more inside the 1100 x 1100 canvas."""
    tilted = rr.rotate(draw_chip((10, 10), 20), 4.0)
    xp = mg.microfluidic_chip(data=mg.DataArray(data=tilted, dims=("y", "x")), shape=(10, 10), num_iter=10000,
                              rotation=-4.0, min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100,
                              col_dist=100)
    xp = xp.unstack().transpose("mark_row", "mark_col", ...)
    assert xp.roi.sizes["mark_row"] == 10 and xp.roi.sizes["mark_col"] == 10
    radii = np.sqrt(xp.fg.sum(["roi_x", "roi_y"]).to_numpy() / np.pi)
    print("radii", radii.min(), radii.max(), "x00", xp.x[0, 0].values.item(), "y00", xp.y[0, 0].values.item(),
          "x43", xp.x[4, 3].values.item(), "y43", xp.y[4, 3].values.item())
    assert 0.9 * 10 < radii.min() and radii.max() < 1.1 * 10
    assert 0.95 * 100 < xp.x[0, 0].values.item() < 1.05 * 100
    assert 0.95 * 100 < xp.y[0, 0].values.item() < 1.05 * 100
    assert 395 < xp.x[4, 3].values.item() < 405 and 495 < xp.y[4, 3].values.item() < 505
