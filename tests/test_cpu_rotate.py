"""The NumPy restatement of the rotation arithmetic (tests/rotate_ref.py, the oracle of the GPU tests) against
``scipy.ndimage.rotate`` -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

pytest.importorskip("scipy")
from scipy import ndimage  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rotate_ref as rr  # noqa: E402

SHAPES = [(37, 53), (64, 64), (130, 71)]
ANGLES = [0.7, -3.25, 45, 90, 180, 1e-3, 200.5]
# largest |restatement - scipy| / (max - min) of a float64 plane over SHAPES x ANGLES, measured with scipy 1.15.3
F64_MEASURED = 2.61e-14


def _scipy(img, angle):
    return ndimage.rotate(img, angle, axes=(-1, -2), reshape=False, order=1, mode="constant", cval=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_scipy_in_every_pixel(shape):
    for angle in ANGLES:
        rng = np.random.default_rng(0)
        for dtype in ("uint8", "uint16", "float32"):
            img = rr.random_image(rng, dtype, shape)
            got = rr.rotate(img, angle)
            assert got.dtype == img.dtype and got.shape == img.shape
            np.testing.assert_array_equal(got, _scipy(img, angle), err_msg=f"{dtype} {shape} {angle}")


def test_restatement_float64_within_rounding_of_scipy():
    """float64 differs from scipy only by the rounding of the sampling coordinate (about 1e-14 of a pixel, scipy sums
    it in another order) times the pixel gradient.  Measured: 2.61e-14 of the plane's (max - min) at worst over the
    shapes and angles above (scipy 1.15.3); the bound is ten times that.  It bounds the restatement against scipy --
    the kernel is held to the restatement bit for bit (tests/test_gpu_rotate.py)."""
    worst = 0.0
    for shape in SHAPES:
        for angle in ANGLES:
            rng = np.random.default_rng(0)
            for dtype in ("uint8", "uint16", "float32", "float64"):  # (the draws before the float64 one: as measured)
                img = rr.random_image(rng, dtype, shape)
            diff = np.abs(rr.rotate(img, angle) - _scipy(img, angle)).max() / (img.max() - img.min())
            worst = max(worst, float(diff))
    print(f"float64 restatement vs scipy: worst relative difference {worst:.3e}")
    assert worst <= 10 * F64_MEASURED


def test_sign_of_the_rotation():
    """One bright pixel right of the centre, 90 degrees: it lands above the centre (scipy's sense with
    axes=(-1, -2): positive angles turn the picture counter-clockwise on a display with y pointing down)."""
    img = np.zeros((9, 9), dtype=np.uint16)
    img[4, 7] = 1000
    got = rr.rotate(img, 90)
    want = np.zeros_like(img)
    want[1, 4] = 1000
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, _scipy(img, 90))
    back = np.zeros_like(img)
    back[7, 4] = 1000
    np.testing.assert_array_equal(rr.rotate(img, -90), back)


def test_matrix_and_offset_are_scipys():
    m, off = rr.rotation_matrix_offset(90, 37, 53)
    np.testing.assert_array_equal(m, [[0.0, 1.0], [-1.0, 0.0]])  # cosdg / sindg: exact at multiples of 90
    np.testing.assert_array_equal(off, [18.0 - 26.0, 26.0 + 18.0])
    m, off = rr.rotation_matrix_offset(0.0, 5, 7)
    np.testing.assert_array_equal(m, np.eye(2))
    np.testing.assert_array_equal(off, [0.0, 0.0])
