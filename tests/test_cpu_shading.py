"""Shading model (BaSiC fit, DESIGN.md §4 "shading"): registry, the NumPy oracle's resampling and recovery of
known fields, and fit()'s refusals -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import magnify_amd as mg  # noqa: E402
import ref_shading as rs  # noqa: E402
from magnify_amd import shading  # noqa: E402


def test_shading_correct_is_registered():
    import inspect

    assert "shading_correct" in mg.components.get_all()
    params = inspect.signature(mg.components.get("shading_correct")).parameters
    assert list(params) == ["get_darkfield", "smoothness_flatfield", "smoothness_darkfield", "timepoints",
                            "working_size"]
    assert params["timepoints"].default == (0,) and params["working_size"].default == 128
    assert mg.shading is shading
    with pytest.raises(NotImplementedError):
        mg.components.get("basic_correct")()(None)


def _area_brute(img, w):
    ty, tx = img.shape
    out = np.zeros((w, w))
    for i in range(w):
        for j in range(w):
            y0, y1, x0, x1 = i * ty / w, (i + 1) * ty / w, j * tx / w, (j + 1) * tx / w
            acc = 0.0
            for s in range(int(np.floor(y0)), int(np.ceil(y1))):
                wy = min(y1, s + 1) - max(y0, s)
                xs = np.arange(int(np.floor(x0)), int(np.ceil(x1)))
                wx = np.minimum(x1, xs + 1) - np.maximum(x0, xs)
                acc += wy * (wx * img[s, xs]).sum()
            out[i, j] = acc / ((y1 - y0) * (x1 - x0))
    return out


def _linear_brute(a, ty, tx):
    h, w = a.shape
    out = np.zeros((ty, tx))
    for y in range(ty):
        sy = min(max((y + 0.5) * h / ty - 0.5, 0.0), h - 1)
        y0 = int(np.floor(sy))
        y1, fy = min(y0 + 1, h - 1), sy - y0
        for x in range(tx):
            sx = min(max((x + 0.5) * w / tx - 0.5, 0.0), w - 1)
            x0 = int(np.floor(sx))
            x1, fx = min(x0 + 1, w - 1), sx - x0
            out[y, x] = ((1 - fy) * ((1 - fx) * a[y0, x0] + fx * a[y0, x1])
                         + fy * ((1 - fx) * a[y1, x0] + fx * a[y1, x1]))
    return out


def test_oracle_resampling_matches_brute_force_on_non_integer_ratios():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 65536, size=(1000, 1200)).astype(np.uint16)
    got = rs.downsample(img[None], 128)[0].astype(np.float64)
    want = _area_brute(img.astype(np.float64), 128)
    np.testing.assert_allclose(got, want, rtol=1e-6)
    small = rng.random((128, 128))
    np.testing.assert_allclose(rs.upsample(small, 1000, 1200), _linear_brute(small, 1000, 1200), rtol=1e-12,
                               atol=1e-12)


def test_oracle_recovers_known_fields():
    tiles, flat, dark = rs.synthetic_stack(seed=0)
    f, d, its = rs.fit(tiles)
    ef, ed, eoff = rs.recovery(f, d, flat, dark)
    assert ef <= 0.03  # measured 0.0173 (max |flat error| over the central 80 %)
    assert ed <= 0.35  # measured 0.242 (dark minus its mean, relative to the dark's range of 200 counts)
    assert eoff <= 1.2  # measured 0.94: the constant part of the dark is weakly identified
    assert all(1 <= i <= 500 for i in its)
    f0, d0, _ = rs.fit(tiles, get_darkfield=False)
    assert not d0.any()
    assert rs.recovery(f0, d0, flat, dark)[0] <= 0.12  # measured 0.083: without darkfield it leaks into the flat


@pytest.mark.parametrize("bad, kw", [
    (np.zeros((1, 64, 64), np.uint16), {}),                   # N < 2
    (np.zeros((4, 64, 64), np.uint16), {"working_size": 7}),
    (np.zeros((4, 64, 64), np.uint16), {"working_size": 129}),
    (np.zeros(64, np.uint16), {}),                            # ndim < 2
    (np.zeros((4, 64, 64), np.complex64), {}),                # dtype
    (np.zeros((4, 7, 64), np.uint16), {}),                    # fewer than 8 pixels on a side
])
def test_fit_refusals(bad, kw):
    with pytest.raises(ValueError):
        shading.fit(bad, **kw)
