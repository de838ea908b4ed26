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


# ---- anchors of the mirrored, staged restatement (ref_shading.alm_stages and friends): it must be the model where its
# float32 roundings are off, and the inputs of tests/test_gpu_shading_stages.py must meet the conditions stated there.


def _chain(D, k, get_darkfield, round32):
    c = rs.Consts(D.astype(np.float64), get_darkfield)
    st, outs = rs.fresh_state(c), []
    for _ in range(k):
        outs.append(rs.alm_stages(st, D, np.ones_like(D), c, get_darkfield, round32=round32))
        st = rs.next_state(outs[-1])
    return c, st, outs


@pytest.mark.parametrize("get_darkfield", [True, False])
def test_alm_stages_without_float32_is_the_oracle(get_darkfield):
    tiles = rs.synthetic_stack(n=8, size=64, seed=2)[0]
    D = rs.downsample_exact(tiles, 33)
    c, st, _ = _chain(D, 10, get_darkfield, round32=False)
    ref = rs.State(c)
    for _ in range(10):
        ratio = rs.alm_step(ref, D.astype(np.float64), np.ones(D.shape), c)
    for name, want in (("What", ref.W_hat), ("Fw", ref.F_w), ("Aoff", ref.A_off), ("coeff", ref.coeff), ("E", ref.E),
                       ("Y", ref.Y), ("B1", ref.B1_off), ("mu", ref.mu)):
        got = np.asarray(st[name], np.float64)
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), name
    assert st["iterations"] == 10 and (ref.coeff < 1).any() and (ref.coeff >= 1).any()
    if get_darkfield:
        assert np.abs(ref.A_off).max() > 0 and ref.B1_off > 0  # the darkfield step ran and was compared
    else:
        assert not ref.A_off.any()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("ty, tx, w", [(8, 8, 8), (129, 128, 128), (300, 211, 100), (8, 13, 1), (17, 40, 8)])
def test_downsample_exact_is_the_oracle_downsample(dtype, ty, tx, w):
    rng = np.random.default_rng(ty)
    tiles = rng.integers(0, 256 if dtype == np.uint8 else 65536, size=(3, ty, tx)).astype(dtype)
    got, want = rs.downsample_exact(tiles, w), rs.downsample(tiles, w)
    assert got.dtype == np.float32
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)))
    assert (rs.overlap_matrix(ty, w).sum(1) == ty).all() and (rs.overlap_matrix(tx, w).sum(1) == tx).all()


@pytest.mark.parametrize("w, ty, tx", [(8, 8, 8), (8, 37, 301), (100, 300, 211), (1, 9, 9)])
def test_upsample_fields_is_the_oracle_full_fields(w, ty, tx):
    rng = np.random.default_rng(w)
    flat_w, dark_w = 1 + 0.3 * rng.random((w, w)), 100 * rng.standard_normal((w, w))
    for got, want in zip(rs.upsample_fields(flat_w, dark_w, ty, tx), rs.full_fields(flat_w, dark_w, ty, tx)):
        assert got.dtype == np.float32
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
def test_apply_mirrored_is_the_oracle_apply_in_range(dtype):
    rng = np.random.default_rng(5)
    top = 255 if dtype == np.uint8 else 65535
    tiles = rng.integers(0, top + 1, size=(4, 19, 37)).astype(dtype)
    flat = (0.5 + rng.random((19, 37))).astype(np.float32)
    dark = (0.2 * top * rng.random((19, 37))).astype(np.float32)
    got, want = rs.apply_mirrored(tiles, flat, dark), rs.apply(tiles, flat, dark)
    assert got.dtype == want.dtype == dtype
    np.testing.assert_array_equal(got, want)
    if np.dtype(dtype).kind == "u":
        assert (got == 0).any() and (got == top).any()  # both clamps took part


def test_apply_mirrored_special_values():
    flat = np.array([1.0, 1e-30, -1.0, 0.0, 0.0, 1.0], np.float32)
    dark = np.array([9.0, 0.0, 0.0, 5.0, 1.0, 0.0], np.float32)
    x = np.array([5, 7, 7, 5, 5, 65535], np.uint16)
    # dark above the pixel, a tiny flat, a negative flat, 0 / 0 (NaN), x / 0 (+inf), the largest pixel
    np.testing.assert_array_equal(rs.apply_mirrored(x, flat, dark), [0, 65535, 0, 0, 65535, 65535])
    xf = np.array([np.nan, np.inf, -np.inf, 5.0, 5.0, 1.0], np.float32)
    got = rs.apply_mirrored(xf, flat, dark)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == np.inf and np.isnan(got[3]) and got[4] == np.inf


@pytest.mark.parametrize("w", [1, 2, 3, 8, 24, 33, 50, 64, 96, 100, 127, 128])
def test_cos_table_bound_holds_for_the_float64_table(w):
    k, x = np.mgrid[0:w, 0:w]
    a = np.where(k == 0, np.sqrt(1.0 / w), np.sqrt(2.0 / w))
    c64 = a * np.cos(np.pi * ((2 * x + 1) * k).astype(np.float64) / (2.0 * w))
    c = rs.cos_table(w)
    assert np.all(np.abs(c64 - c) <= rs.cos_table_bound(w))
    assert np.abs((c @ c.T).astype(np.float64) - np.eye(w)).max() <= 1e-17 * w  # orthonormal in extended precision
    if w > 1:
        from scipy.fft import dctn

        xx = np.random.default_rng(w).standard_normal((w, w))
        assert np.abs((c @ xx.astype(rs.LD) @ c.T).astype(np.float64) - dctn(xx, norm="ortho")).max() <= 1e-13


@pytest.mark.parametrize("name", list(rs.STAGE_CASES))
def test_stage_inputs_meet_their_conditions(name):
    kind, w, k0 = rs.STAGE_CASES[name]
    tiles = rs.stage_tiles(kind)
    D = rs.downsample_exact(tiles, w)
    n, P = D.shape[0], w * w
    _, _, coeffs = rs.run_oracle(D, k0 + 1)
    below = [int((c < 1).sum()) for c in coeffs]
    if name == "n2_w50_fresh":
        assert below == [0]  # the darkfield step is skipped in iteration 1 ...
    elif name == "n2_w50_k1":
        assert below == [0, 1]  # ... and runs in iteration 2: the skip-dark word is set, then cleared
    elif k0 > 0:
        # the snapshot (and the iteration under test) has images on both sides of coeff = 1; a fresh state has
        # coeff = 1 everywhere by construction
        assert all(0 < b < n for b in below[-2:]), below
    margins = np.abs(np.concatenate(coeffs[-2:]) - 1)
    assert margins.min() > 1e-3  # no image so close to coeff = 1 that the float32 E could move it across
    if name == "n5_w33_k7":
        assert P % 1024 != 0 and P > 1024 and P % 256 != 0
    if name == "n300_w24_k3":
        assert n > 256 and min(below[-2:]) > 100
    if name == "n8_w1_k2":
        assert P == 1


@pytest.mark.parametrize("name", list(rs.FIT_CASES))
def test_fit_inputs_stop_away_from_the_tolerance(name):
    (flat, dark, its), (mflat, mdark, mits, ratios) = rs.fit_three_ways(name)
    assert its == mits and len(its) >= 2
    for before, last in ratios:
        assert before > 1.01e-6 and last < 0.99e-6, ratios  # the device cannot stop an iteration off
    assert np.isfinite(mflat).all() and np.isfinite(mdark).all()
    assert np.abs(mflat - flat).max() < 1e-6  # the float32 E, Y and weights move the flat by less than the floor
    if rs.FIT_CASES[name][1].get("get_darkfield", True):
        assert np.abs(mdark).max() > 0
    else:
        assert not mdark.any()
