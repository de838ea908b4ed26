"""Background subtraction without a GPU: the NumPy oracle (tests/background_ref.py) against SciPy's grey opening and on
hand-made cases, the refusals of ``check_background`` at build time, and the ``background=`` keyword of the builders."""
import inspect

import numpy as np
import pytest

import background_ref as br
import despeckle_ref as sr
import magnify_amd as mg
from magnify_amd import background

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


def random_plane(rng, dtype, shape):
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    return rng.normal(-100.0, 50.0, size=shape).astype(dtype)


# ---- the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_opening_is_scipys_nearest_grey_opening(dtype):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    for h, w in ((1, 1), (3, 70), (37, 5), (65, 130), (2, 9)):
        plane = random_plane(rng, dtype, (h, w))
        for radius in (1, 4, 9, 32):  # h or w below the radius among them
            want = ndimage.grey_opening(plane, size=2 * radius + 1, mode="nearest")
            got = br.opening(plane, radius)
            assert got.dtype == plane.dtype and np.array_equal(got, want), (radius, h, w)
            assert np.array_equal(br.estimate(plane, radius), want)
            assert (got <= plane).all() and np.array_equal(br.subtract(plane, radius), plane - want)
            if dtype is np.uint8:
                assert np.array_equal(br.opening_by_shifts(plane, radius), want), (radius, h, w)


def test_oracle_by_hand():
    line = np.array([[5, 5, 9, 5, 5, 1, 5, 5, 7, 7, 7, 5]], dtype=np.uint16)
    # radius 1: the single 9 does not fit a window of 3 and goes, the run of three 7s fits and stays; the 1 stays a pit
    assert br.erode(line, 1).tolist() == [[5, 5, 5, 5, 1, 1, 1, 5, 5, 7, 5, 5]]
    assert br.opening(line, 1).tolist() == [[5, 5, 5, 5, 5, 1, 5, 5, 7, 7, 7, 5]]
    assert br.subtract(line, 1).tolist() == [[0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert br.erode(line, 2).tolist() == [[5, 5, 5, 1, 1, 1, 1, 1, 5, 5, 5, 5]]
    assert br.opening(line, 2).tolist() == [[5, 5, 5, 5, 5, 1, 5, 5, 5, 5, 5, 5]]  # a window of 5: the 7s go too
    # a dark pixel spreads to exactly its (2R + 1)^2 neighbourhood in E; in B it is back where it was, and still there
    plane = np.full((9, 11), 100, dtype=np.uint8)
    plane[4, 6] = 3
    e = br.erode(plane, 2)
    yy, xx = np.mgrid[0:9, 0:11]
    assert np.array_equal(e == 3, (abs(yy - 4) <= 2) & (abs(xx - 6) <= 2)) and np.array_equal(br.opening(plane, 2), plane)
    plane[:] = 100
    plane[4, 6] = 200  # a bright one is gone
    assert (br.opening(plane, 2) == 100).all() and br.subtract(plane, 2).sum() == 100


def test_oracle_nan_rules():
    nan, inf = np.nan, np.inf
    plane = np.full((7, 9), 10.0, dtype=np.float32)
    plane[3, 4] = nan
    assert np.array_equal(br.opening(plane, 1), np.full((7, 9), 10.0, dtype=np.float32))  # ignored in every window
    out = br.subtract(plane, 1)
    assert np.isnan(out[3, 4]) and np.nansum(out) == 0 and np.isnan(out).sum() == 1  # P - B is NaN where P is
    plane[1:6, 2:7] = nan  # the windows of radius 1 around the inner 3 x 3 have nothing left
    e = br.erode(plane, 1)
    assert np.array_equal(np.isnan(e), np.pad(np.ones((3, 3), bool), ((2, 2), (3, 3))))
    b = br.opening(plane, 1)
    assert np.isnan(b[3, 4]) and np.isnan(b).sum() == 1  # every other window of E holds a number
    assert np.isnan(br.subtract(plane, 1)).sum() == 25
    assert np.isnan(br.opening(np.full((3, 3), nan), 1)).all()
    spec = np.array([[1.0, inf, -inf, 0.0, -0.0, nan, 5.0]])
    assert br.same(br.erode(spec, 1), np.array([[1.0, -inf, -inf, -inf, 0.0, 0.0, 5.0]]))
    assert br.same(br.opening(spec, 1), np.array([[1.0, 1.0, -inf, 0.0, 0.0, 5.0, 5.0]]))
    assert br.same(br.minus(np.array([inf, inf, 1.0, nan]), np.array([inf, 1.0, nan, 1.0])), np.array([0.0, inf, nan, nan]))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_oracle_clamp_engages_with_smoothing(dtype):
    rng = np.random.default_rng(3)
    plane = random_plane(rng, dtype, (40, 50))
    for smooth in (1, 2):
        b = br.estimate(plane, 3, smooth)
        assert np.array_equal(b, br.opening(sr.median(plane, smooth), 3))
        above = b > plane
        assert 0.1 < above.mean() < 0.6  # about a third of the pixels
        out = br.subtract(plane, 3, smooth)
        assert (out[above] == 0).all() and np.array_equal(out[~above], (plane - b)[~above])
    assert not (br.estimate(plane, 3) > plane).any()


# ---- the settings ----------------------------------------------------------------------------------------------------

BAD = [dict(background=True), dict(background=0), dict(background=129), dict(background=2.5), dict(background="16"),
       dict(background=-1), dict(background=16, background_smooth=3), dict(background=16, background_smooth=-1),
       dict(background=16, background_smooth=True), dict(background=16, background_smooth=1.0),
       dict(background=16, background_smooth=None), dict(background=16, background_channel=True),
       dict(background=16, background_channel=[]), dict(background=16, background_channel=["a", 2.5])]

BUILDERS = {
    "beads_pipe": ({}, ["standardize_format", "flatfield_correct", "stitch", "find_beads", "drop", "restore_format"], "stitch"),
    "mrbles_pipe": (dict(spectra="s.csv", codes="c.csv"),
                    ["standardize_format", "flatfield_correct", "stitch", "find_beads", "identify_mrbles", "drop",
                     "restore_format"], "stitch"),
    "microfluidic_chip_pipe": ({}, ["standardize_format", "identify_buttons", "stitch", "rotate", "find_buttons", "drop",
                                    "restore_format"], "rotate"),
    "image_pipe": ({}, ["standardize_format", "stitch", "rotate", "drop", "restore_format"], "stitch"),
}


def test_check_background_refusals():
    background.check_background(1)
    background.check_background(np.int64(128), np.int32(2), "bf")
    background.check_background(16, 0, ["bf", "cy5", 0])
    for radius in (True, False, 0, 129, 2.5, -3, "16", None, 16.0, np.float32(4)):
        with pytest.raises(ValueError, match="radius"):
            background.check_background(radius)
    for smooth in (-1, 3, True, 1.0, "1", None):
        with pytest.raises(ValueError, match="smooth"):
            background.check_background(16, smooth)
    for channel in (True, [], 2.5, ["bf", None], [["bf"]]):
        with pytest.raises(ValueError, match="channel"):
            background.check_background(16, 0, channel)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_builders_take_background(name):
    kw, stages, anchor = BUILDERS[name]
    build = getattr(mg, name)
    for fn in (build, getattr(mg, name[:-len("_pipe")])):  # the defaults in the eight signatures
        params = inspect.signature(fn).parameters
        assert params["background"].default is None and params["background_smooth"].default == 0
        assert params["background_channel"].default is None
    pipe = build(**kw)
    assert [n for n, _ in pipe.components] == stages  # background=None: the stages of today
    at = stages.index(anchor) + 1
    with_it = stages[:at] + ["subtract_background"] + stages[at:]
    pipe = build(background=16, **kw)
    assert [n for n, _ in pipe.components] == with_it
    assert pipe.components[at][1].keywords == dict(radius=16, smooth=0, channel=None)
    pipe = build(background=40, background_smooth=2, background_channel=["bf", "cy5"], depth="max", despeckle=500, **kw)
    assert [n for n, _ in pipe.components] == ["project_depth", with_it[0], "remove_outliers"] + with_it[1:]
    assert pipe.components[at + 2][1].keywords == dict(radius=40, smooth=2, channel=["bf", "cy5"])
    for bad in BAD:  # refused when the pipeline is built
        with pytest.raises(ValueError):
            build(**bad, **kw)


def test_component_is_registered_and_checks_before_any_launch():
    assert "subtract_background" in mg.components.get_all() and mg.background is background and "background" in mg.__all__
    assert list(inspect.signature(mg.components.get("subtract_background")).parameters) == ["radius", "smooth", "channel"]
    assert background.MAX_RADIUS == 128 and background.ROWS >= 1 and background.COLS >= 1 and background.SPAN >= 1
    flat = mg.DataArray(np.zeros((4, 5), np.uint16), ("y", "x"))
    with pytest.raises(ValueError, match="radius"):
        background.subtract_background(flat, 0)
    with pytest.raises(ValueError, match="smooth"):
        background.subtract_background(flat, 4, smooth=3)
    with pytest.raises(ValueError, match="page dimensions"):
        background.subtract_background(mg.DataArray(np.zeros((4, 5), np.uint16), ("a", "b")), 4)
    with pytest.raises(ValueError, match="image"):
        background.subtract_background(mg.Dataset({"tile": flat}), 4)
    stack = mg.DataArray(np.zeros((2, 4, 5), np.uint16), ("channel", "im_y", "im_x"), coords={"channel": ["bf", "cy5"]})
    with pytest.raises(ValueError, match="not found"):
        background.subtract_background(stack, 4, channel="egfp")
    with pytest.raises(ValueError, match="not found"):
        background.subtract_background(mg.Dataset({"image": stack}), 4, channel=["bf", "egfp"])
    with pytest.raises(ValueError, match="channel"):
        background.subtract_background(flat, 4, channel="bf")
    for fn in (background.estimate, background.subtract):
        with pytest.raises(TypeError):
            fn(np.zeros((4, 5), np.uint16), 4)
        with pytest.raises(ValueError, match="radius"):
            fn(np.zeros((4, 5), np.uint16), 129)
