"""Hot-pixel removal without a GPU: the NumPy oracle (tests/despeckle_ref.py) against SciPy's median filter and on
hand-made cases, the refusals of ``check_despeckle`` at build time, and the ``despeckle=`` keyword of the builders."""
import inspect

import numpy as np
import pytest

import despeckle_ref as sr
import magnify_amd as mg
from magnify_amd import despeckle

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


# ---- the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_median_is_scipys_nearest_median_filter(dtype):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    for k in (1, 2):
        for h, w in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53)):
            plane, _ = sr.random_planes(rng, dtype, (h, w), specks=0.05)
            want = ndimage.median_filter(plane, size=2 * k + 1, mode="nearest")
            got = sr.median(plane, k)
            assert got.dtype == plane.dtype and np.array_equal(got, want), (k, h, w)


def test_oracle_banded_median_is_the_median():
    rng = np.random.default_rng(2)
    for k in (1, 2):
        for h, w, bands in ((1, 9, 16), (5, 3, 16), (67, 41, 16), (64, 8, 4)):
            plane = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
            assert np.array_equal(sr.median_banded(plane, k, bands), sr.median(plane, k)), (k, h, w)


def test_oracle_by_hand():
    plane = np.array([[1, 2, 3], [4, 90, 6], [7, 8, 9]], dtype=np.uint8)
    # the centre's window is the plane: 1 2 3 4 6 7 8 9 90 -> 6; the corner (0, 0) counts itself four times and its
    # edge neighbours twice: 1 1 1 1 2 2 4 4 90 -> 2
    med = sr.median(plane, 1)
    assert med[1, 1] == 6 and med[0, 0] == 2
    out, count = sr.remove(plane, 1, "bright", 83.5)
    assert count == 1 and out[1, 1] == 6 and np.array_equal(out != plane, np.arange(9).reshape(3, 3) == 4)
    assert sr.remove(plane, 1, "bright", 84)[1] == 0  # 90 - 6 = 84 is not above 84: strict
    assert sr.remove(plane, 1, "dark", 0)[1] == sr.flags(plane, 1, "dark", 0).sum() > 0
    out, count = sr.remove(plane, 1, "all")
    assert count == 9 and np.array_equal(out, med)
    # a defect map replaces exactly its pixels, whatever the threshold
    dmap = np.zeros((3, 3), dtype=np.uint8)
    dmap[0, 0] = 7
    out, count = sr.remove(plane, 1, "bright", 1e9, defects=dmap)
    assert count == 1 and out[0, 0] == 2 and out[1, 1] == 90


def test_oracle_float_specials():
    nan, inf = np.nan, np.inf
    plane = np.array([[1.0, 2.0, 3.0], [4.0, nan, inf], [7.0, 8.0, 9.0]], dtype=np.float32)
    med = sr.median(plane, 1)
    assert med[1, 1] == 7.0  # 1 2 3 4 7 8 9 inf nan: NaN sorts last, +inf before it
    out, count = sr.remove(plane, 1, "both", 0.0)
    assert np.isnan(out[1, 1])  # a NaN pixel is kept
    assert out[1, 2] == med[1, 2] == 9.0  # +inf over a finite median (2 3 3 8 9 9 inf inf nan) goes
    mostly = np.full((3, 3), nan, dtype=np.float64)
    mostly[0, 1], mostly[1, 1] = 5.0, inf  # at most three of any window's nine are numbers
    assert np.isnan(sr.median(mostly, 1)).all()
    out, count = sr.remove(mostly, 1, "both", 0.0)
    assert count == 0 and sr.same(out, mostly)  # a NaN median leaves every pixel alone
    infs = np.full((3, 3), inf)
    assert sr.remove(infs, 1, "both", 0.0)[1] == 0  # inf - inf is NaN: kept
    assert sr.same(np.float32([0.0, nan]), np.float32([-0.0, nan])) and not sr.same(np.float32([1]), np.float64([1]))


def test_oracle_votes_and_map():
    block = np.full((4, 5, 5), 10, dtype=np.uint16)
    block[:, 2, 2] = 500      # in every plane
    block[:2, 0, 4] = 500     # in half of them
    block[3, 4, 0] = 500      # in one
    v = sr.votes(block, 1, "bright", 100)
    assert v.dtype == np.int32 and v[2, 2] == 4 and v[0, 4] == 2 and v[4, 0] == 1 and v.sum() == 7
    assert sr.defect_map(block, 1, "bright", 100, 0.5).sum() == 2
    assert sr.defect_map(block, 1, "bright", 100, 1.0).sum() == 1
    assert sr.defect_map(block, 1, "bright", 100, 0.01).sum() == 3


# ---- the settings ----------------------------------------------------------------------------------------------------

BAD = [dict(despeckle=True), dict(despeckle="500"), dict(despeckle=float("nan")), dict(despeckle=float("inf")),
       dict(despeckle=-1), dict(despeckle=-0.5), dict(despeckle=5, despeckle_radius=0), dict(despeckle=5, despeckle_radius=3),
       dict(despeckle=5, despeckle_radius=1.0), dict(despeckle=5, despeckle_radius=True),
       dict(despeckle=5, despeckle_which="all"), dict(despeckle=5, despeckle_which="hot"), dict(despeckle=5, despeckle_which=None),
       dict(despeckle=5, despeckle_scope="chip"), dict(despeckle=5, despeckle_scope=None)]

BUILDERS = {
    "beads_pipe": ({}, ["standardize_format", "flatfield_correct", "stitch", "find_beads", "drop", "restore_format"]),
    "mrbles_pipe": (dict(spectra="s.csv", codes="c.csv"),
                    ["standardize_format", "flatfield_correct", "stitch", "find_beads", "identify_mrbles", "drop",
                     "restore_format"]),
    "microfluidic_chip_pipe": ({}, ["standardize_format", "identify_buttons", "stitch", "rotate", "find_buttons", "drop",
                                    "restore_format"]),
    "image_pipe": ({}, ["standardize_format", "stitch", "rotate", "drop", "restore_format"]),
}


def test_check_despeckle_refusals():
    despeckle.check_despeckle(0)
    despeckle.check_despeckle(np.float32(2.5), np.int64(2), "both", "sensor", 1)
    for threshold in (True, "5", None, float("nan"), float("inf"), -1, -1e-9, 1j):
        with pytest.raises(ValueError, match="threshold"):
            despeckle.check_despeckle(threshold)
    for radius in (0, 3, 1.0, True, "1", None):
        with pytest.raises(ValueError, match="radius"):
            despeckle.check_despeckle(5, radius)
    for which in ("all", "hot", None, 0):
        with pytest.raises(ValueError, match="which"):
            despeckle.check_despeckle(5, 1, which)
    for scope in ("chip", None, 1):
        with pytest.raises(ValueError, match="scope"):
            despeckle.check_despeckle(5, 1, "bright", scope)
    for fraction in (0, -0.5, 1.01, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="min_fraction"):
            despeckle.check_despeckle(5, 1, "bright", "plane", fraction)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_builders_take_despeckle(name):
    kw, stages = BUILDERS[name]
    build = getattr(mg, name)
    for fn in (build, getattr(mg, name[:-len("_pipe")])):  # the defaults in the eight signatures
        params = inspect.signature(fn).parameters
        assert params["despeckle"].default is None and params["despeckle_radius"].default == 1
        assert params["despeckle_which"].default == "bright" and params["despeckle_scope"].default == "plane"
    pipe = build(**kw)
    assert [n for n, _ in pipe.components] == stages  # despeckle=None: the stages of today
    pipe = build(despeckle=500, **kw)
    assert [n for n, _ in pipe.components] == stages[:1] + ["remove_outliers"] + stages[1:]
    assert pipe.components[1][1].keywords == dict(threshold=500, radius=1, which="bright", scope="plane")
    pipe = build(despeckle=2.5, despeckle_radius=2, despeckle_which="both", despeckle_scope="sensor", depth="max", **kw)
    assert [n for n, _ in pipe.components] == ["project_depth"] + stages[:1] + ["remove_outliers"] + stages[1:]
    assert pipe.components[2][1].keywords == dict(threshold=2.5, radius=2, which="both", scope="sensor")
    for bad in BAD:  # refused when the pipeline is built
        with pytest.raises(ValueError):
            build(**bad, **kw)


def test_component_is_registered_and_checks_before_any_launch():
    assert "remove_outliers" in mg.components.get_all() and mg.despeckle is despeckle
    assert list(inspect.signature(mg.components.get("remove_outliers")).parameters) == [
        "threshold", "radius", "which", "scope", "min_fraction"]
    assert despeckle.TILE >= 1 and despeckle.MAX_K == 2 and despeckle.RADII == (1, 2)
    flat = mg.DataArray(np.zeros((4, 5), np.uint16), ("y", "x"))
    with pytest.raises(ValueError, match="threshold"):
        despeckle.remove_outliers_component(flat, -1)
    with pytest.raises(ValueError, match="min_fraction"):
        despeckle.remove_outliers_component(flat, 5, scope="sensor", min_fraction=0)
    with pytest.raises(ValueError, match="page dimensions"):
        despeckle.remove_outliers_component(mg.DataArray(np.zeros((4, 5), np.uint16), ("a", "b")), 5)
    with pytest.raises(ValueError, match="tile"):
        despeckle.remove_outliers_component(mg.Dataset({"image": flat}), 5)
    with pytest.raises(TypeError):
        despeckle.median(np.zeros((4, 5), np.uint16))
    with pytest.raises(ValueError, match="radius"):
        despeckle.median(np.zeros((4, 5), np.uint16), 3)
