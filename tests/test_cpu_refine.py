"""The circle fit without a GPU: the accuracy of the oracle (tests/refine_ref.py) on painted sub-pixel disks, its
status corners, the binding of mg_roi_refine_circles and its refusals, ``check_refine``, the pipelines with and
without ``refine=``, and mg.save / mg.load / restore_format of the new coordinates."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import magnify_amd as mg
import refine_cases as cases
import refine_ref as ref
from magnify_amd import _native as nat
from magnify_amd import hotpath, reduce, refine


# ---- accuracy of the oracle ---------------------------------------------------------------------------------------------------

def test_oracle_accuracy_on_painted_disks():
    """600 painted windows, L = 48, K = 64, reach = 3: every case status 0, centre and radius within 0.25 px of the
    truth, the polarity of its kind.  Seen with this generator: centre worst 0.133 px, radius worst 0.119 px (mostly on
    the low side), at least 39 of 64 rays used."""
    cs = ref.direction_table(64)
    worst_c = worst_r = 0.0
    low = 0
    min_used = 64
    todo = cases.accuracy_cases(600, 48)
    assert len(todo) == 600
    for kind, win, (cy, cx, r), start in todo:
        assert win.shape == (48, 48) and win.dtype == np.uint16
        assert np.abs(start / 16.0 - np.rint([cy, cx, r])).max() <= 1.0
        o = ref.refine_window(win, start, cs, 3, 0, 1.0, 0.25, 32)
        status, n_used, n_valid, pol = o["info"]
        assert status == ref.OK, (kind, cy, cx, r, start, o["info"])
        assert pol == cases.POLARITY[kind], (kind, cy, cx, r, start, o["info"])
        fy, fx, rad = start[0] / 16.0 + o["fit"][0], start[1] / 16.0 + o["fit"][1], math.sqrt(o["fit"][2])
        dc, dr = math.hypot(fy - cy, fx - cx), abs(rad - r)
        worst_c, worst_r, min_used, low = max(worst_c, dc), max(worst_r, dr), min(min_used, n_used), low + (rad < r)
        assert dc <= 0.25 and dr <= 0.25, (kind, cy, cx, r, start, dc, dr)
        assert 32 <= n_used <= n_valid <= 64 and o["kept"].sum() == n_used
    print(f"refine oracle, 600 cases: centre worst {worst_c:.3f} px, radius worst {worst_r:.3f} px "
          f"({low} of 600 below the truth), fewest rays used {min_used}")


def test_oracle_on_a_noiseless_smooth_step():
    """A smooth radial step about a whole-pixel centre: every ray is valid, the fit returns the centre and the radius of
    the steepest change; a forced polarity of the right sign changes nothing, of the wrong sign finds no circle."""
    L, cy, cx, r0 = 40, 20.0, 20.0, 9.0
    ii, jj = np.mgrid[0:L, 0:L].astype(np.float64)
    d = np.hypot(ii - cy, jj - cx)
    win = 1000.0 / (1.0 + np.exp(-(d - r0) / 0.7))  # a smooth step of radius r0, brighter outside
    o = ref.refine_window(win, np.array([320, 320, 9 * 16]), ref.direction_table(64), 3, 0, 1.0, 0.25, 32)
    assert o["info"][0] == 0 and o["info"][3] == 1 and o["info"][1] == 64
    # (the bound of the accuracy test: a noiseless picture is no harder than a noisy one)
    assert math.hypot(o["fit"][0], o["fit"][1]) <= 0.25 and abs(math.sqrt(o["fit"][2]) - r0) <= 0.25
    forced = ref.refine_window(win, np.array([320, 320, 9 * 16]), ref.direction_table(64), 3, 1, 1.0, 0.25, 32)
    np.testing.assert_array_equal(forced["fit"], o["fit"])
    wrong = ref.refine_window(win, np.array([320, 320, 9 * 16]), ref.direction_table(64), 3, -1, 1.0, 0.25, 32)
    assert wrong["info"][0] != 0 and wrong["info"][3] == -1 and np.isnan(wrong["fit"]).all()


def test_oracle_status_corners():
    cs = ref.direction_table(16)
    flat = np.full((17, 17), 7, dtype=np.uint8)
    o = ref.refine_window(flat, [128, 128, 64], cs, 2, 0, 1.0, 0.25, 8)
    assert list(o["info"]) == [ref.TOO_FEW, 0, 0, 1] and np.isnan(o["fit"]).all()  # every e = 0; P+ = P- = 0: +1
    ramp = np.add.outer(np.arange(17), np.arange(17)).astype(np.float32)
    o = ref.refine_window(ramp, [128, 128, 64], cs, 2, 0, 1.0, 0.25, 8)
    # along the axes the samples are exact and the derivatives equal: the first arg-max is the first index, no edge
    assert np.isnan(o["w"][[0, 4, 8, 12]]).all() and np.isnan(o["rho"][[0, 4, 8, 12]]).all() and o["info"][2] <= 12
    outside = ref.refine_window(flat, [-400, 900, 64], cs, 2, 0, 1.0, 0.25, 8)
    assert list(outside["info"]) == [ref.TOO_FEW, 0, 0, 1]
    clamped = ref.refine_window(flat, [10**8, -10**8, 10**8], cs, 2, 0, 1.0, 0.25, 8)
    assert list(clamped["info"]) == [ref.TOO_FEW, 0, 0, 1]
    # a start circle 6 px off at reach 3: no edge in reach of most rays, or a fit that lies out of reach
    rng = np.random.default_rng(1)
    win = cases.paint("bright", 48, 24.0, 24.0, 10.0, rng)
    far = ref.refine_window(win, [(24 + 6) * 16, 24 * 16, 160], ref.direction_table(64), 3, 0, 1.0, 0.25, 32)
    assert far["info"][0] in (ref.TOO_FEW, ref.OUT_OF_REACH) and np.isnan(far["fit"]).all()
    near = ref.refine_window(win, [(24 + 2) * 16, 24 * 16, 160], ref.direction_table(64), 3, 0, 1.0, 0.25, 32)
    assert near["info"][0] == ref.OK and abs(26.0 + near["fit"][0] - 24.0) < 0.25


# ---- the entry point ----------------------------------------------------------------------------------------------------------

def test_entry_point_declared_exported_bound():
    assert len(nat.PROTOTYPES["mg_roi_refine_circles"]) == 20 and nat.RESTYPES["mg_roi_refine_circles"] is ctypes.c_int
    fn = nat.lib().mg_roi_refine_circles
    assert len(fn.argtypes) == 20 and fn.argtypes[14] is ctypes.c_double and fn.argtypes[15] is ctypes.c_double
    assert (nat.DEFINES["MG_REFINE_MAX_RAYS"], nat.DEFINES["MG_REFINE_MAX_REACH"], nat.DEFINES["MG_REFINE_MAX_LEN"]) == \
        (128, 8, 1024)
    assert (refine.MAX_RAYS, refine.MAX_REACH, refine.MAX_LEN, refine.SUBPIXEL) == (128, 8, 1024, 16)
    assert (ref.MAX_RAYS, ref.MAX_REACH, ref.MAX_LEN, ref.SUBPIXEL) == (128, 8, 1024, 16)
    one = 16  # (never dereferenced: every call below is refused first)

    def call(roi=one, dtype=nat.MG_U16, sm=0, st=0, circle=one, csm=0, cst=0, cs=one, k=64, m=1, t=1, L=48, reach=3, pol=0,
             reject=1.0, strength=0.25, min_rays=32, info=one, fit=one):
        return fn(roi, dtype, sm, st, circle, csm, cst, cs, k, m, t, L, reach, pol, reject, strength, min_rays, info, fit,
                  None)

    assert call(roi=None) == -1 and call(circle=None) == -1 and call(cs=None) == -1
    assert call(info=None) == -1 and call(fit=None) == -1
    assert call(dtype=99) == -1 and call(m=-1) == -1 and call(t=0) == -1 and call(L=0) == -1 and call(L=1025) == -1
    assert call(k=7) == -1 and call(k=129) == -1 and call(reach=0) == -1 and call(reach=9) == -1
    assert call(pol=2) == -1 and call(pol=-2) == -1
    assert call(reject=0.0) == -1 and call(reject=-1.0) == -1 and call(reject=math.nan) == -1 and call(reject=math.inf) == -1
    assert call(strength=-0.1) == -1 and call(strength=1.1) == -1 and call(strength=math.nan) == -1
    assert call(min_rays=2) == -1 and call(min_rays=65) == -1
    assert call(m=2**16, t=2**15) == -1
    assert call(sm=-1) == -1 and call(st=-1) == -1 and call(csm=-1) == -1 and call(cst=-1) == -1
    assert call(m=0) == 0 and call(m=0, dtype=99) == -1  # no markers: MG_OK, nothing launched


def test_direction_table_is_the_oracles():
    for k in (8, 64, 128):
        np.testing.assert_array_equal(hotpath.direction_table(k), ref.direction_table(k))
        assert hotpath.direction_table(k).shape == (k, 2) and hotpath.direction_table(k).flags.c_contiguous


# ---- settings and pipes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [
    dict(rays=7), dict(rays=129), dict(rays=64.0), dict(rays=True), dict(rays="64"), dict(rays=None),
    dict(reach=0), dict(reach=9), dict(reach=3.0), dict(reach=None),
    dict(polarity="up"), dict(polarity=2), dict(polarity=-2), dict(polarity=None), dict(polarity=1.0), dict(polarity=True),
    dict(reject=0), dict(reject=-1.0), dict(reject=math.nan), dict(reject=math.inf), dict(reject="1"), dict(reject=None),
    dict(min_strength=-0.01), dict(min_strength=1.01), dict(min_strength=math.nan), dict(min_strength="0.25"),
    dict(min_rays=2), dict(min_rays=65), dict(min_rays=32.0), dict(rays=8, min_rays=9),
    dict(roi_length=0), dict(roi_length=1025), dict(roi_length=48.0),
])
def test_check_refine_refuses(kw):
    with pytest.raises(ValueError):
        refine.check_refine(**kw)


def test_check_refine_accepts():
    assert refine.check_refine() == (64, 3, 0, 1.0, 0.25, 32)
    assert refine.check_refine(8, 1, "brighter", 0.5, 0, 3, 1) == (8, 1, 1, 0.5, 0.0, 3)
    assert refine.check_refine(128, 8, "darker", 2, 1, 128, 1024) == (128, 8, -1, 2.0, 1.0, 128)
    assert refine.check_refine(polarity=-1)[2] == -1 and refine.check_refine(rays=np.int64(9))[5] == 4
    for build, kw in ((mg.beads_pipe, {}), (mg.mrbles_pipe, dict(spectra=None, codes=None)), (mg.microfluidic_chip_pipe, {})):
        for bad in (dict(refine="otsu"), dict(refine=True), dict(refine=1.0), dict(refine="edge", refine_rays=4),
                    dict(refine="edge", refine_reach=0), dict(refine="edge", refine_polarity="both"),
                    dict(refine="edge", roi_length=2000)):
            with pytest.raises(ValueError):  # when the pipe is built, not at the first assay
                build(**kw, **bad)


def test_pipes_with_and_without_refine():
    today = {
        mg.beads_pipe: ["standardize_format", "flatfield_correct", "stitch", "find_beads", "drop", "restore_format"],
        mg.mrbles_pipe: ["standardize_format", "flatfield_correct", "stitch", "find_beads", "identify_mrbles", "drop",
                         "restore_format"],
        mg.microfluidic_chip_pipe: ["standardize_format", "identify_buttons", "stitch", "rotate", "find_buttons", "drop",
                                    "restore_format"],
    }
    for build, names in today.items():
        kw = dict(spectra=None, codes=None) if build is mg.mrbles_pipe else {}
        assert [n for n, _ in build(**kw).components] == names
        assert [n for n, _ in build(**kw, refine=None).components] == names
        finder = "find_buttons" if build is mg.microfluidic_chip_pipe else "find_beads"
        got = [n for n, _ in build(**kw, refine="edge").components]
        assert got.index("refine_markers") == got.index(finder) + 1
        assert [n for n in got if n != "refine_markers"] == names
        got = [n for n, _ in build(**kw, refine="edge", segment="otsu", profile=1.0).components]
        assert got[got.index(finder) + 1:got.index(finder) + 4] == ["refine_markers", "segment_rois", "profile_rois"]
        step = dict(build(**kw, refine="edge").components)["refine_markers"]
        assert step.keywords == dict(channel=None, rays=64, reach=3, polarity="auto")
        step = dict(build(**kw, refine="edge", search_channel=["b", "a"], refine_rays=32, refine_reach=5,
                          refine_polarity="darker").components)["refine_markers"]
        assert step.keywords == dict(channel="b", rays=32, reach=5, polarity="darker")  # the first search channel
        step = dict(build(**kw, refine="edge", search_channel="b", refine_channel=1).components)["refine_markers"]
        assert step.keywords["channel"] == 1
    for fn in (mg.beads, mg.mrbles, mg.microfluidic_chip, mg.beads_pipe, mg.mrbles_pipe, mg.microfluidic_chip_pipe):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("refine", "refine_channel", "refine_rays", "refine_reach", "refine_polarity")] == \
            [None, None, 64, 3, "auto"]
    p = inspect.signature(refine.refine_markers).parameters
    assert [p[k].default for k in ("channel", "rays", "reach", "polarity", "reject", "min_strength", "min_rays")] == \
        [None, 64, 3, "auto", 1.0, 0.25, None]
    assert "refine_markers" in mg.registry.components and "refine" in mg.__all__


# ---- the dataset layer --------------------------------------------------------------------------------------------------------

def dataset(m=3, n_c=2, n_t=2, L=8, h=40, w=50, chip=False, seed=0):
    rng = np.random.default_rng(seed)
    coords = {"fg": (("mark", "time", "roi_y", "roi_x"), rng.random((m, n_t, L, L)) > 0.5),
              "bg": (("mark", "time", "roi_y", "roi_x"), rng.random((m, n_t, L, L)) > 0.5),
              "x": (("mark", "time"), np.rint(rng.uniform(0, w, (m, n_t)))),
              "y": (("mark", "time"), np.rint(rng.uniform(0, h, (m, n_t)))),
              "valid": (("mark", "time"), np.ones((m, n_t), dtype=bool))}
    if chip:
        coords["tag"] = (("mark",), np.array(["a"] * m))
    return mg.Dataset({"roi": mg.DataArray(rng.integers(0, 999, (m, n_c, n_t, L, L)).astype(np.uint16),
                                           ("mark", "channel", "time", "roi_y", "roi_x")),
                       "image": mg.DataArray(np.zeros((n_c, n_t, h, w), dtype=np.uint16), ("channel", "time", "im_y", "im_x"))},
                      coords=coords)


FLOATS, INTS = ("x_fit", "y_fit", "radius_fit", "fit_rms", "fit_strength"), ("fit_rays", "fit_status", "fit_polarity", "radius")


def test_no_markers_adds_empty_coordinates_and_launches_nothing():
    ds = dataset(m=0)
    ds._cache["radius"] = np.zeros(0, dtype=np.int64)
    out = refine.refine_markers(ds)
    assert refine.REFINE_VARS == FLOATS + INTS
    for name in FLOATS:
        assert out.coords[name].shape == (0, 2) and out.coords[name].dims == ("mark", "time")
        assert out.coords[name].dtype == np.float64
    for name in INTS:
        assert out.coords[name].shape == (0, 2) and out.coords[name].dtype == np.int32
    assert set(reduce.refine_circles(ds, circle=np.zeros((0, 3)))) == set(FLOATS + INTS)
    for k in ("x", "y", "fg", "bg", "valid"):
        assert out.coords[k] is ds.coords[k]
    assert out.data_vars["roi"] is ds.data_vars["roi"]


def test_refuses_on_the_host():
    ds = dataset()
    with pytest.raises(ValueError, match="radius="):  # a dataset that no longer carries the finder's radii
        refine.refine_markers(ds)
    with pytest.raises(ValueError, match="radius="):
        reduce.refine_circles(ds)
    for kw in (dict(radius=2.5), dict(radius=[1, 2]), dict(radius=-1), dict(radius=np.ones((3, 5))), dict(radius=math.nan),
               dict(radius="4"), dict(radius=4, rays=4), dict(radius=4, reach=20), dict(radius=4, polarity="in"),
               dict(radius=4, channel="no such channel"), dict(circle="window"), dict(circle=np.zeros((3, 2))),
               dict(circle=np.zeros((2, 3))), dict(circle=np.zeros((3, 5, 3))), dict(circle=np.full((3, 3), np.nan))):
        with pytest.raises((ValueError, KeyError)):
            reduce.refine_circles(ds, **kw)
    gone = ds.drop_vars(["image"])  # what roi_only leaves behind knows no image size
    with pytest.raises(ValueError, match="circle="):
        reduce.refine_circles(gone, radius=4)
    np.testing.assert_array_equal(refine.finder_radius(ds, 4), np.full((3, 2), 4))
    np.testing.assert_array_equal(refine.finder_radius(ds, [1, 2, 3]), [[1, 1], [2, 2], [3, 3]])
    ds._cache["radius"] = np.arange(6).reshape(3, 1, 2)  # a chip's (row, col, time)
    np.testing.assert_array_equal(refine.finder_radius(ds), [[0, 1], [2, 3], [4, 5]])
    ds._cache["radius"] = np.array([7, 8, 9])  # beads
    np.testing.assert_array_equal(refine.finder_radius(ds), [[7, 7], [8, 8], [9, 9]])


@pytest.mark.parametrize("chip", [False, True])
def test_refine_coordinates_survive_save_load_and_restore_format(tmp_path, chip):
    rng = np.random.default_rng(5)
    m, n_t = 6, 3
    ds = dataset(m=m, n_t=n_t, chip=chip)
    new = {k: (("mark", "time"), rng.random((m, n_t)) * 30) for k in FLOATS}
    new["fit_rms"][1][2, 1] = math.nan
    new.update({k: (("mark", "time"), rng.integers(-1, 60, (m, n_t)).astype(np.int32)) for k in INTS})
    ds = ds.assign_coords(new)
    if chip:
        ds = ds.assign_coords(mark_row=(("mark",), np.repeat(np.arange(2), 3)), mark_col=(("mark",), np.tile(np.arange(3), 2)))
        ds._cache["mark_shape"] = (2, 3)
    mg.save(tmp_path / "r.nc", ds)
    back = mg.load(tmp_path / "r.nc")
    for name in FLOATS + INTS:
        assert name in back.coords and back.coords[name].dims == ("mark", "time")
        assert back.coords[name].dtype == ds.coords[name].dtype
        np.testing.assert_array_equal(back.coords[name].values, ds.coords[name].values)
    # the finder's radii travel as a coordinate: a loaded dataset can be refined again without radius=
    np.testing.assert_array_equal(refine.finder_radius(back.assign_coords(radius=(("mark", "time"), np.full((m, n_t), 5)))),
                                  np.full((m, n_t), 5))
    ds.attrs["__original_tile_dims__"] = ["channel", "time", "tile_y", "tile_x"]
    out = mg.postprocess.restore_format(ds)
    want = ("mark_row", "mark_col", "time") if chip else ("mark", "time")
    for name in FLOATS + INTS:
        assert out.coords[name].dims == want, name
        np.testing.assert_array_equal(out.coords[name].values.reshape(m, n_t), ds.coords[name].values)
