"""Radial profiles without a GPU: the oracle (tests/radial_ref.py) against an independent float formulation, the
binding of mg_roi_radial_profile, the host-side refusals, quantisation, the marker centres at the image borders, the
helpers on a hand-made table, the pipelines with and without ``profile=``, and mg.save / mg.load of the variables."""
import ctypes
import math

import numpy as np
import pytest

import magnify_amd as mg
import radial_ref as ref
from magnify_amd import _native as nat
from magnify_amd import _dataset, profile, reduce


# ---- the oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L, centre, edges", [
    (16, (7.3, 8.11), [0.0, 1.0, 2.0, 3.5, 7.0, 30.0]),
    (33, (16.0 + 1 / 3, -2.7), [1.3, 2.9, 3.1, 10.7, 20.2]),
    (7, (3.21, 3.33), [0.4, 0.9]),
])
def test_oracle_against_hypot_digitize(L, centre, edges):
    rng = np.random.default_rng(L)
    cq, eq = np.rint(np.array(centre) * 16).astype(np.int64), np.rint(np.array(edges) * 16).astype(np.int64)
    ii, jj = np.mgrid[0:L, 0:L]
    d = np.hypot(ii * 16.0 - cq[0], jj * 16.0 - cq[1])
    assert np.abs(d[..., None] - eq).min() > 1e-9  # no pixel within 1e-9 of an edge: float arithmetic decides the same
    k = np.digitize(d, eq.astype(np.float64)) - 1
    k[(k < 0) | (k >= len(eq) - 1)] = -1
    roi = rng.integers(0, 65535, (1, 2, 1, L, L)).astype(np.uint16)
    mask = rng.random((1, 1, L, L)) > 0.3
    got = ref.profile(roi, mask, cq.reshape(1, 1, 2), eq)
    np.testing.assert_array_equal(got["rings"][0, 0], k)
    for c in range(2):
        for r in range(len(eq) - 1):
            sel = (k == r) & mask[0, 0]
            x = roi[0, c, 0][sel].astype(np.int64)
            assert got["count"][0, c, 0, r] == sel.sum()
            assert got["moments"][0, c, 0, r, 0] == float(x.sum()) and got["moments"][0, c, 0, r, 1] == float((x * x).sum())


def test_oracle_edge_pixels_go_outward_and_nan_is_left_out():
    L, eq = 16, np.arange(0, 9) * 16
    roi = np.zeros((1, 1, 1, L, L), dtype=np.float32)
    roi[0, 0, 0, 8 + 3, 8 + 4] = 5.0   # distance exactly 5: ring 5, not 4
    roi[0, 0, 0, 8 - 4, 8] = 4.0       # exactly 4
    roi[0, 0, 0, 8, 8 - 3] = 3.0       # exactly 3
    roi[0, 0, 0, 8, 8 + 1] = math.nan  # ring 1, left out
    got = ref.profile(roi, None, [[[8 * 16, 8 * 16]]], eq)
    np.testing.assert_array_equal(got["moments"][0, 0, 0, :, 0], [0, 0, 0, 3, 4, 5, 0, 0])
    assert got["count"][0, 0, 0, 1] == 7  # eight pixels at distance 1 .. 1.41, one of them NaN
    assert got["rings"][0, 0, 0, 0] == -1  # the corner at 8 sqrt 2 lies beyond the last edge
    clamped = ref.profile(roi, None, [[[10**6, -10**6]]], eq)
    assert (clamped["rings"] == ref.profile(roi, None, [[[2048 * 16, -1024 * 16]]], eq)["rings"]).all()


# ---- the entry point -------------------------------------------------------------------------------------------------------

def test_entry_point_declared_exported_bound():
    assert len(nat.PROTOTYPES["mg_roi_radial_profile"]) == 17 and nat.RESTYPES["mg_roi_radial_profile"] is ctypes.c_int
    fn = nat.lib().mg_roi_radial_profile
    assert len(fn.argtypes) == 17
    assert (nat.DEFINES["MG_PROFILE_MAX_RINGS"], nat.DEFINES["MG_PROFILE_SUBPIXEL"], nat.DEFINES["MG_PROFILE_MAX_LEN"]) == \
        (128, 16, 1024)
    assert (profile.MAX_RINGS, profile.SUBPIXEL, profile.MAX_LEN) == (128, 16, 1024)
    # judged on the host before anything is launched: these return MG_EINVAL without a device
    e = np.array([0, 16, 32], dtype=np.int32)
    bad = np.array([0, 16, 16], dtype=np.int32)
    far = np.array([0, 16, 46341], dtype=np.int32)
    neg = np.array([-1, 16, 32], dtype=np.int32)
    one = 16  # (never dereferenced: every call below is refused first)

    def call(roi=one, dtype=nat.MG_U16, mask=None, sm=0, st=0, centre=one, csm=0, cst=0, edges=e, r=2, m=1, c=1, t=1, L=4,
             count=one, moments=one):
        return fn(roi, dtype, mask, sm, st, centre, csm, cst, edges.ctypes.data if edges is not None else None, r, m, c,
                  t, L, count, moments, None)

    assert call(roi=None) == -1 and call(centre=None) == -1 and call(edges=None) == -1
    assert call(count=None) == -1 and call(moments=None) == -1
    assert call(dtype=99) == -1 and call(m=-1) == -1 and call(c=0) == -1 and call(t=0) == -1 and call(L=0) == -1
    assert call(L=1025) == -1 and call(r=0) == -1 and call(r=129) == -1
    assert call(edges=bad) == -1 and call(edges=far) == -1 and call(edges=neg) == -1
    assert call(m=2**16, c=2**8, t=2**7) == -1
    assert call(sm=-1) == -1 and call(st=-1) == -1 and call(csm=-1) == -1 and call(cst=-1) == -1
    assert call(m=0) == 0  # no markers: MG_OK, nothing launched


# ---- refusals on the host --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [
    dict(width=0.0), dict(width=-1.0), dict(width=0.03), dict(width=math.nan), dict(width=math.inf), dict(width="1"),
    dict(width=True), dict(width=None),
    dict(rings=0), dict(rings=129), dict(rings=2.0), dict(rings=True), dict(rings="3"),
    dict(width=0.25, roi_length=100),          # ceil(100 / 0.5) = 200 rings by default
    dict(width=30.0, rings=128),               # the last edge at 3840 pixels
    dict(mask=3), dict(mask=np.ones((2, 2), dtype=bool)),
    dict(roi_length=0), dict(roi_length=1025), dict(roi_length=10.0),
    dict(edges=[1.0]), dict(edges=[]), dict(edges=list(range(130))), dict(edges=[0.0, 1.0, 1.0]), dict(edges=[2.0, 1.0]),
    dict(edges=[0.0, 1.0, 1.01]),              # 16 and 16.16: the same sixteenth
    dict(edges=[-0.5, 1.0]), dict(edges=[0.0, 2897.0]), dict(edges=[0.0, math.nan]), dict(edges=[0.0, math.inf]),
    dict(edges=[[0.0, 1.0]]), dict(edges="01"),
])
def test_check_profile_refuses(kw):
    with pytest.raises(ValueError):
        profile.check_profile(**kw)


def test_check_profile_accepts():
    assert profile.check_profile(1.0) is None and profile.check_profile(2, None, None) is None
    np.testing.assert_array_equal(profile.check_profile(1.0, 3), [0, 16, 32, 48])
    assert len(profile.check_profile(1.0, None, "own", 100)) == 51 and len(profile.check_profile(1.0, None, "fg", 7)) == 5
    assert len(profile.check_profile(0.5, 128)) == 129 and profile.check_profile(0.0625, 1)[1] == 1
    np.testing.assert_array_equal(profile.check_profile(edges=[0.0, 2896.25]), [0, 46340])
    assert profile.check_profile(edges=np.array([1, 2, 5])).dtype == np.int32
    for build, kw in ((mg.beads_pipe, {}), (mg.mrbles_pipe, dict(spectra=None, codes=None)), (mg.microfluidic_chip_pipe, {})):
        for bad in (dict(profile=0.0), dict(profile=1.0, profile_rings=0), dict(profile=1.0, profile_mask=5),
                    dict(profile=0.25, roi_length=100)):
            with pytest.raises(ValueError):  # when the pipe is built, not at the first assay
                build(**kw, **bad)


def dataset(m=3, n_c=2, n_t=2, L=8, h=40, w=50, chip=False, seed=0):
    rng = np.random.default_rng(seed)
    coords = {"fg": (("mark", "time", "roi_y", "roi_x"), rng.random((m, n_t, L, L)) > 0.5),
              "bg": (("mark", "time", "roi_y", "roi_x"), rng.random((m, n_t, L, L)) > 0.5),
              "x": (("mark", "time"), rng.uniform(0, w, (m, n_t))), "y": (("mark", "time"), rng.uniform(0, h, (m, n_t)))}
    if chip:
        coords["tag"] = (("mark",), np.array(["a"] * m))
    return mg.Dataset({"roi": mg.DataArray(rng.integers(0, 999, (m, n_c, n_t, L, L)).astype(np.uint16),
                                           ("mark", "channel", "time", "roi_y", "roi_x")),
                       "image": mg.DataArray(np.zeros((n_c, n_t, h, w), dtype=np.uint16), ("channel", "time", "im_y", "im_x"))},
                      coords=coords)


def test_radial_profile_refuses_on_the_host():
    ds = dataset()
    for kw in (dict(width=0.0), dict(rings=200), dict(edges=[1.0, 1.0]), dict(width=0.01), dict(mask=7),
               dict(centre="middle"), dict(centre=np.zeros((3, 3))), dict(centre=np.zeros((2, 2))),
               dict(centre=np.zeros((3, 5, 2))), dict(centre=np.full((3, 2), np.nan)), dict(centre=np.full((3, 2), np.inf))):
        with pytest.raises(ValueError):
            reduce.radial_profile(ds, **kw)
    with pytest.raises(KeyError):
        reduce.radial_profile(ds, mask="no_such_mask", centre="window")
    gone = ds.drop_vars(["image"])  # what roi_only leaves behind knows no image size
    with pytest.raises(ValueError, match="centre="):
        reduce.radial_profile(gone)
    with pytest.raises(ValueError, match="centre="):
        profile.profile_rois(gone)


def test_no_markers_launches_nothing():
    ds = dataset(m=0)
    count, moments = reduce.radial_profile(ds, width=1.0)
    assert count.shape == (0, 2, 2, 4) and count.dtype == np.int32 and count.dims == ("mark", "channel", "time", "ring")
    assert moments.shape == (0, 2, 2, 4, 2) and moments.dims[-1] == "moment"
    assert reduce.radial_profile(ds, time=1)[0].shape == (0, 2, 1, 4)
    out = profile.profile_rois(ds, width=2.0)
    for name in profile.PROFILE_VARS:
        assert out[name].shape == (0, 2, 2, 2) and out[name].dims == ("mark", "channel", "time", "ring")
    np.testing.assert_array_equal(out.coords["ring"].values, [1.0, 3.0])
    np.testing.assert_array_equal(out.coords["ring_inner"].values, [0.0, 2.0])
    np.testing.assert_array_equal(out.coords["ring_outer"].values, [2.0, 4.0])


# ---- quantisation ----------------------------------------------------------------------------------------------------------

def test_quantisation():
    np.testing.assert_array_equal(profile.quantise([0.0, 0.03125, 0.09375, 0.1, 1.0, 2.53, -0.03125, -0.1]),
                                  [0, 0, 2, 2, 16, 40, -0.0, -2])  # rint: halves go to the even sixteenth
    np.testing.assert_array_equal(profile.ring_edges(0.3, 4), np.rint(np.arange(5) * 0.3 * 16))
    np.testing.assert_array_equal(profile.ring_edges(0.3, 4), [0, 5, 10, 14, 19])  # k * width first, then quantised
    np.testing.assert_array_equal(profile.ring_edges(edges=[0.26, 1.49, 7.0]), [4, 24, 112])
    c = profile.ring_coords(np.array([4, 24, 112]))
    np.testing.assert_array_equal(c["ring_inner"], [0.25, 1.5])
    np.testing.assert_array_equal(c["ring_outer"], [1.5, 7.0])
    np.testing.assert_array_equal(c["ring"], [0.875, 4.25])
    assert len(profile.ring_edges(1.0, None, None, 101)) == 52 and len(profile.ring_edges(2.5, None, None, 100)) == 21
    count, _ = reduce.radial_profile(dataset(m=0), edges=[0.26, 1.49, 7.0])
    np.testing.assert_array_equal(count.coords["ring_inner"].values, [0.25, 1.5])  # the quantised values are reported


# ---- centre="marker" -------------------------------------------------------------------------------------------------------

def test_marker_centres_at_the_borders_and_half_pixels():
    h, w, L = 40, 50, 8
    ds = dataset(m=8, n_t=2, L=L, h=h, w=w)
    x = np.array([[1.2, 25.5], [48.7, 26.5], [20.0, 3.5], [20.25, 4.5], [0.0, 49.0], [49.4, 0.4], [25.0, 25.0], [4.0, 46.0]])
    y = np.array([[20.0, 0.3], [20.5, 39.2], [1.0, 21.5], [38.9, 22.5], [0.0, 39.0], [39.4, 0.4], [3.5, 36.5], [4.0, 36.0]])
    ds = ds.assign_coords(x=(("mark", "time"), x), y=(("mark", "time"), y))
    got = _dataset.marker_centres(ds, L, None)
    assert got.shape == (8, 2, 2)
    for g in range(8):
        for t in range(2):
            # Python's round is half-to-even, as the finder's; utils.bounding_box shifts the window into the image
            top = min(max(round(y[g, t]) - L // 2, 0), h - L)
            left = min(max(round(x[g, t]) - L // 2, 0), w - L)
            assert got[g, t, 0] == y[g, t] - top and got[g, t, 1] == x[g, t] - left, (g, t)
    assert got[0, 1, 1] == 25.5 - 22 and got[1, 1, 1] == 26.5 - 22  # 25.5 -> 26, 26.5 -> 26
    assert got[0, 0, 1] == 1.2 and got[1, 0, 1] == 48.7 - 42 and got[2, 0, 0] == 1.0 and got[3, 0, 0] == 38.9 - 32
    np.testing.assert_array_equal(_dataset.marker_centres(ds, L, 1), got[:, 1:2])
    np.testing.assert_array_equal(_dataset.marker_centres(ds, L, -1), got[:, -1:])


# ---- the helpers -----------------------------------------------------------------------------------------------------------

def test_profile_mean_and_std_against_numpy():
    import torch

    rng = np.random.default_rng(3)
    groups = [rng.normal(500, 30, n) for n in (0, 1, 2, 17, 400)]
    count = torch.tensor([[len(g) for g in groups]], dtype=torch.int32)
    moments = torch.tensor([[[g.sum(), (g * g).sum()] for g in groups]], dtype=torch.float64)
    mean, std, std1 = reduce.profile_mean(count, moments), reduce.profile_std(count, moments), reduce.profile_std(count, moments, 1)
    assert mean.shape == (1, 5) and math.isnan(mean[0, 0]) and math.isnan(std[0, 0]) and math.isnan(std1[0, 0])
    assert math.isnan(std1[0, 1]) and std[0, 1] == 0.0
    for i in (1, 2, 3, 4):
        np.testing.assert_allclose(mean[0, i], groups[i].mean(), rtol=1e-14)
    for i in (2, 3, 4):
        np.testing.assert_allclose(std[0, i], groups[i].std(), rtol=1e-9)
        np.testing.assert_allclose(std1[0, i], groups[i].std(ddof=1), rtol=1e-9)
    flat = reduce.profile_std(torch.tensor([3]), torch.tensor([[3 * 0.1, 3 * 0.1 * 0.1]], dtype=torch.float64))
    assert flat[0] >= 0.0  # cancellation never goes below zero
    assert "cancel" in reduce.profile_std.__doc__


# ---- the pipelines ---------------------------------------------------------------------------------------------------------

def test_pipes_with_and_without_profile():
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
        assert [n for n, _ in build(**kw, profile=None).components] == names
        finder = "find_buttons" if build is mg.microfluidic_chip_pipe else "find_beads"
        got = [n for n, _ in build(**kw, profile=1.5, profile_rings=7, profile_mask="fg").components]
        assert got.index("profile_rois") == got.index(finder) + 1 and got.index("profile_rois") < got.index("drop")
        assert [n for n in got if n != "profile_rois"] == names
        got = [n for n, _ in build(**kw, profile=1.0, segment="otsu").components]
        assert got[got.index(finder) + 1:got.index(finder) + 3] == ["segment_rois", "profile_rois"]
        step = dict(build(**kw, profile=1.5, profile_rings=7, profile_mask="fg").components)["profile_rois"]
        assert step.keywords == dict(width=1.5, rings=7, mask="fg")
    import inspect

    for fn in (mg.beads, mg.mrbles, mg.microfluidic_chip, mg.beads_pipe, mg.mrbles_pipe, mg.microfluidic_chip_pipe):
        p = inspect.signature(fn).parameters
        assert (p["profile"].default, p["profile_rings"].default, p["profile_mask"].default) == (None, None, "own")


# ---- save / load -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chip", [False, True])
def test_profile_variables_survive_save_load(tmp_path, chip):
    rng = np.random.default_rng(5)
    m, n_c, n_t, r = 6, 2, 3, 5
    ds = dataset(m=m, n_c=n_c, n_t=n_t, chip=chip)
    ds = ds.assign_coords({k: (("ring",), v) for k, v in profile.ring_coords(profile.ring_edges(1.5, r)).items()})
    dims = ("mark", "channel", "time", "ring")
    ds["profile_count"] = mg.DataArray(rng.integers(0, 99, (m, n_c, n_t, r)).astype(np.int32), dims)
    ds["profile_sum"] = mg.DataArray(rng.random((m, n_c, n_t, r)) * 1e9, dims)
    ds["profile_sumsq"] = mg.DataArray(rng.random((m, n_c, n_t, r)) * 1e18, dims)
    if chip:
        ds = ds.assign_coords(mark_row=(("mark",), np.repeat(np.arange(2), 3)), mark_col=(("mark",), np.tile(np.arange(3), 2)))
        ds._cache["mark_shape"] = (2, 3)
    mg.save(tmp_path / "p.nc", ds)
    back = mg.load(tmp_path / "p.nc")
    for name in profile.PROFILE_VARS:
        assert name in back.data_vars and back[name].dims == dims and back[name].dtype == ds[name].dtype
        np.testing.assert_array_equal(back[name].values, ds[name].values)
    for name in ("ring", "ring_inner", "ring_outer"):
        np.testing.assert_array_equal(back.coords[name].values, ds.coords[name].values)
    # and restore_format: the chip's markers go back to (mark_row, mark_col), the ring axis stays last
    ds.attrs["__original_tile_dims__"] = ["channel", "time", "tile_y", "tile_x"]
    out = mg.postprocess.restore_format(ds)
    want = ("mark_row", "mark_col", "channel", "time", "ring") if chip else dims
    assert out.profile_sum.dims == want
    np.testing.assert_array_equal(out.profile_sum.values.reshape(m, n_c, n_t, r), ds.profile_sum.values)
