"""Per-pixel unmixing without a GPU: the oracle (tests/unmix_ref.py) against an independent route (the reference's
per-bead least squares), what the feature is for (a bead with a brightness falloff and hot pixels), the settings and
definitions of magnify_amd.unmix, the refusals of the Python layer and of the two entry points, and the binding."""
import ctypes
import math

import numpy as np
import pytest

import magnify_amd as mg
import unmix_ref as ref
from magnify_amd import _native as nat
from magnify_amd import hotpath, reduce, unmix

SPECTRA = np.array([[1.0, 0.2, 0.05, 0.0], [0.1, 1.0, 0.3, 0.02], [0.0, 0.25, 1.0, 0.4]])  # (lanthanide, channel)


def disk(L, r):
    ii, jj = np.mgrid[0:L, 0:L]
    return (ii - L // 2) ** 2 + (jj - L // 2) ** 2 <= r * r


# ---- the oracle against an independent route ----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_mean_of_pixel_volumes_is_the_reference_expression(seed):
    """Unmixing is linear: with offset = bg median and a full-rank table the masked mean of the per-pixel volumes is
    lstsq(sp.T, (fg mean - bg median).T), up to the rounding of two float64 routes.  (Measured here over the four seeds:
    the largest relative difference is below 2e-14; the volumes are some hundreds, none near zero.)"""
    rng = np.random.default_rng(seed)
    m, L = 4, 21
    fg = np.broadcast_to(disk(L, 7), (m, 1, L, L))
    bg = ~np.broadcast_to(disk(L, 9), (m, 1, L, L))
    vols = rng.uniform(200, 900, (m, 3))
    roi = rng.integers(90, 111, (m, 4, 1, L, L)).astype(np.float64)
    fall = rng.uniform(0.5, 1.0, (m, 1, 1, L, L))
    roi = np.where(fg[:, None], roi + fall * (vols @ SPECTRA)[:, :, None, None, None], roi)
    roi = np.rint(roi).astype(np.uint16)
    w = unmix.unmixing_matrix(SPECTRA)
    off = ref.nanmedian_windows(roi, bg)
    count, total, _, _ = ref.roi_unmix_stats(roi, fg, [0, 1, 2, 3], w, off)
    assert (count == disk(L, 7).sum()).all()
    mean_v = total[:, 0, :3] / count[:, 0, :3]
    fg_mean = np.stack([[roi[g, c, 0][fg[g, 0]].astype(np.float64).mean() for c in range(4)] for g in range(m)])
    want = np.linalg.lstsq(SPECTRA.T, (fg_mean - off[:, :, 0]).T, rcond=None)[0].T
    assert np.abs(want).min() > 100
    print("largest relative difference:", np.abs(mean_v / want - 1).max())
    np.testing.assert_allclose(mean_v, want, rtol=1e-10, atol=0)


def test_median_of_pixel_ratios_ignores_falloff_and_hot_pixels():
    """Why the feature exists.  Every pixel of the bead has the true ratio, under a brightness falloff towards the rim;
    three hot pixels sit in one channel.  The per-pixel median ratio is the true ratio to 1e-12; the reference's
    mean-based ratio is off by more than 1 % (here: the hot pixels add 3 * 60000 / 317 = 568 to a channel mean of some
    hundreds)."""
    L, r = 31, 10
    fg = disk(L, r)[None, None]
    ii, jj = np.mgrid[0:L, 0:L]
    fall = 1.0 - 0.6 * ((ii - L // 2) ** 2 + (jj - L // 2) ** 2) / float(r * r)  # 1 in the middle, 0.4 at the rim
    true = np.array([700.0, 350.0, 140.0])
    inten = true @ SPECTRA  # per channel
    roi = np.full((1, 4, 1, L, L), 100.0)
    roi[0, :, 0] += np.where(fg[0, 0], fall, 0.0)[None] * inten[:, None, None]
    for y, x in ((15, 15), (12, 18), (20, 13)):
        assert fg[0, 0, y, x]
        roi[0, 1, 0, y, x] += 60000.0
    off = np.full((1, 4, 1), 100.0)
    w = unmix.unmixing_matrix(SPECTRA)
    count, _, order, _ = ref.roi_unmix_stats(roi, fg, [0, 1, 2, 3], w, off, q=(0.5,))
    median_ratio = ref.interpolate(count, order, (0.5,))[0, 0, 3:, 0]
    np.testing.assert_allclose(median_ratio, true[1:] / true[0], rtol=1e-12, atol=0)
    fg_mean = np.array([roi[0, c, 0][fg[0, 0]].mean() for c in range(4)]) - 100.0
    v = np.linalg.lstsq(SPECTRA.T, fg_mean, rcond=None)[0]
    mean_ratio = v[1:] / v[0]
    assert (np.abs(mean_ratio / (true[1:] / true[0]) - 1.0) > 0.01).all(), mean_ratio
    # without the hot pixels the mean-based ratio is right: they alone account for the error
    clean = roi.copy()
    clean[0, 1, 0][[15, 12, 20], [15, 18, 13]] -= 60000.0
    fg_mean = np.array([clean[0, c, 0][fg[0, 0]].mean() for c in range(4)]) - 100.0
    v = np.linalg.lstsq(SPECTRA.T, fg_mean, rcond=None)[0]
    np.testing.assert_allclose(v[1:] / v[0], true[1:] / true[0], rtol=1e-9)


def test_oracle_order_and_left_to_right_sums():
    # -0.0 sorts below +0.0; NaN drops out; +-inf stay; the volumes are summed left to right
    s = ref.sorted_values(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -0.0]))
    assert s.tobytes() == np.array([-np.inf, -0.0, -0.0, 0.0, 1.0, np.inf]).tobytes()
    x = np.array([[1e16], [1.0], [-1e16]])
    assert ref.volumes(x, np.ones((1, 3)))[0, 0] == 0.0  # (1e16 + 1) - 1e16 in float64; right to left would give 1
    assert ref.volumes(x[::-1], np.ones((1, 3)))[0, 0] == 0.0 and ref.volumes(x[[0, 2, 1]], np.ones((1, 3)))[0, 0] == 1.0
    d = ref.derived(np.array([[0.0, 2.0, 0.0]]), np.array([[1.0], [3.0]]))
    assert np.isnan(d[2, 0]) and d[2, 1] == 3.0 and d.shape == (3, 3)
    roi = np.zeros((1, 1, 1, 2, 2))
    count, total, order, _ = ref.roi_unmix_stats(roi, None, [0], np.array([[1.0], [2.0]]), None, (0.5,))
    assert count[0, 0].tolist() == [4, 4, 0] and np.isnan(order[0, 0, 2]).all() and total[0, 0, 2] == 0.0
    assert ref.order_pairs(np.arange(5.0), (0, 0.25, 0.5, 0.6, 1)).tolist() == [[0, 1], [1, 2], [2, 3], [2, 3], [4, 4]]


# ---- settings and definitions -------------------------------------------------------------------------------------------

def test_check_unmix():
    assert unmix.check_unmix(None) is None and unmix.check_unmix("pixel") == "pixel"
    for bad in ("voxel", "", "Pixel", 1, True, 0.5, ["pixel"], b"pixel"):
        with pytest.raises(ValueError):
            unmix.check_unmix(bad)
    for bad in ("voxel", 3):
        with pytest.raises(ValueError):  # when the pipe is built, not at the first assay
            mg.mrbles_pipe(spectra=None, codes=None, unmix=bad)
    steps = dict(mg.mrbles_pipe(spectra="s.csv", codes="c.csv", unmix="pixel").components)
    assert steps["identify_mrbles"].keywords["unmix"] == "pixel"
    assert dict(mg.mrbles_pipe(spectra="s.csv", codes="c.csv").components)["identify_mrbles"].keywords["unmix"] is None
    import inspect

    for f in (mg.mrbles, mg.mrbles_pipe, mg.identify.identify_mrbles):
        assert inspect.signature(f).parameters["unmix"].default is None
    assert mg.unmix is unmix and "unmix" in mg.__all__


def test_unmixing_matrix():
    w = unmix.unmixing_matrix(SPECTRA)
    assert w.shape == (3, 4) and w.dtype == np.float64 and w.flags.c_contiguous
    np.testing.assert_allclose(w @ SPECTRA.T, np.eye(3), atol=1e-12)
    inten = np.random.default_rng(0).uniform(0, 1000, (4, 6))
    np.testing.assert_allclose(w @ inten, np.linalg.lstsq(SPECTRA.T, inten, rcond=None)[0], rtol=1e-10, atol=1e-9)
    assert unmix.unmixing_matrix(SPECTRA.astype(np.float32).tolist()).dtype == np.float64
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((2, 0)), np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]])):
        with pytest.raises(ValueError):
            unmix.unmixing_matrix(bad)


def test_derived_names():
    assert unmix.derived_names(["eu", "dy", "sm"]) == ["eu", "dy", "sm", "dy/eu", "sm/eu"]
    assert unmix.derived_names(np.array(["eu"])) == ["eu"]
    with pytest.raises(ValueError):
        unmix.derived_names([])


def test_header_defines():
    want = {"MG_UNMIX_MAX_CHANNELS": 16, "MG_UNMIX_MAX_LN": 8, "MG_UNMIX_MAX_Q": 8, "MG_UNMIX_MAX_LEN": 1024}
    for k, v in want.items():
        assert nat.DEFINES[k] == v
    assert (unmix.MAX_CHANNELS, unmix.MAX_LN, unmix.MAX_Q, unmix.MAX_LEN) == (16, 8, 8, 1024)
    budget = nat.DEFINES["MG_UNMIX_LDS_KEY_BYTES"]
    assert budget == hotpath.UNMIX_LDS_KEY_BYTES and budget % 8 == 0
    # the workload's own bead -- a disk of radius 25 with 5 lanthanides -- fits, and two such workgroups fit 160 KiB of
    # LDS with 2 KiB each left for the kernel's own tables
    assert disk(100, 25).sum() * 5 * 8 <= budget and 2 * (budget + 2048) <= 160 * 1024


# ---- refusals of the Python layer ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix, channels, n_c", [
    (np.ones(3), None, 3), (np.ones((1, 1, 3)), None, 3), (np.ones((0, 3)), None, 3), (np.ones((9, 3)), None, 3),
    (np.ones((2, 17)), None, 17), (np.ones((2, 3)), None, 4), (np.ones((2, 3)), [0, 1], 3), (np.ones((2, 2)), [0, 3], 3),
    (np.ones((2, 2)), [-1, 0], 3), (np.ones((2, 2)), [1, 1], 3), (np.ones((2, 2)), [0.0, 1.0], 3),
    (np.ones((2, 2)), [[0, 1]], 3), (np.array([[1.0, np.nan]]), None, 2), (np.array([[1.0, np.inf]]), None, 2),
    (np.ones((2, 0)), [], 3),
])
def test_check_table_refuses(matrix, channels, n_c):
    with pytest.raises(ValueError):
        unmix.check_table(matrix, channels, n_c)


def test_check_table_and_q_accept():
    w, ch = unmix.check_table([[1, 2, 3]], None, 3)
    assert w.dtype == np.float64 and w.shape == (1, 3) and ch.dtype == np.int32 and ch.tolist() == [0, 1, 2]
    w, ch = unmix.check_table(np.ones((8, 16), dtype=np.float32), list(range(15, -1, -1)), 16)
    assert w.flags.c_contiguous and ch.tolist() == list(range(15, -1, -1))
    assert unmix.check_q(()).shape == (0,) and unmix.check_q(0.5).tolist() == [0.5]
    assert unmix.check_q([0, 1, 0.5, 0.5, 0.25, 0.75, 0.1, 0.9]).dtype == np.float64
    for bad in ([0.1] * 9, [-0.1], [1.0001], [math.nan], [math.inf]):
        with pytest.raises(ValueError):
            unmix.check_q(bad)
    assert unmix.channel_indices(["a", "b", "c"], None) == [0, 1, 2]
    assert unmix.channel_indices(["a", "b", "c"], ["c", 0, np.int64(1)]) == [2, 0, 1]
    for bad in (["d"], [True], [1.5]):
        with pytest.raises(ValueError):
            unmix.channel_indices(["a", "b", "c"], bad)


def dataset(m=3, n_c=3, n_t=2, L=8, seed=0):
    rng = np.random.default_rng(seed)
    return mg.Dataset({"roi": mg.DataArray(rng.integers(0, 999, (m, n_c, n_t, L, L)).astype(np.uint16),
                                           ("mark", "channel", "time", "roi_y", "roi_x"))},
                      coords={"fg": (("mark", "time", "roi_y", "roi_x"), rng.random((m, n_t, L, L)) > 0.5),
                              "bg": (("mark", "time", "roi_y", "roi_x"), rng.random((m, n_t, L, L)) > 0.5),
                              "channel": ("channel", ["a", "b", "c"][:n_c])})


def test_python_layer_refuses_before_any_launch():
    import torch

    ds = dataset()
    w = np.ones((2, 3))
    for kw in (dict(matrix=np.ones((2, 2))), dict(matrix=w, channels=["a", "b", "zz"]), dict(matrix=w, channels=["a", "a", "b"]),
               dict(matrix=np.ones((9, 3))), dict(matrix=w, q=[1.5]), dict(matrix=w, q=[0.5] * 9),
               dict(matrix=w, offset="fg_median"), dict(matrix=w, offset=np.zeros((3, 3, 2))), dict(matrix=w, mask=5),
               dict(matrix=np.array([[1.0, np.nan, 1.0]]))):
        with pytest.raises(ValueError):
            reduce.unmixed_stats(ds, **kw)
    roi = torch.zeros((2, 3, 1, 4, 4), dtype=torch.uint16)
    for kw in (dict(matrix=np.ones((2, 2))), dict(matrix=w, channels=[0, 1, 3]), dict(matrix=w, q=[-1.0])):
        with pytest.raises(ValueError):
            hotpath.unmix_stats(roi, None, **kw)
    with pytest.raises(ValueError):
        hotpath.unmix_stats(torch.zeros((1, 3, 1, 1025, 1025), dtype=torch.uint8), None, w)
    with pytest.raises(TypeError):
        hotpath.unmix_stats(torch.zeros((2, 3, 1, 4, 4), dtype=torch.int32), None, w)
    image = torch.zeros((3, 1, 4, 4), dtype=torch.float32)
    for kw in (dict(matrix=np.ones((2, 2))), dict(matrix=w, channels=[2, 2, 1]), dict(matrix=w, offset=[1.0, 2.0]),
               dict(matrix=w, offset=[1.0, 2.0, np.inf])):
        with pytest.raises(ValueError):
            hotpath.unmix_planes(image, **kw)
    with pytest.raises(ValueError):
        hotpath.unmix_planes(image[0], w)
    with pytest.raises(ValueError):
        unmix.planes(np.zeros((3, 4, 4)), w)
    with pytest.raises(TypeError):
        hotpath.unmix_planes(image.to(torch.int64), w)


# ---- the library --------------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_bound():
    assert len(nat.PROTOTYPES["mg_roi_unmix_stats"]) == 20 and nat.RESTYPES["mg_roi_unmix_stats"] is ctypes.c_int
    assert len(nat.PROTOTYPES["mg_unmix_planes"]) == 16 and len(nat.PROTOTYPES["mg_roi_unmix_keys_in_lds"]) == 2
    lib = nat.lib()
    assert len(lib.mg_roi_unmix_stats.argtypes) == 20 and len(lib.mg_unmix_planes.argtypes) == 16
    budget = nat.DEFINES["MG_UNMIX_LDS_KEY_BYTES"]
    for n_ln in (1, 2, 5, 8):
        cap = budget // (8 * n_ln)
        assert hotpath.unmix_keys_in_lds(n_ln, 0) and hotpath.unmix_keys_in_lds(n_ln, cap)
        assert not hotpath.unmix_keys_in_lds(n_ln, cap + 1)
    assert not hotpath.unmix_keys_in_lds(5, 128 * 128) and hotpath.unmix_keys_in_lds(5, int(disk(100, 25).sum()))
    for bad in ((0, 1), (9, 1), (1, -1)):
        with pytest.raises(ValueError):
            hotpath.unmix_keys_in_lds(*bad)


def test_stats_entry_refuses_on_the_host():
    """Judged before anything is launched: these return MG_EINVAL without a device."""
    fn = nat.lib().mg_roi_unmix_stats
    one = 16  # (never dereferenced: every call below is refused first)
    ch3, w23, q1 = np.array([0, 1, 2], dtype=np.int32), np.ones((2, 3)), np.array([0.5])

    def call(roi=one, dtype=nat.MG_U16, mask=None, sm=0, st=0, m=1, c=3, t=1, L=4, ch=ch3, n_k=3, w=w23, n_ln=2, off=None,
             q=q1, n_q=1, count=one, total=one, order=one):
        return fn(roi, dtype, mask, sm, st, m, c, t, L, None if ch is None else ch.ctypes.data, n_k,
                  None if w is None else w.ctypes.data, n_ln, off, None if q is None else q.ctypes.data, n_q, count, total,
                  order, None)

    assert call(m=0) == 0  # no markers: MG_OK, nothing launched
    assert call(m=0, q=None, n_q=0, order=None) == 0
    for kw in (dict(roi=None), dict(count=None), dict(total=None), dict(order=None), dict(q=None), dict(ch=None), dict(w=None),
               dict(dtype=99), dict(m=-1), dict(c=0), dict(t=0), dict(L=0), dict(L=1025), dict(n_k=0), dict(n_k=17),
               dict(n_ln=0), dict(n_ln=9), dict(n_q=-1), dict(n_q=9), dict(sm=-1), dict(st=-1),
               dict(ch=np.array([0, 1, 3], dtype=np.int32)), dict(ch=np.array([0, -1, 2], dtype=np.int32)),
               dict(ch=np.array([0, 1, 1], dtype=np.int32)), dict(w=np.array([[1.0, np.nan, 1.0], [1.0, 1.0, 1.0]])),
               dict(w=np.array([[1.0, 1.0, 1.0], [1.0, 1.0, -np.inf]])), dict(q=np.array([np.nan])), dict(q=np.array([1.5])),
               dict(q=np.array([-0.5])), dict(m=2 ** 20, t=2 ** 10), dict(m=2 ** 15, c=3 * 2 ** 15, ch=ch3, t=1),
               dict(m=0, dtype=99)):
        assert call(**kw) == -1, kw


def test_planes_entry_refuses_on_the_host():
    fn = nat.lib().mg_unmix_planes
    one = 16
    ch3, w23, off3 = np.array([2, 0, 1], dtype=np.int32), np.ones((2, 3)), np.zeros(3)

    def call(src=one, dtype=nat.MG_U16, cs=16, ts=0, c=3, t=1, h=2, w_=2, ch=ch3, n_k=3, w=w23, n_ln=2, off=off3, ratios=0,
             dst=one):
        return fn(src, dtype, cs, ts, c, t, h, w_, None if ch is None else ch.ctypes.data, n_k,
                  None if w is None else w.ctypes.data, n_ln, None if off is None else off.ctypes.data, ratios, dst, None)

    for kw in (dict(src=None), dict(dst=None), dict(ch=None), dict(w=None), dict(dtype=99), dict(c=0), dict(t=0), dict(h=0),
               dict(w_=0), dict(h=-1), dict(cs=-1), dict(ts=-1), dict(n_k=0), dict(n_k=17), dict(n_ln=0), dict(n_ln=9),
               dict(ratios=2), dict(ratios=-1), dict(ch=np.array([0, 1, 3], dtype=np.int32)),
               dict(ch=np.array([0, 0, 1], dtype=np.int32)), dict(w=np.array([[1.0, np.inf, 1.0], [1.0, 1.0, 1.0]])),
               dict(off=np.array([0.0, np.nan, 0.0])), dict(src=17), dict(dst=18), dict(t=2 ** 30, ratios=1)):
        assert call(**kw) == -1, kw
