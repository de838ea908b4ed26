"""``rotation="auto"`` on the device: mg_skew_profiles and ``magnify_amd.skew`` against their NumPy
restatement (tests/skew_ref.py, itself held to the tilted chips by tests/test_cpu_skew.py) bit for bit, the entry's
refusals, and the tilted chip of tests/test_gpu_rotate.py found without being told its tilt."""
import warnings

import numpy as np
import pytest

pytest.importorskip("scipy")

import rotate_ref as rr  # noqa: E402
import skew_cases as sc  # noqa: E402
import skew_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

ANGLES = [0.0, 0.37, -0.37, 10.0, -10.0, 44.9, -44.9]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    magnify_amd.seed(4321)
    return magnify_amd


def _entry(plane, angles, lo=0.0, scale=0.0, **override):
    """mg_skew_profiles itself on a device tensor (a view with any row stride): (status, sums, counts)."""
    import torch

    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    h, w = plane.shape
    nb = min(h, w) + 2
    table = torch.from_numpy(sr.angle_table(angles)).cuda()
    sums = torch.zeros((len(angles), 2, nb), dtype=torch.int64, device="cuda")
    counts = torch.zeros((len(angles), 2, nb), dtype=torch.int32, device="cuda")
    args = dict(d_plane=plane.data_ptr(), dtype=nat.dtype_code(plane.dtype), h=h, w=w, row_stride=plane.stride(0), lo=lo,
                scale=scale, d_cs=table.data_ptr(), n_angles=len(angles), d_sums=sums.data_ptr(),
                d_counts=counts.data_ptr(), stream=hotpath._stream())
    args.update(override)
    rc = nat.lib().mg_skew_profiles(*args.values())
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def _check(plane_np, plane_dev, angles, lo=0.0, scale=0.0, what=""):
    rc, sums, counts = _entry(plane_dev, angles, lo, scale)
    assert rc == 0, what
    want_sums, want_counts = sr.profiles(plane_np, angles, lo, scale)
    np.testing.assert_array_equal(counts, want_counts, err_msg=what)
    np.testing.assert_array_equal(sums, want_sums, err_msg=what)
    assert counts.any()


# 33 x 47: one tile, cut on both sides; 131 x 197: odd, three by four tiles, so flushed tiles meet in bins
@pytest.mark.parametrize("dtype,shape", [("uint8", (33, 47)), ("uint16", (131, 197)), ("uint16", (8, 8))])
def test_integer_planes_equal_the_restatement(mg, dtype, shape):
    import torch

    plane = rr.random_image(np.random.default_rng(shape[0]), dtype, shape)
    _check(plane, torch.from_numpy(plane).cuda(), ANGLES, what=f"{dtype} {shape}")


def test_a_view_with_a_row_stride(mg):
    import torch

    wide = rr.random_image(np.random.default_rng(7), "uint16", (131, 260))
    view = torch.from_numpy(wide).cuda()[:, 21:218]
    assert view.stride(0) == 260 and view.shape == (131, 197)
    _check(np.ascontiguousarray(wide[:, 21:218]), view, ANGLES, what="row stride")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_planes_are_quantised_and_nan_is_left_out(mg, dtype):
    import torch

    rng = np.random.default_rng(61)
    plane = rng.uniform(-50.0, 450.0, size=(61, 128)).astype(dtype)
    plane[rng.random(plane.shape) < 0.05] = np.nan
    plane[30, 60:70] = np.nan
    lo, scale = 10.25, 65535.0 / 391.5  # pixels below lo and above lo + 65535 / scale = 401.75 on both sides
    assert (plane < lo).any() and (plane > lo + 65535.0 / scale).any()
    _check(plane, torch.from_numpy(plane).cuda(), ANGLES, lo, scale, what=dtype)


def test_no_partial_sum_overflows_on_a_saturated_plane(mg):
    import torch

    plane = np.full((300, 300), 65535, dtype=np.uint16)
    _check(plane, torch.from_numpy(plane).cuda(), [0.0, 0.37, 44.9], what="all 65535")


def test_profiles_chunks_a_long_table_and_derives_the_float_range(mg):
    import torch

    from magnify_amd import skew

    assert skew.MAX_ANGLES == 64
    angles = np.linspace(-44.9, 44.9, 130)
    plane = rr.random_image(np.random.default_rng(130), "uint16", (131, 197))
    sums, counts = skew.profiles(torch.from_numpy(plane).cuda(), angles)
    want_sums, want_counts = sr.profiles(plane, angles)
    assert sums.dtype == np.uint64 and counts.dtype == np.uint32 and sums.shape == (130, 2, 133)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(sums, want_sums)
    fplane = np.random.default_rng(131).normal(5.0, 2.0, size=(61, 128)).astype(np.float32)
    sums, counts = skew.profiles(torch.from_numpy(fplane).cuda(), ANGLES)
    want_sums, want_counts = sr.profiles(fplane, ANGLES)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(sums, want_sums)
    np.testing.assert_array_equal(skew.score(sums, counts), sr.score(want_sums, want_counts))
    flat = torch.full((16, 16), 3.5, dtype=torch.float64, device="cuda")
    sums, counts = skew.profiles(flat, [0.0])
    assert not sums.any() and counts.any()
    fplane[3, 4] = np.nan
    with pytest.raises(ValueError):
        skew.profiles(torch.from_numpy(fplane).cuda(), ANGLES)


def test_refusals_launch_nothing(mg):
    import torch

    plane = torch.from_numpy(rr.random_image(np.random.default_rng(3), "uint16", (40, 48))).cuda()
    bad = [dict(d_plane=0), dict(d_cs=0), dict(d_sums=0), dict(d_counts=0), dict(dtype=17), dict(h=7), dict(w=7),
           dict(h=32769), dict(w=32769), dict(row_stride=47), dict(n_angles=0), dict(n_angles=65),
           dict(lo=float("nan")), dict(lo=float("inf")), dict(scale=float("nan")), dict(scale=float("-inf"))]
    many = [0.0] * 65  # (room for the 65 angles that are refused)
    for override in bad:
        rc, sums, counts = _entry(plane, many, **{"n_angles": 3, **override})
        assert rc == -1, override
        assert not sums.any() and not counts.any(), override
    rc, sums, counts = _entry(plane, many, n_angles=64)
    assert rc == 0 and counts[:64].any() and not counts[64:].any()


@pytest.mark.parametrize("name", ["10x10 at 4", "noisy 10x10 at 4", "4x5 at 2.9"])
def test_estimate_rotation_has_the_oracles_bits(mg, name):
    import torch

    plane, feature, tilt = sc.chips()[name]
    want = sr.estimate_rotation(plane, feature)
    got = mg.skew.estimate_rotation(torch.from_numpy(plane).cuda(), feature)
    print(name, "device", got, "oracle", want)
    assert got == want
    assert abs(got[0] + tilt) <= sc.tolerance(plane) and got[1] >= 2.5
    ds_like = mg.skew.estimate_rotation(plane[None, None], feature, channel=0, time=0)  # a host (channel, time, y, x) image
    assert ds_like == want


def test_tilted_chip_is_found_without_being_told_its_tilt(mg):
    """tests/test_gpu_rotate.py::test_tilted_chip_is_found_after_rotating_it_back with ``rotation="auto"`` in the place of
    -4.0: that test's assertions, and the angle found."""
    tilted = rr.rotate(sc.draw_chip((10, 10), 20), 4.0)
    xp = mg.microfluidic_chip(data=mg.DataArray(data=tilted, dims=("y", "x")), shape=(10, 10), num_iter=10000,
                              rotation="auto", min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100,
                              col_dist=100)
    print("rotation", xp.attrs["rotation"], "confidence", xp.attrs["rotation_confidence"])
    assert abs(xp.attrs["rotation"] + 4.0) <= 0.104
    assert xp.attrs["rotation_confidence"] >= 2.5
    xp = xp.unstack().transpose("mark_row", "mark_col", ...)
    assert xp.roi.sizes["mark_row"] == 10 and xp.roi.sizes["mark_col"] == 10
    radii = np.sqrt(xp.fg.sum(["roi_x", "roi_y"]).to_numpy() / np.pi)
    print("radii", radii.min(), radii.max(), "x00", xp.x[0, 0].values.item(), "y00", xp.y[0, 0].values.item(),
          "x43", xp.x[4, 3].values.item(), "y43", xp.y[4, 3].values.item())
    assert 0.9 * 10 < radii.min() and radii.max() < 1.1 * 10
    assert 0.95 * 100 < xp.x[0, 0].values.item() < 1.05 * 100
    assert 0.95 * 100 < xp.y[0, 0].values.item() < 1.05 * 100
    assert 395 < xp.x[4, 3].values.item() < 405 and 495 < xp.y[4, 3].values.item() < 505


def _noise_tiles():
    return np.random.default_rng(11).integers(0, 60000, size=(2, 2, 40, 40)).astype(np.uint16)


def test_an_image_without_a_grid_is_left_as_it_is_with_a_warning(mg):
    data = mg.DataArray(data=_noise_tiles(), dims=("row", "col", "y", "x"))
    plain = mg.image(data, overlap=5)
    assert "rotation" not in plain.attrs
    assert sr.estimate_rotation(plain["image"].values, 16)[1] < 2.0  # (what the warning is about)
    with pytest.warns(UserWarning, match="no grid"):
        auto = mg.image(data, overlap=5, rotation="auto")
    assert auto.attrs["rotation"] == 0.0 and 0.0 < auto.attrs["rotation_confidence"] < 2.0
    got, want = auto["image"].values, plain["image"].values
    assert got.dtype == want.dtype and got.shape == want.shape == (70, 70)
    np.testing.assert_array_equal(got, want)


def test_a_numeric_rotation_is_what_it_was(mg):
    data = mg.DataArray(data=_noise_tiles(), dims=("row", "col", "y", "x"))
    plain = mg.image(data, overlap=5)["image"].values
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        turned = mg.image(data, overlap=5, rotation=7.5, rotation_feature=3, rotation_max=99)  # (not read, not checked)
    assert "rotation" not in turned.attrs
    np.testing.assert_array_equal(turned["image"].values.view(np.uint8), rr.rotate(plain, 7.5).view(np.uint8))


@pytest.mark.parametrize("bad", [dict(rotation_max=0), dict(rotation_max=45), dict(rotation_max=float("nan")),
                                 dict(rotation_feature=3.9), dict(rotation_feature="wide"),
                                 dict(rotation_min_confidence=-1), dict(rotation="straight")])
def test_bad_settings_raise_when_the_pipe_is_built(mg, bad):
    from magnify_amd import preprocess

    for build in (mg.image_pipe, mg.microfluidic_chip_pipe):
        with pytest.raises(ValueError):
            build(**{"rotation": "auto", **bad})
    with pytest.raises(ValueError):
        preprocess.rotate(mg.Dataset(), **{"rotation": "auto", **{k: v for k, v in bad.items()}})
