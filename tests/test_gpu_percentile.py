"""``hotpath.percentiles`` / ``plot.percentile_limits`` on the device against the sorted oracle
(tests/roishow_ref.percentile), bit for bit: every dtype at the percentiles 0, 1, 50, 99.8 and 100 on shapes that take
every load path of mg_percentile_histogram, on strided planes and on the roi layout, and on value patterns that put
nearly everything into one bin."""
import numpy as np
import pytest

import roishow_ref as rr
from synth import draw_beads

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
QS = (0, 1, 50, 99.8, 100)
# one value, one column, odd widths (rows start anywhere in a 16-byte vector), several workgroups
SHAPES = [(1, 1), (19, 1), (37, 53), (300, 517)]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    magnify_amd.seed(97)
    return magnify_amd


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


def uniform(rng, shape, dtype):
    """Over the full range of the type: every bit of the key is in use."""
    if np.dtype(dtype).kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    bits = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    bits = np.where(np.isnan(bits), np.float32(1.5), bits)
    return bits.astype(dtype)


def check(view, host, qs=QS):
    from magnify_amd import hotpath

    got = hotpath.percentiles(view, qs)
    want = np.array([rr.percentile(host, q) for q in qs])
    assert got.dtype == np.float64 and got.shape == (len(qs),)
    np.testing.assert_array_equal(got, want)
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_uniform_values_over_the_full_range(mg, shape, dtype):
    rng = np.random.default_rng(100 * shape[0] + shape[1])
    host = uniform(rng, shape, dtype)
    check(dev(host), host)
    if shape == (37, 53):  # every row on its own: 53 elements start anywhere in a 16-byte vector
        view = dev(np.pad(host, ((0, 0), (0, 3))))[:, :53]
        assert not view.is_contiguous()
        check(view, host)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_planes_of_a_channel_and_time_view_are_read_where_they_lie(mg, dtype):
    rng = np.random.default_rng(11)
    big = uniform(rng, (3, 5, 37, 53), dtype)
    d_big = dev(big)
    view = d_big[1, 0:5:2]  # timepoints 0, 2, 4 of channel 1: three planes that are not neighbours
    assert not view.is_contiguous() and view.data_ptr() != d_big.data_ptr()
    check(view, big[1, 0:5:2])
    both = d_big[0:3:2, 1:4]  # two strided dimensions over the planes
    check(both, big[0:3:2, 1:4])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_roi_layout(mg, dtype):
    rng = np.random.default_rng(12)
    roi = uniform(rng, (9, 2, 3, 7, 7), dtype)  # (mark, channel, time, L, L), L = 7: windows start anywhere
    d_roi = dev(roi)
    for c in range(2):
        view = d_roi[:, c]
        assert not view.is_contiguous()
        check(view, roi[:, c])


def patterns(dtype):
    """name -> (300, 517) array: the value patterns that are not white noise."""
    rng = np.random.default_rng(13)
    shape = (300, 517)
    kind = np.dtype(dtype).kind
    top = np.iinfo(dtype).max if kind == "u" else 60000
    out = {"constant": np.full(shape, 77, dtype=dtype)}
    out["two_values"] = np.where(rng.random(shape) < 0.3, 5, top).astype(dtype)
    hot = np.full(shape, 120, dtype=np.float64)  # 95 % at one value, a thin tail on both sides and inside its coarse bin
    tail = rng.random(shape) < 0.05
    hot[tail] = np.concatenate([rng.integers(0, top + 1, size=tail.sum() // 2),
                                rng.integers(96, 128, size=tail.sum() - tail.sum() // 2)])
    out["hot_bin"] = hot.astype(dtype)
    if kind == "f":
        # the 22 leading key bits are the same everywhere: only the last pass tells the values apart
        out["one_coarse_bin"] = (np.float32(1.0) + rng.integers(0, 1024, size=shape).astype(np.float32)
                                 * np.float32(2.0 ** -23)).astype(dtype)
        special = (rng.standard_normal(shape) * 1e3).astype(np.float32)
        flat = special.reshape(-1)
        pick = rng.permutation(flat.size)
        flat[pick[:40000]] = np.nan
        flat[pick[40000:40100]] = np.inf
        flat[pick[40100:40600]] = -np.inf
        flat[pick[42500:44000]] = 0.0
        flat[pick[44000:45500]] = -0.0
        flat[pick[45500:48000]] = (rng.integers(1, 2 ** 23, size=2500).astype(np.uint32)).view(np.float32)  # denormals
        flat[pick[48000:50000]] = -(rng.integers(1, 2 ** 23, size=2000).astype(np.uint32)).view(np.float32)
        out["special_values"] = special.astype(dtype)
    return out


@pytest.mark.parametrize("name", ["constant", "two_values", "hot_bin", "one_coarse_bin", "special_values"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_value_patterns(mg, dtype, name):
    pats = patterns(dtype)
    if name not in pats:
        assert np.dtype(dtype).kind == "u"  # the float patterns: nothing to run for integer pixels
        return
    host = pats[name]
    got = check(dev(host), host)
    if name == "hot_bin":
        assert got[2] == 120 and got[0] < 96 and got[4] > 128 and 96 <= got[1] < 120
    if name == "special_values":
        assert got[0] == -np.inf and got[4] == np.inf and np.isfinite(got[1:4]).all() and got[2] == 0.0
        check(dev(host), host, (0.3, 0.6, 20, 45, 50.5, 56, 99.95))  # seven ranks: more prefixes than one pass takes


def test_float64_values_that_differ_below_float32_precision(mg):
    rng = np.random.default_rng(14)
    host = 1000.0 + rng.integers(0, 2 ** 20, size=(37, 53)).astype(np.float64) * 2.0 ** -40  # all round to 1000.0f
    host[3, 4], host[30, 50] = 1000.0 + 2.0 ** -14, 1000.0 - 2.0 ** -14  # one float32 step up, one down
    assert len(np.unique(host)) > 1000 and len(np.unique(host.astype(np.float32))) == 3
    got = check(dev(host), host)
    assert got[0] == np.float32(1000.0 - 2.0 ** -14) and got[2] == 1000.0 and got[4] == np.float32(1000.0 + 2.0 ** -14)
    big = np.array([[1e300, -1e300, 3.0, 1e-300]])  # beyond float32: +-inf and 0, as the rounding gives them
    np.testing.assert_array_equal(check(dev(big), big, (0, 34, 67, 100)), [-np.inf, 0.0, 3.0, np.inf])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_a_channel_of_nan_is_refused(mg, dtype):
    import magnify_amd as m
    from magnify_amd import hotpath

    with pytest.raises(ValueError):
        hotpath.percentiles(dev(np.full((19, 7), np.nan, dtype=dtype)), (1, 99))
    image = np.ones((2, 1, 8, 8), dtype=dtype)
    image[1] = np.nan
    xp = m.Dataset({"image": m.DataArray(image, ("channel", "time", "im_y", "im_x"))})
    with pytest.raises(ValueError, match="channel 1"):
        m.plot.percentile_limits(xp)
    one = hotpath.percentiles(dev(np.array([np.nan, 4.0, np.nan], dtype=dtype)), (0, 50, 100))
    np.testing.assert_array_equal(one, [4.0, 4.0, 4.0])


def test_percentile_limits_of_a_bead_dataset(mg):
    beads = np.array([[60, 60], [60, 190], [128, 128], [190, 70], [185, 185]])
    rng = np.random.default_rng(15)
    a = draw_beads((256, 256), beads) + rng.integers(90, 130, size=(256, 256)).astype(np.uint16)
    b = draw_beads((256, 256), beads, value=3000) + rng.integers(300, 900, size=(256, 256)).astype(np.uint16)
    data = mg.DataArray(data=np.stack([a, b]), dims=("channel", "y", "x"), coords={"channel": ["red", "green"]})
    xp = mg.beads(data=data, min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=10000)
    assert xp.sizes["mark"] >= 1 and "channel" in xp.roi.dims
    image = xp.image.transpose("channel", "time", "im_y", "im_x").values
    roi = xp.roi.transpose("channel", "mark", "time", "roi_y", "roi_x").values
    for source, host in (("image", image), ("roi", roi)):
        got = mg.plot.percentile_limits(xp, source=source)
        assert got.shape == (2, 2) and got.dtype == np.float64
        np.testing.assert_array_equal(got, rr.percentile_limits(host, 1.0, 99.8))
        np.testing.assert_array_equal(mg.plot.percentile_limits(xp, 0, 100, source=source),
                                      [[host[c].min(), host[c].max()] for c in range(2)])
        assert (got[:, 0] < got[:, 1]).all()
    rgb = mg.plot.overview(xp, contrast_limits=mg.plot.percentile_limits(xp), overlay=None)  # usable as limits
    assert rgb.shape == (1, 256, 256, 3)
