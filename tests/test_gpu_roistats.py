"""mg_roi_masked_stats / ``hotpath.masked_stats`` / ``reduce.masked_*`` / the ``roi.where(mask).<reduction>`` idiom on
the device against the NumPy oracle (tests/roistats_ref.py): every dtype at window sizes 1 .. 64 and on both sides of
the LDS budget, every kind of mask and mask layout, the value patterns that break a variance or a selection, and every
shape of ``q``.  Counts, integer sums, min / max, order statistics and quantiles are compared for equality; float sums
and m2 against the bounds derived in roistats_ref.sum_bound / m2_bound."""
import warnings
from fractions import Fraction

import numpy as np
import pytest

import roistats_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
M, C, T = 4, 2, 3
Q7 = (0, 0.01, 0.25, 0.5, 0.75, 0.998, 1)
Q16 = tuple(np.linspace(0.0, 1.0, 16))
BUDGET = 49152  # bytes of LDS for a window's keys: 4 a pixel, 8 for float64 (MG_ROISTATS_LDS_KEY_BYTES)


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


def check(hp, roi, mask_host, q, mask_dev=None, what=""):
    """Run the kernel on roi (M, C, T, L, L) under mask_dev (default: mask_host uploaded) and hold every output to the
    oracle's records of (roi, mask_host).  Returns (count, stats, order) as NumPy arrays."""
    from magnify_amd import reduce

    recs = ref.stack(roi, mask_host, q)
    count_d, stats_d, order_d = hp.masked_stats(dev(roi), dev(mask_host) if mask_dev is None else mask_dev, q)
    count, stats, order = count_d.cpu().numpy(), stats_d.cpu().numpy(), order_d.cpu().numpy()
    m, c, t = roi.shape[:3]
    assert count.shape == (m, c, t) and count.dtype == np.int32
    assert stats.shape == (m, c, t, 4) and order.shape == (m, c, t, len(q), 2)
    np.testing.assert_array_equal(count, ref.field(recs, "n", np.int64), err_msg=f"{what}: count")
    for name, col in (("min", 2), ("max", 3)):
        want = ref.field(recs, name)
        assert np.array_equal(stats[..., col], want, equal_nan=True), f"{what}: {name}"
    assert np.array_equal(order, ref.field(recs, "order"), equal_nan=True), f"{what}: order statistics"
    if len(q):
        got_q = reduce.interpolate_quantiles(count_d, order_d, q).cpu().numpy()
        want_q = ref.field(recs, "quantile")
        assert np.array_equal(got_q, want_q, equal_nan=True), f"{what}: quantiles differ from np.nanquantile"
    worst_sum = worst_m2 = 0.0
    for g in range(m):
        for k in range(c):
            for i in range(t):
                r, (s, m2) = recs[g][k][i], stats[g, k, i, :2]
                where = f"{what}: window ({g}, {k}, {i}), n = {r['n']}"
                if r["n"] == 0:
                    assert s == 0 and m2 == 0, where
                    continue
                if r["integer"]:
                    assert s == r["sum"], f"{where}: sum {s} != {r['sum']}"
                    if r["constant"]:
                        assert m2 == 0, f"{where}: m2 of a constant window is {m2}"
                    else:
                        err, bound = abs(Fraction(float(m2)) - r["m2"]), ref.m2_bound(r)
                        worst_m2 = max(worst_m2, float(err / bound))
                        assert err <= bound, f"{where}: m2 {m2} vs {float(r['m2'])}: error / bound = {float(err / bound)}"
                    continue
                if not r["finite"]:  # +-inf under the mask: the sum in numpy's class, m2 NaN
                    want = float(r["sum"])
                    assert (np.isnan(s) and np.isnan(want)) or s == want, f"{where}: sum {s}, numpy {want}"
                    assert np.isnan(m2), f"{where}: m2 {m2} with an infinity under the mask"
                    continue
                err, bound = abs(ref.LD(s) - r["sum"]), ref.sum_bound(r)
                assert err <= bound, f"{where}: sum {s} vs {r['sum']}: error {err} > {bound}"
                if bound > 0:
                    worst_sum = max(worst_sum, float(err / bound))
                if r["constant"]:
                    assert m2 == 0, f"{where}: m2 of a constant window is {m2}"
                else:
                    err, bound = abs(ref.LD(m2) - r["m2"]), ref.m2_bound(r)
                    worst_m2 = max(worst_m2, float(err / bound))
                    assert err <= bound, f"{where}: m2 {m2} vs {r['m2']}: error / bound = {float(err / bound)}"
    print(f"{what}: worst error / bound: sum {worst_sum:.3g}, m2 {worst_m2:.3g}")
    return count, stats, order


@pytest.mark.parametrize("L", [1, 2, 7, 16, 33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_mask_kind_full_range(hp, dtype, L):
    """Full-range pixels; empty, one-pixel, two-pixel, full, disk and random masks, one per (marker, timepoint)."""
    rng = np.random.default_rng(L * 10 + np.dtype(dtype).itemsize)
    roi = ref.full_range(dtype, (M, C, T, L, L), rng)
    check(hp, roi, ref.mask_set(M, T, L, rng), Q7, what=f"{np.dtype(dtype).name} L={L}")


@pytest.mark.parametrize("dtype,L,in_lds", [(np.uint8, 110, True), (np.uint8, 111, False), (np.uint16, 110, True),
                                            (np.uint16, 111, False), (np.float32, 110, True), (np.float32, 111, False),
                                            (np.float64, 78, True), (np.float64, 79, False)])
def test_both_sides_of_the_lds_budget(hp, dtype, L, in_lds):
    """The largest window whose keys fit the LDS budget and the smallest that selects from global memory, per key
    width: the same contract on both paths."""
    key_bytes = 8 if dtype == np.float64 else 4
    assert hp.ROISTATS_LDS_KEY_BYTES == BUDGET
    assert (L * L * key_bytes <= BUDGET) == in_lds
    assert hp.masked_stats_keys_in_lds(dtype, L) == in_lds
    rng = np.random.default_rng(L)
    roi = ref.full_range(dtype, (M, C, T, L, L), rng)
    if np.dtype(dtype).kind == "f":
        roi[rng.random(roi.shape) < 0.01] = np.nan
    check(hp, roi, ref.mask_set(M, T, L, rng), Q7, what=f"{np.dtype(dtype).name} L={L}")


@pytest.mark.parametrize("dtype,L,in_lds", [(np.uint8, 16, True), (np.uint16, 110, True), (np.uint16, 111, False),
                                            (np.float32, 110, True), (np.float32, 111, False), (np.float64, 78, True),
                                            (np.float64, 79, False)])
def test_median_on_both_sides_of_the_lds_budget(hp, dtype, L, in_lds):
    """``hotpath.masked_median`` is the median mode of the statistics kernel: numpy's nanmedian exactly, with the keys
    in LDS and selecting from global memory, through the 16-byte loads (uint8, L = 16: every window aligned) and the
    one-pixel path (the other sizes: window bases off 16 bytes), for an even and an odd count on either side.  Per
    marker: a random mask (timepoint 0 trimmed to an even, timepoint 1 to an odd count), an empty one (NaN), one
    pixel, all set; a mask per timepoint, then one mask for both as a stride-0 view.  Floats: NaN pixels under the mask;
    +-0 and +-inf in one window."""
    assert hp.masked_stats_keys_in_lds(dtype, L) == in_lds
    m, c, t = 4, 1, 2
    rng = np.random.default_rng(L + np.dtype(dtype).itemsize)
    is_float = np.dtype(dtype).kind == "f"
    if is_float:
        roi = rng.normal(0, 50, size=(m, c, t, L, L)).astype(dtype)
        roi[rng.random(roi.shape) < 0.02] = np.nan
        roi[3, 0, 0, 0, :4] = [-0.0, 0.0, np.inf, -np.inf]
    else:
        roi = rng.integers(0, np.iinfo(dtype).max + 1, size=(m, c, t, L, L)).astype(dtype)
    mask = np.zeros((m, t, L, L), dtype=bool)
    mask[0] = rng.random((t, L, L)) < 0.4
    mask[2, :, L // 2, L // 3] = True
    mask[3] = True
    for i in range(t):  # the random mask: an even count of values at timepoint 0, an odd one at timepoint 1
        live = np.argwhere(mask[0, i] & ~np.isnan(roi[0, 0, i].astype(np.float64)))
        assert len(live) > 2
        if len(live) % 2 != i:
            mask[0, i][tuple(live[0])] = False

    def oracle(masks):
        want, n = np.full((m, c, t), np.nan), np.zeros((m, c, t), dtype=np.int64)
        for g, k, i in np.ndindex(m, c, t):
            values = roi[g, k, i].astype(np.float64)
            under = np.sort(values[masks[g, i] & ~np.isnan(values)])
            n[g, k, i] = under.size
            if under.size and dtype == np.float64:  # the mean of the two middle values in float64, as rp.roi_reduce has it
                want[g, k, i] = (under[(under.size - 1) // 2] + under[under.size // 2]) / 2.0
            elif under.size:
                want[g, k, i] = np.nanmedian(np.where(masks[g, i], values, np.nan))
        return want, n

    d_roi = dev(roi)
    one = np.broadcast_to(mask[:, 1:], mask.shape)
    d_one = dev(mask[:, 1:].view(np.uint8)).expand(m, t, L, L)
    assert d_one.stride(1) == 0
    for what, host, device in (("a mask per timepoint", mask, dev(mask.view(np.uint8))), ("stride-0 time view", one, d_one)):
        want, n = oracle(host)
        got = hp.masked_median(d_roi, device).cpu().numpy()
        print(f"{np.dtype(dtype).name} L={L} {what}: counts {n.reshape(-1).tolist()}")
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2, 3]]).any()
    n = oracle(mask)[1]
    assert {int(v) % 2 for v in n[n > 1]} == {0, 1} and (n == 1).any() and (n == 0).any()


def test_mask_layouts(hp):
    """(M, L, L); (M, T, L, L); a stride-0 time view; bool and uint8 (any non-zero byte is set); a marker stride larger
    than L * L, read in place."""
    import torch

    L = 7
    rng = np.random.default_rng(5)
    roi = ref.full_range(np.uint16, (M, C, T, L, L), rng)
    per_time = rng.random((M, T, L, L)) < 0.5
    one = per_time[:, 0]
    q = (0.25, 0.5)
    base = check(hp, roi, one, q, what="(M, L, L) bool")
    for name, mask_dev in (
            ("(M, L, L) uint8", dev(one.astype(np.uint8) * 200)),
            ("stride-0 time view", dev(one)[:, None].expand(M, T, L, L)),
            ("(M, 1, L, L)", dev(one[:, None])),
            ("marker stride 2 L L", dev(np.stack([one, ~one], axis=1))[:, :1])):
        if name == "marker stride 2 L L":
            assert mask_dev.stride(0) == 2 * L * L
        got = check(hp, roi, one, q, mask_dev=mask_dev, what=name)
        for a, b in zip(base, got):
            assert np.array_equal(a, b, equal_nan=True), name
    check(hp, roi, per_time, q, what="(M, T, L, L) bool")
    check(hp, roi, per_time, q, mask_dev=dev(per_time.astype(np.uint8)), what="(M, T, L, L) uint8")
    strided = torch.zeros((M, T, L, 2 * L), dtype=torch.bool, device="cuda")
    strided[..., ::2] = dev(per_time)
    check(hp, roi, per_time, q, mask_dev=strided[..., ::2], what="a mask that has to be made contiguous")
    assert hp.masked_stats(dev(roi)[:0], dev(one)[:0], q)[2].shape == (0, C, T, 2, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_value_patterns(hp, dtype):
    """A constant window; two values one ulp apart; NaN sprinkled and everything under the mask NaN; +-0.0; +-inf;
    float32 denormals."""
    L = 16
    rng = np.random.default_rng(11)
    mask = ref.mask_set(M, T, L, rng)
    mask[0, 0] = True
    shape = (M, C, T, L, L)
    a = dtype(7.25)
    patterns = {
        "constant": np.full(shape, dtype(-1234.5678), dtype=dtype),
        "one ulp apart": np.where(rng.random(shape) < 0.5, a, np.nextafter(a, dtype(8))).astype(dtype),
        "signed zeros": np.where(rng.random(shape) < 0.5, dtype(0.0), dtype(-0.0)).astype(dtype),
        "zeros around": np.choose(rng.integers(0, 4, shape), [dtype(0.0), dtype(-0.0), dtype(1.5), dtype(-1.5)]).astype(dtype),
    }
    sprinkled = ref.full_range(dtype, shape, rng)
    sprinkled[rng.random(shape) < 0.2] = np.nan
    patterns["NaN sprinkled"] = sprinkled
    hidden = ref.full_range(dtype, shape, rng)
    hidden[np.broadcast_to(mask[:, None], shape)] = np.nan
    patterns["all NaN under the mask"] = hidden
    for name, special in (("+inf", [np.inf]), ("-inf", [-np.inf]), ("both infinities", [np.inf, -np.inf])):
        v = rng.standard_normal(shape).astype(dtype)
        v[rng.random(shape) < 0.05] = rng.choice(special)
        if len(special) == 2:
            v[..., 0, 0], v[..., 0, 1] = np.inf, -np.inf
        patterns[name] = v
    if dtype == np.float32:
        tiny = rng.integers(1, 1 << 23, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31)
        patterns["denormals"] = tiny.view(np.float32)
    for name, roi in patterns.items():
        count, stats, _ = check(hp, roi, mask, Q7, what=f"{np.dtype(dtype).name} {name}")
        if name == "all NaN under the mask":
            assert (count == 0).all() and np.isnan(stats[..., 2:]).all()
        if name == "denormals":
            assert (stats[count > 0][:, 0] != 0).any()


def test_integer_value_patterns(hp):
    """uint16 all 65535 at L = 64 (the largest exact sum; m2 exactly 0); one odd pixel in a saturated window; uint8
    constant."""
    L = 64
    rng = np.random.default_rng(13)
    mask = ref.mask_set(M, T, L, rng)
    top = np.full((M, C, T, L, L), 65535, dtype=np.uint16)
    count, stats, _ = check(hp, top, mask, Q7, what="uint16 saturated")
    assert mask[1, 0].all() and stats[1, 0, 0, 0] == 65535 * L * L and count[1, 0, 0] == L * L  # (the full mask)
    odd = top.copy()
    odd[..., L // 2, L // 2] = 65534
    odd[..., 0, 0] = 0
    check(hp, odd, mask, Q7, what="uint16 saturated but two pixels")
    check(hp, np.full((M, C, T, 7, 7), 200, dtype=np.uint8), ref.mask_set(M, T, 7, rng), Q7, what="uint8 constant")


@pytest.mark.parametrize("q", [(), (0,), (1,), (0.5,), Q7, Q16], ids=["none", "0", "1", "half", "seven", "sixteen"])
def test_every_shape_of_q(hp, q):
    rng = np.random.default_rng(17)
    for dtype, L in ((np.uint16, 16), (np.float32, 7)):
        roi = ref.full_range(dtype, (M, C, T, L, L), rng)
        check(hp, roi, ref.mask_set(M, T, L, rng), q, what=f"{np.dtype(dtype).name} q={q}")


def tie_fractions(n, n_low):
    """16 fractions for a window of n survivors whose n_low smallest are equal and smaller than the next: 0 and 1, a
    repeated one, two neighbours (hi of the first is lo of the second), one whose pos is an integer, the two ranks on
    either side of the step from the lowest value to the next, and some in no order.  Held to ``ref.ranks`` here."""
    d = np.float64(n - 1)
    k = n // 2
    whole = next(j for j in range(1, n - 1) if d * np.float64(j / d) == j)
    q = [0.75, 0, (k + 0.5) / d, (k + 1.5) / d, 0.3, 0.3, 1, whole / d, (n_low - 0.5) / d, (n_low - 1.5) / d,
         0.998, 0.01, 0.5, 0.25, 0.125, 0.6]
    lo, hi = ref.ranks(n, q)
    assert len(q) == 16 and q[4] == q[5] and hi[2] == lo[3] == k + 1 and lo[2] == k
    assert d * np.float64(q[7]) == whole == lo[7]
    assert (lo[8], hi[8]) == (n_low - 1, n_low) and (lo[9], hi[9]) == (n_low - 2, n_low - 1)
    return tuple(q)


@pytest.mark.parametrize("L,in_lds", [(8, True), (79, False)])
def test_ties_at_every_rank(hp, L, in_lds):
    """The walk over the fractions where sorted[lo + 1] is sorted[lo] again and where it is the next value up: float64
    windows under a full mask, keys in LDS (L = 8) and selected from global memory (L = 79).  Marker 0: three distinct
    values (timepoint 0 with a known number of the lowest, so that two fractions straddle the step; timepoint 1 drawn);
    marker 1: constant; marker 2: all NaN but one pixel (timepoint 0) and but two (timepoint 1) -- counts of exactly 1
    and 2 under the full mask.  Every output against the oracle, the order statistics for equality."""
    assert hp.masked_stats_keys_in_lds(np.float64, L) == in_lds
    m, c, t, n = 3, 1, 2, L * L
    rng = np.random.default_rng(L)
    values = np.array([-2.5, 0.0, 7.25])
    n_low = n // 3 + 1
    roi = np.empty((m, c, t, n), dtype=np.float64)
    roi[0, 0, 0] = rng.permutation(np.concatenate([np.full(n_low, values[0]), rng.choice(values[1:], n - n_low)]))
    roi[0, 0, 1] = rng.choice(values, n)
    roi[1] = 3.75
    roi[2] = np.nan
    roi[2, 0, 0, n // 2] = 1.5
    roi[2, 0, 1, [3, n - 1]] = 2.5, -1.5
    q = tie_fractions(n, n_low)
    srt = np.sort(roi[0, 0, 0])
    lo, hi = ref.ranks(n, q)
    assert (srt[lo] == srt[hi])[hi > lo].any() and (srt[lo] < srt[hi]).any()  # both answers of a next-key-up step
    count, _, _ = check(hp, roi.reshape(m, c, t, L, L), np.ones((m, t, L, L), dtype=np.uint8), q, what=f"ties L={L}")
    np.testing.assert_array_equal(count[:, 0], [[n, n], [n, n], [1, 2]])


@pytest.mark.parametrize("L,stats_in_lds,unmix_in_lds", [(8, True, True), (90, False, True), (100, False, False)])
def test_unmix_walks_the_fractions_as_masked_stats_does(hp, L, stats_in_lds, unmix_in_lds):
    """Both quantile kernels call one walk: with the 1 x 1 matrix [[1.0]] and no offset a volume is the pixel, and
    mg_roi_unmix_stats gives the count and the bits of every order statistic that mg_roi_masked_stats gives on the same
    float64 roi, mask and q -- with the keys of both in LDS (L = 8), of unmix only (L = 90), of neither (L = 100, where
    the mask is full: no other has more masked pixels than unmix keeps)."""
    m, t = 2, 2
    rng = np.random.default_rng(L)
    roi = dev(ref.full_range(np.float64, (m, 1, t, L, L), rng))
    mask = np.ones((m, t, L, L), dtype=np.uint8) if L == 100 else (rng.random((m, t, L, L)) < 0.5).astype(np.uint8)
    n_masked = mask.reshape(m, t, -1).sum(axis=-1)
    assert hp.masked_stats_keys_in_lds(np.float64, L) == stats_in_lds
    assert all(hp.unmix_keys_in_lds(1, int(k)) == unmix_in_lds for k in n_masked.ravel())
    q = (0, 0.01, 0.25, 0.5, 0.5, 0.75, 0.998, 1)
    count, _, order = hp.masked_stats(roi, dev(mask), q)
    u_count, _, u_order = hp.unmix_stats(roi, dev(mask), np.array([[1.0]]), q=q)
    assert u_order.shape == (m, t, 1, len(q), 2) and int(count.min()) > 0
    np.testing.assert_array_equal(u_count.cpu().numpy()[:, :, 0], count.cpu().numpy()[:, 0])
    np.testing.assert_array_equal(u_order.cpu().numpy()[:, :, 0].view(np.uint64),
                                  order.cpu().numpy()[:, 0].view(np.uint64))


def test_same_bits_on_every_call(hp):
    rng = np.random.default_rng(19)
    for dtype, L in ((np.float32, 33), (np.float64, 79), (np.float64, 16)):
        roi, mask = dev(ref.full_range(dtype, (M, C, T, L, L), rng)), dev(rng.random((M, T, L, L)) < 0.5)
        first = [x.cpu().numpy().view(np.uint8) for x in hp.masked_stats(roi, mask, Q7)]
        again = [x.cpu().numpy().view(np.uint8) for x in hp.masked_stats(roi, mask, Q7)]
        for a, b in zip(first, again):
            np.testing.assert_array_equal(a, b)


def test_refusals(hp):
    rng = np.random.default_rng(23)
    roi = dev(ref.full_range(np.uint16, (M, C, T, 7, 7), rng))
    mask = dev(rng.random((M, T, 7, 7)) < 0.5)
    for q in (tuple(np.linspace(0, 1, 17)), (-0.1,), (1.1,), (float("nan"),), (0.5, 2.0)):
        with pytest.raises(ValueError):
            hp.masked_stats(roi, mask, q)
    with pytest.raises(ValueError):
        hp.masked_stats(roi, mask[:, :2], (0.5,))
    with pytest.raises(TypeError):
        hp.masked_stats(__import__("torch").zeros((M, C, T, 7, 7), dtype=__import__("torch").int32, device="cuda"), mask, (0.5,))
    with pytest.raises(ValueError):
        hp.masked_stats_keys_in_lds(np.uint16, 0)


# ---- reduce.masked_* and the idiom ---------------------------------------------------------------------------------
DIM = ["roi_x", "roi_y"]


@pytest.fixture(scope="module", params=[np.uint16, np.float32], ids=["uint16", "float32"])
def scene(request):
    """A small hand-built Dataset on the device: roi (mark, channel, time, roi_y, roi_x), fg (mark, time, roi_y, roi_x)
    with every kind of mask, bg on (mark, roi_y, roi_x); its host copies and the oracle's records."""
    import magnify_amd as mg
    from magnify_amd import hotpath

    hotpath.require_gpu()
    L = 9
    rng = np.random.default_rng(29)
    roi = ref.full_range(request.param, (M, C, T, L, L), rng) if request.param == np.uint16 else \
        (rng.standard_normal((M, C, T, L, L)) * 1000).astype(np.float32)
    if request.param == np.float32:
        roi[rng.random(roi.shape) < 0.05] = np.nan
    fg = ref.mask_set(M, T, L, rng)
    bg = rng.random((M, L, L)) < 0.3
    ds = mg.Dataset({"roi": mg.DataArray(dev(roi), ("mark", "channel", "time", "roi_y", "roi_x"))},
                    coords={"fg": (("mark", "time", "roi_y", "roi_x"), dev(fg)), "bg": (("mark", "roi_y", "roi_x"), dev(bg)),
                            "channel": np.array(["a", "b"])})
    q = (0.1, 0.9)
    return {"mg": mg, "ds": ds, "roi": roi, "fg": fg, "bg": bg, "q": q, "recs": ref.stack(roi, fg, q),
            "nan_copy": np.where(fg[:, None], roi.astype(np.float64), np.nan)}


def on_device(arr):
    import torch

    return isinstance(arr.raw, torch.Tensor) and arr.raw.is_cuda


def test_reduce_functions(scene):
    """reduce.masked_count / min / max / var / std / quantile against the oracle; the mask by name, as a DataArray and
    for one timepoint."""
    from magnify_amd import reduce

    ds, recs, nan_copy = scene["ds"], scene["recs"], scene["nan_copy"]
    n = ref.field(recs, "n", np.int64)
    np.testing.assert_array_equal(reduce.masked_count(ds, "fg").values, n)
    assert np.array_equal(reduce.masked_min(ds, "fg").values, ref.field(recs, "min"), equal_nan=True)
    assert np.array_equal(reduce.masked_max(ds, "fg").values, ref.field(recs, "max"), equal_nan=True)
    got = reduce.masked_quantile(ds, scene["q"], "fg")
    assert got.dims == ("quantile", "mark", "channel", "time") and on_device(got)
    assert np.array_equal(got.values, np.moveaxis(ref.field(recs, "quantile"), -1, 0), equal_nan=True)
    assert np.array_equal(reduce.masked_quantile(ds, 0.9, "fg").values, ref.field(recs, "quantile")[..., 1], equal_nan=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ddof in (0, 1):
            want = np.nanvar(nan_copy, axis=(-1, -2), ddof=ddof)
            var, std = reduce.masked_var(ds, "fg", ddof=ddof).values, reduce.masked_std(ds, "fg", ddof=ddof).values
            assert np.array_equal(np.isnan(var), np.isnan(want)) and np.array_equal(np.isnan(var), n - ddof <= 0)
            np.testing.assert_allclose(var, want, rtol=1e-12, equal_nan=True)  # (m2 itself is held to its bound above)
            np.testing.assert_allclose(std, np.sqrt(want), rtol=1e-12, equal_nan=True)
    count, stats, order = reduce.masked_stats(ds, ds.fg, scene["q"], time=1)
    assert count.dims == ("mark", "channel", "time") and stats.shape == (M, C, 1, 4) and order.shape == (M, C, 1, 2, 2)
    np.testing.assert_array_equal(count.values[:, :, 0], n[:, :, 1])
    assert np.array_equal(order.values[:, :, 0], ref.field(recs, "order")[:, :, 1], equal_nan=True)
    bg_recs = ref.stack(scene["roi"], scene["bg"])
    np.testing.assert_array_equal(reduce.masked_count(ds, "bg").values, ref.field(bg_recs, "n", np.int64))
    assert np.array_equal(reduce.masked_max(ds, "bg", time=-1).values[:, :, 0], ref.field(bg_recs, "max")[:, :, -1], equal_nan=True)


def test_idiom_stays_on_the_device(scene):
    """xp.roi.where(xp.fg).std / quantile / max / count / sum / mean / min / var over (roi_x, roi_y) and
    xp.where(xp.fg).roi.mean(): device tensors that match the oracle, from an operand that is never materialised; its
    ``.values`` are what ``where`` has always returned."""
    ds, recs, nan_copy, q = scene["ds"], scene["recs"], scene["nan_copy"], scene["q"]
    masked = ds.roi.where(ds.fg)
    assert masked.dtype == np.float64 and masked.shape == scene["roi"].shape and masked.dims == ds.roi.dims
    n = ref.field(recs, "n", np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = {"std": np.nanstd(nan_copy, axis=(-1, -2)), "var": np.nanvar(nan_copy, axis=(-1, -2), ddof=1),
                "mean": np.nanmean(nan_copy, axis=(-1, -2)), "sum": np.nansum(nan_copy, axis=(-1, -2))}
    std = masked.std(dim=DIM)
    quant = masked.quantile(list(q), dim=DIM)
    top, low, cnt = masked.max(dim=["roi_y", "roi_x"]), masked.min(dim=DIM), masked.count(dim=DIM)
    for out in (std, quant, top, low, cnt):
        assert on_device(out)
    assert std.dims == ("mark", "channel", "time") and quant.dims == ("quantile", "mark", "channel", "time")
    np.testing.assert_array_equal(quant.coords["quantile"].values, np.asarray(q))
    np.testing.assert_array_equal(std.coords["channel"].values, np.array(["a", "b"]))
    np.testing.assert_allclose(std.values, want["std"], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(masked.var(dim=DIM, ddof=1).values, want["var"], rtol=1e-12, equal_nan=True)
    assert np.array_equal(quant.values, np.moveaxis(ref.field(recs, "quantile"), -1, 0), equal_nan=True)
    assert np.array_equal(masked.quantile(q[0], dim=DIM).values, ref.field(recs, "quantile")[..., 0], equal_nan=True)
    assert np.array_equal(top.values, ref.field(recs, "max"), equal_nan=True)
    assert np.array_equal(low.values, ref.field(recs, "min"), equal_nan=True)
    np.testing.assert_array_equal(cnt.values, n)
    assert cnt.values.dtype == np.int64
    np.testing.assert_allclose(masked.sum(dim=DIM).values, want["sum"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(masked.mean(dim=DIM).values, want["mean"], rtol=1e-12, atol=1e-9, equal_nan=True)
    if scene["roi"].dtype == np.uint16:  # exact sums: the very bits
        np.testing.assert_array_equal(masked.sum(dim=DIM).values, want["sum"])
        np.testing.assert_array_equal(masked.mean(dim=DIM).values, want["mean"])
    # the README line: over everything, combined on the device
    everything = ds.where(ds.fg).roi
    total = everything.mean()
    assert on_device(total) and total.dims == ()
    np.testing.assert_allclose(total.values, np.nanmean(nan_copy), rtol=1e-12)
    assert everything.count().item() == n.sum() and on_device(everything.count())
    np.testing.assert_allclose(everything.sum().values, np.nansum(nan_copy), rtol=1e-12)
    assert everything.max().item() == np.nanmax(nan_copy) and everything.min().item() == np.nanmin(nan_copy)
    for arr in (masked, everything):
        assert hasattr(arr.raw, "materialize"), "a reduction made a host copy of roi.where(mask)"
    # anything else materialises: exactly the array the host path returns
    values = masked.values
    assert values.dtype == np.float64 and np.array_equal(values, nan_copy, equal_nan=True)
    assert not hasattr(masked.raw, "materialize")
    np.testing.assert_array_equal(ds.roi.where(ds.fg).median().values, np.nanmedian(nan_copy))


def test_idiom_median_is_the_median_kernel(scene):
    from magnify_amd import reduce

    ds = scene["ds"]
    got = ds.roi.where(ds.fg).median(dim=DIM)
    assert on_device(got)
    np.testing.assert_array_equal(got.values.view(np.uint64), reduce.masked_median(ds, "fg").values.view(np.uint64))
    got = ds.roi.where(ds.bg).median(dim=DIM)
    np.testing.assert_array_equal(got.values.view(np.uint64), reduce.masked_median(ds, "bg").values.view(np.uint64))


def test_idiom_with_missing_and_permuted_dims(scene):
    """``assay.isel(time=0).sel(channel=c).roi``: the missing dimensions are views; a permuted roi gives the remaining
    dims in its own order; a mask the kernel does not take (one per channel) goes the host way with the same numbers."""
    mg, ds, recs, nan_copy = scene["mg"], scene["ds"], scene["recs"], scene["nan_copy"]
    n = ref.field(recs, "n", np.int64)
    one = ds.isel(time=0).sel(channel="b")
    masked = one.roi.where(one.fg)
    assert masked.dims == ("mark", "roi_y", "roi_x") and hasattr(masked.raw, "materialize")
    cnt = masked.count(dim=DIM)
    assert on_device(cnt) and cnt.dims == ("mark",)
    np.testing.assert_array_equal(cnt.values, n[:, 1, 0])
    assert np.array_equal(masked.max(dim=DIM).values, ref.field(recs, "max")[:, 1, 0], equal_nan=True)
    assert np.array_equal(masked.values, nan_copy[:, 1, 0], equal_nan=True)
    turned = ds.roi.transpose("time", "roi_x", "mark", "roi_y", "channel").where(ds.fg)
    assert hasattr(turned.raw, "materialize")
    got = turned.max(dim=DIM)
    assert got.dims == ("time", "mark", "channel") and on_device(got)
    assert np.array_equal(got.values, ref.field(recs, "max").transpose(2, 0, 1), equal_nan=True)
    assert np.array_equal(turned.values, nan_copy.transpose(2, 4, 0, 3, 1), equal_nan=True)
    per_channel = mg.DataArray(np.broadcast_to(scene["fg"][:, None], scene["roi"].shape).copy(), ds.roi.dims)
    host = ds.roi.where(per_channel)
    assert not hasattr(host.raw, "materialize")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(host.max(dim=DIM).values, ref.field(recs, "max"), equal_nan=True)
