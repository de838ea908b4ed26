"""Per-pixel unmixing on the GPU: mg_roi_unmix_stats and mg_unmix_planes against tests/unmix_ref.py -- counts and order
statistics bit for bit, sums within the bound of any summation order -- over every dtype, window length, channel
selection, lanthanide count, quantile list, value pattern, mask and stride form; both paths (volumes in LDS, values from
global memory); determinism; refusals that write nothing; reduce.unmixed_stats and the mrbles pipelines."""
import functools

import numpy as np
import pytest

import unmix_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = ("uint8", "uint16", "float32", "float64")
LENGTHS = (1, 2, 7, 33, 64, 100)
M, N_T = 3, 2
COMBOS = ((1, (0,)), (3, (0, 1, 2)), (3, (2,)), (9, tuple(range(9))), (9, (4, 0, 2)))  # (C, channels)
N_LN = (1, 2, 5)
QS = ((), (0.5,), (0.0, 0.25, 0.5, 0.75, 1.0))
WORST = {"sum": 0.0}  # the largest error / bound seen (printed by the last test of the sweep)


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def dev(a):
    import torch

    a = np.array(a, order="C")
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


@functools.lru_cache(maxsize=None)
def windows(dtype_name, L, n_c, seed=0):
    """roi (M, n_c, N_T, L, L), read-only.  (0, 0) full-range random values; (0, 1) a constant per channel: every ratio
    is tied; (1, 0) a ramp, floats with 20 % NaN pixels in the first channel; (1, 1) all zero: with zero offsets every
    ratio is 0 / 0; (2, 0) small integers 0 .. 3: ties and zeros; (2, 1) moderate random values, floats with one +inf."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([seed, L, n_c, dtype.itemsize, dtype.kind == "f"])
    shape = (M, n_c, N_T, L, L)
    if dtype.kind == "u":
        top = np.iinfo(dtype).max
        roi = rng.integers(0, top, shape, endpoint=True).astype(dtype)
        roi[0, :, 1] = (np.arange(n_c)[:, None, None] * 37 + top // 3) % (top + 1)
        roi[1, :, 0] = ((np.arange(L * L).reshape(L, L) * 7)[None] + np.arange(n_c)[:, None, None] * 11) % (top + 1)
        roi[2, :, 1] = rng.integers(100, 200, (n_c, L, L))
    else:
        big = 1e30 if dtype == np.float32 else 1e100
        roi = (rng.uniform(-1, 1, shape) * big ** rng.uniform(-1, 1, shape)).astype(dtype)
        roi[0, :, 1] = (0.1 + np.arange(n_c))[:, None, None]
        roi[1, :, 0] = (np.arange(L * L).reshape(L, L) * 0.37 - 5.0)[None] + np.arange(n_c)[:, None, None]
        roi[1, 0, 0][rng.random((L, L)) < 0.2] = np.nan
        roi[2, :, 1] = rng.normal(1000, 30, (n_c, L, L))
        roi[2, n_c - 1, 1, L // 2, L // 3] = np.inf
    roi[1, :, 1] = 0
    roi[2, :, 0] = rng.integers(0, 4, (n_c, L, L))
    roi.setflags(write=False)
    return roi


@functools.lru_cache(maxsize=None)
def masks(L, seed=0):
    m = np.random.default_rng([seed, L]).random((M, N_T, L, L)) < 0.7
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def special_masks(L):
    """(M, L, L), one per marker: random; empty; one pixel."""
    m = np.array(masks(L, 3)[:, 0])
    m[1] = False
    m[2] = False
    m[2, L // 2, L // 3] = True
    m.setflags(write=False)
    return m


def table(n_ln, n_k, seed=0):
    return np.random.default_rng([seed, n_ln, n_k]).normal(0, 1, (n_ln, n_k))


@functools.lru_cache(maxsize=None)
def offsets(n_c, seed=0):
    off = np.random.default_rng([seed, n_c]).normal(20, 50, (M, n_c, N_T))
    off.setflags(write=False)
    return off


def same_bits(got, want, what=""):
    """float64 arrays: NaN at the same places, the same bit patterns elsewhere (-0.0 is not +0.0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint64)[ok], want.view(np.uint64)[ok], err_msg=what)


def check(got, want, what=""):
    """got: the three device tensors; want: ref.roi_unmix_stats' answer."""
    import torch

    torch.cuda.synchronize()
    count, total, order = (t.cpu().numpy() for t in got)
    w_count, w_total, w_order, vals = want
    assert count.dtype == np.int32 and total.dtype == np.float64 and order.dtype == np.float64
    np.testing.assert_array_equal(count, w_count, err_msg=what)
    same_bits(order, w_order, what)
    for g in range(count.shape[0]):
        for t in range(count.shape[1]):
            for d in range(count.shape[2]):
                v, exact, have = vals[g][t][d], w_total[g, t, d], total[g, t, d]
                if len(v) == 0:
                    assert have == 0.0, (what, g, t, d)
                elif not np.isfinite(exact) or not np.isfinite(v).all():
                    assert (np.isnan(have) and np.isnan(exact)) or have == exact, (what, g, t, d, have, exact)
                else:
                    bound = ref.sum_bound(v)
                    assert abs(have - exact) <= bound, (what, g, t, d, have, exact, bound)
                    if bound > 0:
                        WORST["sum"] = max(WORST["sum"], abs(have - exact) / bound)


def case(dtype_name, L, which):
    i = LENGTHS.index(L) + 2 * DTYPES.index(dtype_name) + which
    n_c, channels = COMBOS[i % 5]
    n_ln, q = N_LN[(i + which) % 3], QS[(i // 2 + which) % 3]
    return n_c, list(channels), table(n_ln, len(channels), i), q


@functools.lru_cache(maxsize=None)
def oracle(dtype_name, L, which):
    n_c, channels, w, q = case(dtype_name, L, which)
    roi = windows(dtype_name, L, n_c)
    mask = (masks(L), special_masks(L)[:, None], None, masks(L, 1))[which]
    off = offsets(n_c) if which in (0, 2) else None
    return ref.roi_unmix_stats(roi, mask, channels, w, off, q)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("which", (0, 1, 2, 3))
def test_sweep(hp, dtype_name, L, which):
    """0: a mask per timepoint, offsets; 1: one mask per marker (time stride 0; random, empty, one pixel), no offsets;
    2: no mask, offsets; 3: a mask that is a view with a larger marker stride, no offsets."""
    import torch

    n_c, channels, w, q = case(dtype_name, L, which)
    d_roi = dev(windows(dtype_name, L, n_c))
    if which == 0:
        d_mask = dev(masks(L))
    elif which == 1:
        d_mask = dev(special_masks(L))
    elif which == 2:
        d_mask = None
    else:
        wide = torch.zeros((M, N_T + 1, L, L), dtype=torch.bool, device="cuda")
        wide[:, :N_T] = dev(masks(L, 1))
        d_mask = wide[:, :N_T]
    d_off = dev(offsets(n_c)) if which in (0, 2) else None
    got = hp.unmix_stats(d_roi, d_mask, w, channels, d_off, q)
    d = 2 * w.shape[0] - 1
    assert got[0].shape == (M, N_T, d) and got[1].shape == (M, N_T, d) and got[2].shape == (M, N_T, d, len(q), 2)
    want = oracle(dtype_name, L, which)
    check(got, want, f"{dtype_name} L={L} case {which} C={n_c} channels={channels} n_ln={w.shape[0]} q={q}")
    if which in (1, 3) and w.shape[0] > 1:  # all zero, zero offsets: every ratio is 0 / 0, every volume takes part
        n = int(want[0][1, 1, 0])
        assert want[0][1, 1, w.shape[0]:].tolist() == [0] * (w.shape[0] - 1)
        assert n == (0 if which == 1 else int(masks(L, 1)[1, 1].sum()))


def test_worst_sum_error_over_bound():
    print(f"\nunmix statistics, worst |sum error| / bound over the sweep: {WORST['sum']:.3e}")
    assert WORST["sum"] <= 1.0


@pytest.mark.parametrize("dtype_name", ("uint16", "float64"))
def test_zero_reference_volume_gives_infinite_ratios(hp, dtype_name):
    """v_0 exactly 0 at some pixels and not at others: x / 0 = +-inf takes part, 0 / 0 drops out."""
    L = 16
    rng = np.random.default_rng(2)
    roi = rng.integers(1, 50, (2, 2, 1, L, L)).astype(dtype_name)
    roi[:, 0, 0, ::3] = 0          # v_0 = 2 x_0 + 0 x_1 = 0 on every third row
    roi[:, 1, 0, ::3, ::4] = 0     # ... where some pixels have v_1 = 0 too
    w = np.array([[2.0, 0.0], [0.5, -1.0], [0.0, 1.0]])
    want = ref.roi_unmix_stats(roi, None, [0, 1], w, None, (0.0, 0.5, 1.0))
    assert np.isinf(want[2][0, 0, 3]).any() and 0 < want[0][0, 0, 3] < L * L and want[0][0, 0, 0] == L * L
    assert want[2][0, 0, 3, 0, 0] == -np.inf and want[2][0, 0, 4, 2, 1] == np.inf
    check(hp.unmix_stats(dev(roi), None, w, [0, 1], None, (0.0, 0.5, 1.0)), want, "zero reference volume")


def test_all_zero_window_counts(hp):
    roi = np.zeros((1, 2, 1, 9, 9), dtype=np.float32)
    w = np.array([[1.0, -1.0], [-2.0, -0.5]])
    want = ref.roi_unmix_stats(roi, None, [0, 1], w, None, (0.5,))
    assert want[0][0, 0].tolist() == [81, 81, 0]
    got = hp.unmix_stats(dev(roi), None, w, [0, 1], None, (0.5,))
    check(got, want, "all zero")
    assert not np.signbit(got[2].cpu().numpy()[0, 0, 0]).any()  # 1 * 0 + -1 * 0 = 0.0 + -0.0 = 0.0 ...
    assert np.signbit(got[2].cpu().numpy()[0, 0, 1]).all()  # ... and -2 * 0 + -0.5 * 0 = -0.0 + -0.0 = -0.0


# ---- both paths ------------------------------------------------------------------------------------------------------------

def disk(L, r):
    ii, jj = np.mgrid[0:L, 0:L]
    return (ii - L // 2) ** 2 + (jj - L // 2) ** 2 <= r * r


def test_large_window_takes_the_global_path(hp):
    L, n_ln = 128, 5
    assert L * L * n_ln * 8 == 640 * 1024 and not hp.unmix_keys_in_lds(n_ln, L * L)
    rng = np.random.default_rng(7)
    roi = rng.integers(0, 65535, (2, 3, 1, L, L)).astype(np.uint16)
    mask = np.ones((2, 1, L, L), dtype=bool)
    w, off = table(n_ln, 3, 1), rng.normal(100, 10, (2, 3, 1))
    want = ref.roi_unmix_stats(roi, mask, [2, 0, 1], w, off, (0.25, 0.5))
    check(hp.unmix_stats(dev(roi), dev(mask), w, [2, 0, 1], dev(off), (0.25, 0.5)), want, "L = 128, all set")
    check(hp.unmix_stats(dev(roi), None, w, [2, 0, 1], dev(off), (0.25, 0.5)), want, "L = 128, no mask")


def test_workload_bead_takes_the_lds_path(hp):
    L, n_ln = 100, 5
    fg = disk(L, 25)
    assert hp.unmix_keys_in_lds(n_ln, int(fg.sum())) and not hp.unmix_keys_in_lds(n_ln, L * L)
    rng = np.random.default_rng(8)
    roi = rng.integers(0, 65535, (3, 9, 1, L, L)).astype(np.uint16)
    mask = np.broadcast_to(fg, (3, 1, L, L))
    w, off = table(n_ln, 9, 2), rng.normal(100, 10, (3, 9, 1))
    want = ref.roi_unmix_stats(roi, mask, list(range(9)), w, off, (0.25, 0.5, 0.75))
    check(hp.unmix_stats(dev(roi), dev(np.array(mask)), w, None, dev(off), (0.25, 0.5, 0.75)), want, "disk of radius 25")


@pytest.mark.parametrize("n_ln", (2, 5))
def test_same_bits_on_either_side_of_the_budget(hp, n_ln):
    """The same pixels under the mask, once just inside the budget and once -- with one more masked pixel, a NaN that
    takes no part -- just outside it: the count and the order statistics are the same bits."""
    L = 128
    cap = hp.UNMIX_LDS_KEY_BYTES // (8 * n_ln)
    assert cap + 1 < L * L and hp.unmix_keys_in_lds(n_ln, cap) and not hp.unmix_keys_in_lds(n_ln, cap + 1)
    rng = np.random.default_rng(n_ln)
    roi = rng.normal(500, 200, (1, 3, 1, L, L)).astype(np.float32)
    order = rng.permutation(L * L)
    inside = np.zeros(L * L, dtype=bool)
    inside[order[:cap]] = True
    outside = inside.copy()
    outside[order[cap]] = True
    roi.reshape(3, -1)[:, order[cap]] = np.nan
    w, q = table(n_ln, 3, 3), (0.0, 0.25, 0.5, 0.75, 1.0)
    a = hp.unmix_stats(dev(roi), dev(inside.reshape(1, 1, L, L)), w, None, None, q)
    b = hp.unmix_stats(dev(roi), dev(outside.reshape(1, 1, L, L)), w, None, None, q)
    want = ref.roi_unmix_stats(roi, inside.reshape(1, 1, L, L), [0, 1, 2], w, None, q)
    check(a, want, "inside the budget")
    check(b, want, "outside the budget")
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes()


# ---- determinism ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ("uint16", "float64"))
def test_same_bits_on_every_call_and_stream(hp, dtype_name):
    import torch

    L = 100
    d_roi, d_mask, d_off = dev(windows(dtype_name, L, 9)), dev(masks(L)), dev(offsets(9))
    w, q = table(5, 3, 9), (0.25, 0.5, 0.75)
    run = lambda: [t.cpu().numpy().tobytes() for t in hp.unmix_stats(d_roi, d_mask, w, [4, 0, 2], d_off, q)]  # noqa: E731
    first = run()
    assert run() == first
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        assert run() == first
    torch.cuda.synchronize()


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_no_markers_and_refusals_write_nothing(hp):
    import torch

    from magnify_amd import _native as nat

    L, n_ln, n_q = 8, 2, 1
    d = 2 * n_ln - 1
    roi = dev(np.full((2, 3, 1, L, L), 3, dtype=np.uint16))
    mask = torch.ones((2, 1, L, L), dtype=torch.uint8, device="cuda")
    off = torch.zeros((2, 3, 1), dtype=torch.float64, device="cuda")
    count = torch.full((2, 1, d), -7, dtype=torch.int32, device="cuda")
    total = torch.full((2, 1, d), -7.0, dtype=torch.float64, device="cuda")
    order = torch.full((2, 1, d, n_q, 2), -7.0, dtype=torch.float64, device="cuda")
    ch3, w23, q1 = np.array([0, 1, 2], dtype=np.int32), np.ones((2, 3)), np.array([0.5])
    fn = nat.lib().mg_roi_unmix_stats

    def call(roi_p=roi.data_ptr(), dtype=nat.MG_U16, mask_p=mask.data_ptr(), sm=L * L, st=0, m=2, c=3, t=1, length=L, ch=ch3,
             n_k=3, w=w23, n_ln_=n_ln, off_p=off.data_ptr(), q=q1, n_q_=n_q, count_p=count.data_ptr(),
             total_p=total.data_ptr(), order_p=order.data_ptr()):
        rc = fn(roi_p, dtype, mask_p, sm, st, m, c, t, length, None if ch is None else ch.ctypes.data, n_k,
                None if w is None else w.ctypes.data, n_ln_, off_p, None if q is None else q.ctypes.data, n_q_, count_p,
                total_p, order_p, hp._stream())
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((count == -7).all()) and bool((total == -7.0).all()) and bool((order == -7.0).all())  # noqa: E731
    assert call(m=0) == 0 and untouched()
    for kw in [dict(roi_p=None), dict(count_p=None), dict(total_p=None), dict(order_p=None), dict(q=None), dict(ch=None),
               dict(w=None), dict(dtype=17), dict(m=-1), dict(c=0), dict(t=0), dict(length=0), dict(length=1025),
               dict(n_k=0), dict(n_k=17), dict(n_ln_=0), dict(n_ln_=9), dict(n_q_=-1), dict(n_q_=9), dict(sm=-1), dict(st=-1),
               dict(ch=np.array([0, 1, 3], dtype=np.int32)), dict(ch=np.array([-1, 1, 2], dtype=np.int32)),
               dict(ch=np.array([2, 1, 2], dtype=np.int32)), dict(w=np.array([[1.0, 1.0, np.nan], [1.0, 1.0, 1.0]])),
               dict(w=np.array([[1.0, 1.0, 1.0], [np.inf, 1.0, 1.0]])), dict(q=np.array([np.nan])), dict(q=np.array([1.25])),
               dict(q=np.array([-0.25])), dict(m=2 ** 20, t=2 ** 10)]:
        assert call(**kw) == -1 and untouched(), kw
    assert call() == 0 and not untouched() and count.cpu().numpy().tolist() == [[[64, 64, 64]]] * 2
    assert call(mask_p=None, off_p=None) == 0  # both optional
    empty = hp.unmix_stats(roi[:0], None, w23, None, None, (0.5,))
    assert empty[0].shape == (0, 1, d) and empty[2].shape == (0, 1, d, 1, 2)
    with pytest.raises(ValueError):
        hp.unmix_stats(roi, None, w23, None, torch.zeros((2, 3, 1), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        hp.unmix_stats(roi, None, w23, None, off[:1])


# ---- mg_unmix_planes -------------------------------------------------------------------------------------------------------

def plane_image(dtype_name, n_c, n_t, h, w, seed=0):
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([seed, h, w, dtype.itemsize])
    if dtype.kind == "u":
        img = rng.integers(0, np.iinfo(dtype).max, (n_c, n_t, h, w), endpoint=True).astype(dtype)
        img[0, 0, 0, 0] = 0
    else:
        img = rng.normal(300, 200, (n_c, n_t, h, w)).astype(dtype)
        img[0, 0, 0, 0] = np.nan
        img[n_c - 1, n_t - 1, h - 1, w - 1] = np.inf
        img[1, 0, h // 2, w // 2] = -np.inf
        if dtype == np.float64:
            img[2, n_t - 1, h // 2, 0] = 1e300  # beyond float32: the cast gives inf
    return img


def same_f32(got, want, what=""):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok], err_msg=what)


@pytest.mark.parametrize("shape", ((1, 1), (3, 5), (6, 10), (33, 130), (64, 257)))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_planes(hp, dtype_name, shape):
    h, w_ = shape
    n_c, n_t = 5, 2
    img = plane_image(dtype_name, n_c, n_t, h, w_)
    d_img = dev(img)
    with np.errstate(all="ignore"):
        for channels, n_ln, off in ((None, 3, None), ([4, 0, 2], 2, [10.0, -3.5, 0.25]), ([3], 1, [7.0]), ([1, 3], 5, None)):
            ch = list(range(n_c)) if channels is None else channels
            w = table(n_ln, len(ch), h)
            for ratios in (False, True):
                want = ref.planes(img, ch, w, off, ratios).astype(np.float32)
                got = hp.unmix_planes(d_img, w, channels, off, ratios).cpu().numpy()
                same_f32(got, want, f"{dtype_name} {shape} channels={channels} n_ln={n_ln} ratios={ratios}")
                assert got.shape == ((2 * n_ln - 1 if ratios else n_ln), n_t, h, w_)
        if dtype_name == "float64":
            assert np.isinf(ref.planes(img, [2], [[1.0]]).astype(np.float32)[0, n_t - 1, h // 2, 0])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_planes_strides_and_alignment(hp, dtype_name):
    h, w_, n_c, n_t = 6, 10, 4, 3
    img = plane_image(dtype_name, n_c, n_t, h, w_, 1)
    w, ch = table(3, 3, 5), [3, 0, 2]
    with np.errstate(all="ignore"):
        want = ref.planes(img, ch, w, None, True).astype(np.float32)
    big = np.zeros((2 * n_c, 2 * n_t, h, w_), dtype=img.dtype)
    big[::2, ::2] = img
    view = dev(big)[::2, ::2]
    assert view.stride(0) == 4 * n_t * h * w_ and view.stride(1) == 2 * h * w_ and not view.is_contiguous()
    same_f32(hp.unmix_planes(view, w, ch, None, True).cpu().numpy(), want, "channel and time strides")
    flat = dev(np.concatenate([np.zeros(1, dtype=img.dtype), img.reshape(-1)]))
    same_f32(hp.unmix_planes(flat[1:].view(n_c, n_t, h, w_), w, ch, None, True).cpu().numpy(), want, "one element off")
    one = hp.unmix_planes(dev(img)[:, :1].expand(n_c, n_t, h, w_), w, ch, None, False).cpu().numpy()
    with np.errstate(all="ignore"):
        same_f32(one, np.repeat(ref.planes(img[:, :1], ch, w).astype(np.float32), n_t, axis=1), "time stride 0")
    # the module's front: (C, H, W) and a dataset's image
    import magnify_amd as mg

    got = mg.unmix.planes(dev(img)[:, 0], w, ch, ratios=True)
    assert got.shape == (5, h, w_)
    same_f32(got.cpu().numpy(), want[:, 0], "(C, H, W)")
    arr = mg.DataArray(dev(img), ("channel", "time", "im_y", "im_x"), {"channel": ["a", "b", "c", "d"]})
    named = mg.unmix.planes(arr, w, ["d", "a", "c"], ratios=True)
    assert named.dims == ("derived", "time", "im_y", "im_x")
    same_f32(named.data.cpu().numpy(), want, "a DataArray, channels by name")


def test_planes_refusals_write_nothing(hp):
    import torch

    from magnify_amd import _native as nat

    h, w_ = 4, 6
    src = dev(np.full((3, 1, h, w_), 5, dtype=np.uint16))
    dst = torch.full((3, 1, h, w_), -7.0, dtype=torch.float32, device="cuda")
    ch3, w23, off3 = np.array([2, 0, 1], dtype=np.int32), np.ones((2, 3)), np.zeros(3)
    fn = nat.lib().mg_unmix_planes

    def call(src_p=src.data_ptr(), dtype=nat.MG_U16, cs=h * w_, ts=0, c=3, t=1, hh=h, ww=w_, ch=ch3, n_k=3, w=w23, n_ln=2,
             off=off3, ratios=1, dst_p=dst.data_ptr()):
        rc = fn(src_p, dtype, cs, ts, c, t, hh, ww, None if ch is None else ch.ctypes.data, n_k,
                None if w is None else w.ctypes.data, n_ln, None if off is None else off.ctypes.data, ratios, dst_p,
                hp._stream())
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((dst == -7.0).all())  # noqa: E731
    for kw in [dict(src_p=None), dict(dst_p=None), dict(ch=None), dict(w=None), dict(dtype=17), dict(c=0), dict(t=0),
               dict(hh=0), dict(ww=0), dict(cs=-1), dict(ts=-1), dict(n_k=0), dict(n_k=17), dict(n_ln=0), dict(n_ln=9),
               dict(ratios=2), dict(ch=np.array([0, 1, 3], dtype=np.int32)), dict(ch=np.array([1, 1, 0], dtype=np.int32)),
               dict(w=np.array([[1.0, np.nan, 1.0], [1.0, 1.0, 1.0]])), dict(off=np.array([0.0, np.inf, 0.0])),
               dict(src_p=src.data_ptr() + 1), dict(dst_p=dst.data_ptr() + 2)]:
        assert call(**kw) == -1 and untouched(), kw
    assert call() == 0 and not untouched()
    assert dst.cpu().numpy()[:2].tolist() == np.full((2, 1, h, w_), 15.0).tolist() and bool((dst[2] == 1.0).all())


# ---- reduce.unmixed_stats and the pipelines ------------------------------------------------------------------------------

def test_reduce_forms(hp):
    import magnify_amd as mg

    L, n_c = 33, 3
    roi, fg, bg = windows("uint16", L, n_c), masks(L), masks(L, 1)
    ds = mg.Dataset({"roi": mg.DataArray(np.array(roi), ("mark", "channel", "time", "roi_y", "roi_x"))},
                    coords={"fg": (("mark", "time", "roi_y", "roi_x"), np.array(fg)),
                            "bg": (("mark", "time", "roi_y", "roi_x"), np.array(bg)), "channel": ("channel", ["a", "b", "c"])})
    w = table(2, 3, 4)
    med = ref.nanmedian_windows(roi, bg)
    want = ref.roi_unmix_stats(roi, fg, [0, 1, 2], w, med, (0.5,))
    got = mg.reduce.unmixed_stats(ds, w)
    assert got[0].dims == ("mark", "time", "derived") and got[2].dims == ("mark", "time", "derived", "quantile", "bound")
    check([g.data for g in got], want, "defaults: bg median, fg, the median")
    by_name = mg.reduce.unmixed_stats(ds, w[:, :2], channels=["c", "a"], offset=None, mask="bg", q=(0.25, 0.75))
    check([g.data for g in by_name], ref.roi_unmix_stats(roi, bg, [2, 0], w[:, :2], None, (0.25, 0.75)), "names, no offset, bg")
    given = mg.reduce.unmixed_stats(ds, w, offset=mg.DataArray(med, ("mark", "channel", "time")), mask=None, q=())
    check([g.data for g in given], ref.roi_unmix_stats(roi, None, [0, 1, 2], w, med, ()), "an offset given, every pixel")
    one = mg.reduce.unmixed_stats(ds, w, time=1)
    assert one[0].shape == (M, 1, 3)
    check([g.data for g in one], ref.roi_unmix_stats(roi[:, :, 1:], fg[:, 1:], [0, 1, 2], w, med[:, :, 1:], (0.5,)), "time=1")
    q = mg.reduce.interpolate_quantiles(got[0].data, got[2].data, (0.5,)).cpu().numpy()
    same_bits(q, ref.interpolate(want[0], want[2], (0.5,)), "interpolated")


SPECTRA = np.array([[1.0, 0.2, 0.05, 0.0], [0.1, 1.0, 0.3, 0.02], [0.0, 0.25, 1.0, 0.4]])  # (eu, dy, sm) x channel
CHANS = ["c620", "c572", "c600", "c650"]
POS = [[200, 200], [200, 800], [512, 512], [800, 200], [800, 800], [512, 200]]


@pytest.fixture(scope="module")
def bead_field(tmp_path_factory):
    """A 1024 x 1024 four-channel bead field and the spectra / codes files (the lanthanides of the existing mrbles
    tests; the spectra file lists dy first, the reference lanthanide must still come out first).  The searched channel
    is clean -- flat beads on a flat background, as in the reference's tests --, the others carry noise, so that the
    pixels of a bead disagree."""
    from synth import draw_beads

    rng = np.random.default_rng(5)
    vols = rng.uniform(200, 900, size=(len(POS), 3))
    data = np.zeros((4, 1024, 1024), dtype=np.uint16)
    for c in range(4):
        inten = (vols @ SPECTRA[:, c]).round().astype(int)
        noise = rng.integers(-5, 6, (1024, 1024)) if c else 0
        data[c] = (draw_beads((1024, 1024), POS, 20, inten).astype(np.int64) + 100 + noise).astype(np.uint16)
    tmp = tmp_path_factory.mktemp("unmix")
    sp_csv, codes_csv = tmp / "spectra.csv", tmp / "codes.csv"
    rows = {"eu": SPECTRA[0], "dy": SPECTRA[1], "sm": SPECTRA[2]}
    sp_csv.write_text("name," + ",".join(CHANS) + "\n" + "".join(f"{n}," + ",".join(map(str, rows[n])) + "\n"
                                                                   for n in ("dy", "eu", "sm")))
    codes_csv.write_text("name,eu,dy,sm\ncode0,1,0.5,0.2\ncode1,1,1.0,0.4\n")
    kw = dict(spectra=str(sp_csv), codes=str(codes_csv), min_bead_diameter=16, max_bead_diameter=24, overlap=0, num_iter=20000,
              search_channel=CHANS[0])
    return data, vols, kw


def run_pipe(data, kw, restore=False, **more):
    import magnify_amd as mg

    mg.seed(99)
    pipe = mg.mrbles_pipe(**kw, **more)
    if not restore:
        pipe.remove_pipe("restore_format")
    return pipe(mg.DataArray(data=data, dims=("channel", "y", "x"), coords={"channel": CHANS}))


def test_mrbles_pixel_unmixing_end_to_end(hp, bead_field):
    import magnify_amd as mg

    data, vols, kw = bead_field
    xp = run_pipe(data, kw, unmix="pixel")
    m = xp.roi.sizes["mark"]
    assert m == len(POS) and list(xp.ln.values) == ["eu", "dy", "sm"]
    for name in ("ln_vol", "ln_ratio", "ln_ratio_spread"):
        assert xp[name].dims == ("mark", "ln") and xp[name].shape == (m, 3) and xp[name].dtype == np.float64, name
    assert xp.ln_pixels.dims == ("mark",) and xp.ln_pixels.dtype == np.int32
    assert xp.tag.dims == ("mark",) and len(xp.tag.values) == m
    assert set(xp.tag.values.tolist()) <= {"code0", "code1", "outlier"}
    roi = xp.roi.transpose("mark", "channel", "time", "roi_y", "roi_x").values
    fg = xp.fg.transpose("mark", "time", "roi_y", "roi_x").values
    bg = xp.bg.transpose("mark", "time", "roi_y", "roi_x").values
    w = mg.unmix.unmixing_matrix(SPECTRA)
    vol, ratio, spread, pixels = ref.identify_pixel(roi, fg, bg, w, [0, 1, 2, 3])
    same_bits(xp.ln_vol.values, vol, "ln_vol")
    same_bits(xp.ln_ratio.values, ratio, "ln_ratio")
    same_bits(xp.ln_ratio_spread.values, spread, "ln_ratio_spread")
    np.testing.assert_array_equal(xp.ln_pixels.values, pixels)
    np.testing.assert_array_equal(xp.ln_pixels.values, fg[:, 0].sum(axis=(1, 2)))
    assert (xp.ln_ratio.values[:, 0] == 1.0).all() and (xp.ln_ratio_spread.values[:, 0] == 0.0).all()
    assert (xp.ln_ratio_spread.values[:, 1:] > 0).all()
    # beads are found in some order: match by position, volumes recovered to a few percent
    got = {(int(round(y / 100)), int(round(x / 100))): v for y, x, v in zip(xp.y.values[:, 0], xp.x.values[:, 0], vol)}
    for p, v in zip(POS, vols):
        np.testing.assert_allclose(got[(round(p[0] / 100), round(p[1] / 100))], v, rtol=0.05)
    public = run_pipe(data, kw, restore=True, unmix="pixel")
    assert public.ln_ratio_spread.dims == ("mark", "ln") and public.ln_pixels.dims == ("mark",)
    assert public.ln_ratio.values.tobytes() == xp.ln_ratio.values.tobytes()


def test_mrbles_without_unmix_is_unchanged(hp, bead_field):
    import magnify_amd as mg

    data, _, kw = bead_field
    xp = run_pipe(data, kw)
    assert "ln_ratio_spread" not in xp.data_vars and "ln_pixels" not in xp.data_vars
    inten = mg.reduce.fg_mean_minus_bg_median(xp, time=0).data[:, :, 0].cpu().numpy()
    want = np.linalg.lstsq(SPECTRA.T, inten.T, rcond=None)[0].T
    np.testing.assert_array_equal(xp.ln_vol.values, want)
    np.testing.assert_array_equal(xp.ln_ratio.values, want / want[:, 0:1])
    assert xp.tag.dims == ("mark",)
    explicit = run_pipe(data, kw, unmix=None)
    assert explicit.ln_vol.values.tobytes() == xp.ln_vol.values.tobytes()


def test_unknown_unmix_is_refused_when_the_pipe_is_built(hp, bead_field):
    import magnify_amd as mg

    _, _, kw = bead_field
    with pytest.raises(ValueError):
        mg.mrbles_pipe(**kw, unmix="voxel")
    with pytest.raises(ValueError):
        mg.identify.identify_mrbles(None, kw["spectra"], kw["codes"], unmix="voxel")
