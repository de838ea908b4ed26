"""Radial profiles on the GPU: mg_roi_radial_profile against tests/radial_ref.py -- counts and integer moments bit for
bit, float moments within the bounds of their arithmetic -- over every dtype, window length, ring count, centre, value
pattern, mask and stride form; determinism; refusals that write nothing; the public pipelines."""
import functools

import numpy as np
import pytest

import radial_ref as ref

pytestmark = pytest.mark.gpu

S = 16
DTYPES = ("uint8", "uint16", "float32", "float64")
LENGTHS = (1, 2, 7, 16, 33, 64, 100)
RINGS = (1, 2, 50, 128)
M, N_C, N_T = 3, 2, 2
U = 2.0 ** -53
WORST = {"sum": 0.0, "sumsq": 0.0}  # the largest error / bound seen (printed by the last test of the sweep)


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


def gamma(k):
    k = np.maximum(np.asarray(k, dtype=np.float64), 0.0)
    return k * U / (1.0 - k * U)


@functools.lru_cache(maxsize=None)
def windows(dtype_name, L, seed=0):
    """roi (M, N_C, N_T, L, L), read-only.  (0, 0, *) full-range random values; (0, 1, 0) a constant; (0, 1, 1) a ramp;
    (1, 0, *) random, floats with NaN pixels; (1, 1, 0) floats: one +inf, (1, 1, 1) floats: +inf and -inf; integers: the
    largest value everywhere (uint16 at L = 100: 10000 times 65535); (2, *, *) moderate random values."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([seed, L, dtype.itemsize, dtype.kind == "f"])
    shape = (M, N_C, N_T, L, L)
    if dtype.kind == "u":
        top = np.iinfo(dtype).max
        roi = rng.integers(0, top, shape, endpoint=True).astype(dtype)
        roi[0, 1, 0] = top // 3
        roi[0, 1, 1] = (np.arange(L * L).reshape(L, L) * 7) % (top + 1)
        roi[1, 1] = top
        roi[2] = rng.integers(100, 200, (N_C, N_T, L, L))
    else:
        big = 1e30 if dtype == np.float32 else 1e150
        roi = (rng.uniform(-1, 1, shape) * big ** rng.uniform(-1, 1, shape)).astype(dtype)
        roi[0, 1, 0] = 0.1
        roi[0, 1, 1] = np.arange(L * L).reshape(L, L) * 0.37 - 5.0
        roi[1, 0][rng.random((N_T, L, L)) < 0.2] = np.nan
        roi[1, 1] = rng.normal(0, 1, (N_T, L, L))
        roi[1, 1, 0, L // 2, L // 3] = np.inf
        roi[1, 1, 1, 0, 0], roi[1, 1, 1, L - 1, L - 1] = np.inf, -np.inf
        roi[2] = rng.normal(1000, 30, (N_C, N_T, L, L))
    roi.setflags(write=False)
    return roi


@functools.lru_cache(maxsize=None)
def masks(L, seed=0):
    m = np.random.default_rng([seed, L]).random((M, N_T, L, L)) < 0.7
    m.setflags(write=False)
    return m


def near_centres(L):
    """(M, N_T, 2): the window middle; exactly on a pixel; at a half pixel; at a corner; outside the window; between four
    pixels off the middle."""
    h = L // 2
    return np.array([[[(L - 1) * 8, (L - 1) * 8], [h * S, h * S]],
                     [[h * S + 8, h * S - 8], [0, (L - 1) * S]],
                     [[-5 * S - 3, L * S + 40], [h * S - 8, (L // 3) * S + 8]]], dtype=np.int32)


def far_centres():
    """At both limits of the allowed range, beyond them (clamped by the kernel), and mixed."""
    lo, hi = -1024 * S, 2048 * S
    return np.array([[[lo, lo], [hi, hi]], [[lo - 1000, hi + 1000], [2 ** 30, -2 ** 30]], [[hi, lo], [lo, 40]]], dtype=np.int32)


def uniform_edges(r, reach):
    """r rings of equal width (at least 1/16 pixel) that reach about ``reach`` sixteenths."""
    return (np.arange(r + 1) * max(reach // r, 1)).astype(np.int32)


def check(got_count, got_moments, want, integer, what=""):
    import torch

    torch.cuda.synchronize()
    count, moments = got_count.cpu().numpy(), got_moments.cpu().numpy()
    np.testing.assert_array_equal(count, want["count"], err_msg=what)
    if integer:
        assert moments.tobytes() == want["moments"].tobytes(), what  # bit for bit
        return
    refm, mag, n = want["moments"], want["mag"], want["count"].astype(np.float64)
    finite = np.isfinite(refm)
    np.testing.assert_array_equal(np.where(finite, 0.0, moments), np.where(finite, 0.0, refm), err_msg=what)  # inf, NaN
    err = np.abs(np.where(finite, moments - refm, 0.0))
    bound = np.stack([gamma(n - 1) * mag[..., 0], gamma(n + 1) * mag[..., 1]], axis=-1)
    for e, name in enumerate(("sum", "sumsq")):
        ok = finite[..., e]
        assert (err[..., e][ok] <= bound[..., e][ok]).all(), (what, name, err[..., e].max())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(ok & (bound[..., e] > 0), err[..., e] / bound[..., e], 0.0)
        WORST[name] = max(WORST[name], float(ratio.max()))


@functools.lru_cache(maxsize=None)
def oracle(dtype_name, L, which):
    """(mask or None, centres, edges, the oracle's answer) of sweep case ``which`` at (dtype, L)."""
    i = LENGTHS.index(L) + DTYPES.index(dtype_name)
    if which == 0:  # near centres, a mask per timepoint, rings over the window
        r = RINGS[i % 4]
        mask, centres, edges = masks(L), near_centres(L), uniform_edges(r, max(L * S * 3 // 4, r))
    elif which == 1:  # no mask, integer edges of one pixel (3-4-5 pixels lie on them), the other ring counts
        r = RINGS[(i + 2) % 4]
        mask, centres, edges = None, near_centres(L), (np.arange(r + 1) * S).astype(np.int32)
    else:  # centres at the limits and beyond: rings of equal width up to the largest edge
        r = RINGS[(i + 1) % 4]
        mask, centres, edges = masks(L), far_centres(), uniform_edges(r, 46340)
    return mask, centres, edges, ref.profile(windows(dtype_name, L), mask, centres, edges)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("which", (0, 1, 2))
def test_sweep(hp, dtype_name, L, which):
    mask, centres, edges, want = oracle(dtype_name, L, which)
    if which == 2 and L >= 16:
        assert want["count"].sum() > 0  # the far rings do reach the window
    count, moments = hp.radial_profile(dev(windows(dtype_name, L)), None if mask is None else dev(mask), centres, edges)
    assert count.shape == (M, N_C, N_T, len(edges) - 1) and moments.shape == count.shape + (2,)
    check(count, moments, want, np.dtype(dtype_name).kind == "u", f"{dtype_name} L={L} case {which} R={len(edges) - 1}")


def test_worst_float_error_over_bound():
    print(f"\nradial profile, worst |error| / bound over the sweep: sum {WORST['sum']:.3e}, sumsq {WORST['sumsq']:.3e}")
    assert WORST["sum"] <= 1.0 and WORST["sumsq"] <= 1.0


def test_pixels_on_an_edge_go_to_the_outer_ring(hp):
    L, h = 16, 8
    roi = np.zeros((1, 1, 1, L, L), dtype=np.uint16)
    roi[0, 0, 0, h + 3, h + 4], roi[0, 0, 0, h - 4, h], roi[0, 0, 0, h, h - 3] = 5, 4, 3
    for edges in (np.arange(9) * S, np.array([0, 16, 32, 48, 64, 80, 100, 127, 128])):  # square-root path, table path
        count, moments = hp.radial_profile(dev(roi), None, np.array([[h * S, h * S]], dtype=np.int32), edges)
        np.testing.assert_array_equal(moments.cpu().numpy()[0, 0, 0, :, 0], [0, 0, 0, 3, 4, 5, 0, 0])
        np.testing.assert_array_equal(moments.cpu().numpy()[0, 0, 0, :, 1], [0, 0, 0, 9, 16, 25, 0, 0])
        assert count.cpu().numpy()[0, 0, 0].tolist()[:3] == [1, 8, 16]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("L", (33, 100))
def test_non_uniform_edges(hp, dtype_name, L):
    edges = np.array([8, 16, 28, 64, 65, 144, 145, 200, 17 * S + 5], dtype=np.int32)  # from 0.5 pixel to inside the window
    centres = near_centres(L)
    want = ref.profile(windows(dtype_name, L), masks(L)[:, :1], centres, edges)
    inside = (want["rings"][0, 0] >= 0).sum()
    assert 0 < inside < L * L and want["rings"][0, 0, 0, 0] == -1  # the corner lies beyond the last edge: no ring
    assert want["rings"][0, 1, L // 2, L // 2] == -1 and want["rings"][0, 1, L // 2, L // 2 + 1] == 1  # inside the first
    count, moments = hp.radial_profile(dev(windows(dtype_name, L)), dev(masks(L)[:, :1]), centres, edges)
    check(count, moments, want, np.dtype(dtype_name).kind == "u", f"{dtype_name} L={L} non-uniform")
    none = hp.radial_profile(dev(windows(dtype_name, L)), None, centres, edges)[0].cpu().numpy()
    np.testing.assert_array_equal(none[0, 0, 0].sum(), inside)  # (window (0, 0, 0) has no NaN)


@pytest.mark.parametrize("dtype_name", ("uint16", "float32"))
def test_mask_and_stride_forms(hp, dtype_name):
    import torch

    L = 33
    roi, mask, centres = windows(dtype_name, L), masks(L), near_centres(L)
    edges = uniform_edges(50, L * S)
    integer = np.dtype(dtype_name).kind == "u"
    d_roi = dev(roi)
    full = ref.profile(roi, mask, centres, edges)
    check(*hp.radial_profile(d_roi, dev(mask), centres, edges), full, integer, "a mask per timepoint")
    check(*hp.radial_profile(d_roi, dev(mask).view(torch.uint8) * 7, dev(centres), edges), full, integer, "uint8 mask, bytes of 7")
    one = ref.profile(roi, mask[:, :1], centres, edges)
    check(*hp.radial_profile(d_roi, dev(mask[:, 0]), centres, edges), one, integer, "one mask per marker (M, L, L)")
    check(*hp.radial_profile(d_roi, dev(mask[:, :1]), centres, edges), one, integer, "one mask per marker (M, 1, L, L)")
    check(*hp.radial_profile(d_roi, dev(mask[:, :1]).expand(M, N_T, L, L), centres, edges), one, integer, "a broadcast view")
    nothing = hp.radial_profile(d_roi, torch.zeros((M, N_T, L, L), dtype=torch.bool, device="cuda"), centres, edges)
    assert not nothing[0].any() and not nothing[1].any()  # an all-zero mask: {0, 0}, count 0 (0.0, not NaN)
    every = ref.profile(roi, None, centres, edges)
    check(*hp.radial_profile(d_roi, None, centres, edges), every, integer, "no mask")
    check(*hp.radial_profile(d_roi, torch.ones((M, L, L), dtype=torch.bool, device="cuda"), centres, edges), every, integer,
          "a mask of ones")
    # centres: one for all timepoints as (M, 2), (M, 1, 2) and an expanded view; a strided view of a wider table
    same = ref.profile(roi, mask, centres[:, :1], edges)
    check(*hp.radial_profile(d_roi, dev(mask), centres[:, 0], edges), same, integer, "centres (M, 2)")
    check(*hp.radial_profile(d_roi, dev(mask), dev(centres[:, :1]), edges), same, integer, "centres (M, 1, 2)")
    check(*hp.radial_profile(d_roi, dev(mask), dev(centres[:, :1]).expand(M, N_T, 2), edges), same, integer, "centres expanded")
    wide = torch.zeros((M, N_T + 1, 4), dtype=torch.int32, device="cuda")
    wide[:, :N_T, :2] = dev(centres)
    check(*hp.radial_profile(d_roi, dev(mask), wide[:, :N_T, :2], edges), full, integer, "centres in a wider table")
    # a channel slice of a larger roi
    big = np.zeros((M, N_C + 2, N_T, L, L), dtype=roi.dtype)
    big[:, 1:1 + N_C] = roi
    check(*hp.radial_profile(dev(big)[:, 1:1 + N_C], dev(mask), centres, edges), full, integer, "a channel slice")
    single = ref.profile(roi[:, 1:], mask, centres, edges)
    check(*hp.radial_profile(d_roi[:, 1:], dev(mask), centres, edges), single, integer, "one channel of two")
    # a window that does not start on 16 bytes, a mask that does not start on its chunk
    flat_roi = dev(np.concatenate([np.zeros(1, dtype=roi.dtype), roi.reshape(-1)]))
    flat_mask = dev(np.concatenate([np.zeros(3, dtype=bool), mask.reshape(-1)]))
    check(*hp.radial_profile(flat_roi[1:].view(d_roi.shape), flat_mask[3:].view(mask.shape), centres, edges), full, integer,
          "unaligned")


@pytest.mark.parametrize("dtype_name", ("float32", "float64"))
def test_same_bits_on_every_call(hp, dtype_name):
    L = 100
    d_roi, d_mask, centres, edges = dev(windows(dtype_name, L)), dev(masks(L)), near_centres(L), uniform_edges(50, 50 * S)
    first = [t.cpu().numpy().tobytes() for t in hp.radial_profile(d_roi, d_mask, centres, edges)]
    for _ in range(3):
        again = [t.cpu().numpy().tobytes() for t in hp.radial_profile(d_roi, d_mask, centres, edges)]
        assert again == first


def test_no_markers_and_refusals_write_nothing(hp):
    import torch

    from magnify_amd import _native as nat

    L, r = 8, 4
    roi = dev(np.full((2, 1, 1, L, L), 3, dtype=np.uint16))
    centre = torch.full((2, 1, 2), 64, dtype=torch.int32, device="cuda")
    mask = torch.ones((2, 1, L, L), dtype=torch.uint8, device="cuda")
    count = torch.full((2, 1, 1, r), -7, dtype=torch.int32, device="cuda")
    moments = torch.full((2, 1, 1, r, 2), -7.0, dtype=torch.float64, device="cuda")
    good = np.arange(r + 1, dtype=np.int32) * S
    fn = nat.lib().mg_roi_radial_profile

    def call(roi_p=roi.data_ptr(), dtype=nat.MG_U16, mask_p=mask.data_ptr(), sm=L * L, st=0, centre_p=centre.data_ptr(), csm=2,
             cst=0, edges=good, n_r=r, m=2, c=1, t=1, length=L, count_p=count.data_ptr(), moments_p=moments.data_ptr()):
        rc = fn(roi_p, dtype, mask_p, sm, st, centre_p, csm, cst, None if edges is None else edges.ctypes.data, n_r, m, c, t,
                length, count_p, moments_p, hp._stream())
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((count == -7).all()) and bool((moments == -7.0).all())  # noqa: E731
    assert call(m=0) == 0 and untouched()
    bad_edges = [np.array([0, 16, 16, 32, 48], dtype=np.int32), np.array([0, 16, 32, 48, 46341], dtype=np.int32),
                 np.array([-1, 16, 32, 48, 64], dtype=np.int32), np.array([0, 32, 16, 48, 64], dtype=np.int32)]
    for kw in [dict(roi_p=None), dict(centre_p=None), dict(edges=None), dict(count_p=None), dict(moments_p=None),
               dict(dtype=17), dict(m=-1), dict(c=0), dict(t=0), dict(length=0), dict(length=1025), dict(n_r=0), dict(n_r=129),
               dict(m=2 ** 16, c=2 ** 8, t=2 ** 7), dict(sm=-1), dict(st=-1), dict(csm=-1), dict(cst=-1)] + \
              [dict(edges=e) for e in bad_edges]:
        assert call(**kw) == -1 and untouched(), kw
    assert call() == 0 and not untouched() and int(count.sum()) > 0
    assert hp.radial_profile(roi[:0], None, np.zeros((0, 2), dtype=np.int32), good)[0].shape == (0, 1, 1, r)
    with pytest.raises(ValueError):
        hp.radial_profile(roi, None, centre, bad_edges[0])
    with pytest.raises(ValueError):
        hp.radial_profile(roi, None, centre[:1], good)
    with pytest.raises(TypeError):
        hp.radial_profile(torch.zeros((2, 1, 1, L, L), dtype=torch.int32, device="cuda"), None, centre, good)


# ---- reduce.radial_profile and the public pipelines -------------------------------------------------------------------------

def hand_dataset(L=33, dtype_name="uint16"):
    import magnify_amd as mg

    return mg.Dataset({"roi": mg.DataArray(np.array(windows(dtype_name, L)), ("mark", "channel", "time", "roi_y", "roi_x"))},
                      coords={"fg": (("mark", "time", "roi_y", "roi_x"), np.array(masks(L))),
                              "bg": (("mark", "time", "roi_y", "roi_x"), np.array(masks(L, 1)))})


def test_reduce_forms(hp):
    import magnify_amd as mg

    L = 33
    ds = hand_dataset(L)
    by_width = mg.reduce.radial_profile(ds, width=1.5, rings=9, mask=None, centre="window")
    by_edges = mg.reduce.radial_profile(ds, edges=np.arange(10) * 1.5, mask=None, centre="window")
    for a, b in zip(by_width, by_edges):  # uniform edges given explicitly: the width form
        assert a.values.tobytes() == b.values.tobytes() and a.dims == b.dims
    assert by_width[0].dims == ("mark", "channel", "time", "ring") and by_width[1].dims[-1] == "moment"
    np.testing.assert_array_equal(by_width[0].coords["ring"].values, np.arange(9) * 1.5 + 0.75)
    centres = np.full((M, 1, 2), (L // 2) * S)
    want = ref.profile(windows("uint16", L), None, centres, np.arange(10) * 24)
    check(by_width[0].data, by_width[1].data, want, True, "centre=window")
    default = mg.reduce.radial_profile(ds, mask=None, centre="window")
    assert default[0].shape[-1] == 17  # ceil(33 / 2)
    # mask="own": fg | bg of a bead; a name; a DataArray; time=k; centres given
    own = ref.profile(windows("uint16", L), masks(L) | masks(L, 1), centres, np.arange(10) * 24)
    got = mg.reduce.radial_profile(ds, width=1.5, rings=9, centre="window")
    check(got[0].data, got[1].data, own, True, "own")
    chip = ds.assign_coords(tag=(("mark",), np.array(["a", "b", "c"])))
    got = mg.reduce.radial_profile(chip, width=1.5, rings=9, centre="window")
    check(got[0].data, got[1].data, want, True, "own on a chip: every pixel")
    fg = ref.profile(windows("uint16", L), masks(L), centres, np.arange(10) * 24)
    for mask in ("fg", ds.coords["fg"]):
        got = mg.reduce.radial_profile(ds, width=1.5, rings=9, mask=mask, centre="window")
        check(got[0].data, got[1].data, fg, True, "fg")
    got = mg.reduce.radial_profile(ds, width=1.5, rings=9, mask="fg", centre="window", time=1)
    assert got[0].shape == (M, N_C, 1, 9)
    np.testing.assert_array_equal(got[0].values, fg["count"][:, :, 1:])
    given = near_centres(L) / 16.0
    got = mg.reduce.radial_profile(ds, width=1.5, rings=9, mask="fg", centre=given)
    check(got[0].data, got[1].data, ref.profile(windows("uint16", L), masks(L), near_centres(L), np.arange(10) * 24), True,
          "centres given")
    got = mg.reduce.radial_profile(ds, width=1.5, rings=9, mask="fg", centre=mg.DataArray(given, ("mark", "time", "yx")), time=-1)
    np.testing.assert_array_equal(got[0].values, ref.profile(windows("uint16", L), masks(L), near_centres(L),
                                                             np.arange(10) * 24)["count"][:, :, -1:])
    mean = mg.reduce.profile_mean(by_width[0].data, by_width[1].data)
    assert mean.shape == (M, N_C, N_T, 9) and bool((mean[2] > 99).all()) and bool((mean[2] < 200).all())


def dataset_oracle(xp, edges_q, own):
    """The oracle applied to the dataset's own roi, x, y, fg and bg (before restore_format)."""
    from magnify_amd.find import _rounded_centres, _window_origin  # (the finder's rule for the window origin)

    roi = xp.roi.values
    L = roi.shape[-1]
    x, y = xp.x.values, xp.y.values
    rc = _rounded_centres(y, x).reshape(x.shape + (2,))
    top, left = _window_origin(rc[..., 0], L, xp.sizes["im_y"]), _window_origin(rc[..., 1], L, xp.sizes["im_x"])
    centre_q = np.rint(np.stack([y - top, x - left], axis=-1) * 16).astype(np.int64)
    mask = (xp.fg.values | xp.bg.values) if own else None
    return ref.profile(roi, mask, centre_q, edges_q), centre_q, top, left


BEAD_R = 12
BEAD_CENTRES = np.array([(22, 140), (150, 22), (277, 140), (150, 257), (100, 100), (100, 124), (220, 200)])  # 4 and 5 touch
BEAD_KW = dict(min_bead_diameter=16, max_bead_diameter=32, overlap=0, num_iter=60000)


def test_beads_end_to_end(hp):
    import magnify_amd as mg
    from synth import draw_beads

    rng = np.random.default_rng(11)
    shape = (300, 280)
    image = 100 + rng.poisson(20, shape)
    image = (image + draw_beads(shape, BEAD_CENTRES, 2 * BEAD_R, 2000).astype(np.int64)).astype(np.uint16)
    data = mg.DataArray(data=image, dims=("y", "x"))

    def run(**kw):
        mg.seed(99)
        pipe = mg.beads_pipe(**BEAD_KW, **kw)
        pipe.remove_pipe("restore_format")
        return pipe(data)

    xp, plain = run(profile=1.0), run()
    for name in ("roi", "fg", "bg", "x", "y"):  # nothing else changes
        assert xp[name].values.tobytes() == plain[name].values.tobytes(), name
    assert "profile_count" not in plain.data_vars and "ring" not in plain.coords
    L = xp.roi.shape[-1]
    edges_q = np.arange(L // 2 + 1) * S
    want, centre_q, top, left = dataset_oracle(xp, edges_q, own=True)
    assert (top == 0).any() and (left == 0).any() and (top == shape[0] - L).any() and (left == shape[1] - L).any()
    assert (centre_q != (L // 2) * S).any()
    np.testing.assert_array_equal(xp.profile_count.values, want["count"])
    assert xp.profile_sum.values.tobytes() == want["moments"][..., 0].tobytes()
    assert xp.profile_sumsq.values.tobytes() == want["moments"][..., 1].tobytes()
    assert xp.profile_count.dims == ("mark", "channel", "time", "ring") and xp.profile_count.dtype == np.int32
    np.testing.assert_array_equal(xp.coords["ring"].values, np.arange(L // 2) + 0.5)
    # the touching neighbour's pixels are absent from the counts
    found = np.stack([xp.y.values[:, 0], xp.x.values[:, 0]], axis=1)
    dist = np.linalg.norm(found[:, None] - BEAD_CENTRES[None], axis=2)
    assert (dist.min(axis=0) <= 3).all(), dist.min(axis=0)
    which = dist.argmin(axis=0)
    every = dataset_oracle(xp, edges_q, own=False)[0]["count"]
    for a in (4, 5):
        i = which[a]
        missing = every[i, 0, 0] - xp.profile_count.values[i, 0, 0]
        assert missing[:6].sum() == 0 and missing[BEAD_R - 3:3 * BEAD_R].sum() > 100, missing
    lone = which[6]
    np.testing.assert_array_equal(xp.profile_count.values[lone, 0, 0][:20], every[lone, 0, 0][:20])
    # the public call: the same numbers after restore_format, and through save / load
    mg.seed(99)
    public = mg.beads(data=data, **BEAD_KW, profile=1.0)
    assert public.profile_sum.dims == ("mark", "ring")
    assert public.profile_sum.values.tobytes() == xp.profile_sum.values[:, 0, 0].tobytes()
    mg.seed(99)
    masked = mg.beads(data=data, **BEAD_KW, profile=2.0, profile_rings=5, profile_mask="fg")
    fg_only = ref.profile(xp.roi.values, xp.fg.values, centre_q, np.arange(6) * 2 * S)
    np.testing.assert_array_equal(masked.profile_count.values, fg_only["count"][:, 0, 0])


def test_tracked_beads_end_to_end(hp):
    import magnify_amd as mg
    import track_ref as tr

    shape, n_beads, r_lo, r_hi, md, n_t = (256, 240), 12, 5, 12, 6, 3
    image, drawn, offsets = tr.scene(0, shape, n_beads, r_lo, r_hi, md, n_t, channels=2)
    data = mg.DataArray(data=image, dims=("channel", "time", "y", "x"), coords={"channel": ["c0", "c1"]})
    kw = dict(min_bead_diameter=2 * r_lo, max_bead_diameter=2 * r_hi, overlap=0, num_iter=60000, search_channel="c0",
              track="ncc", max_drift=md)
    mg.seed(99)
    pipe = mg.beads_pipe(**kw, profile=1.0, profile_rings=16)
    pipe.remove_pipe("restore_format")
    xp = pipe(data)
    assert xp.coords["fg"].data.stride(1) != 0 and (xp.x.values[:, 0] != xp.x.values[:, -1]).any()  # per-time centres
    want, centre_q, _, _ = dataset_oracle(xp, np.arange(17) * S, own=True)
    assert (centre_q[:, 0] != centre_q[:, -1]).any() or (xp.x.values[:, 0] != xp.x.values[:, -1]).any()
    np.testing.assert_array_equal(xp.profile_count.values, want["count"])
    assert xp.profile_sum.values.tobytes() == want["moments"][..., 0].tobytes()
    assert xp.profile_sumsq.values.tobytes() == want["moments"][..., 1].tobytes()
    assert xp.profile_count.shape == (xp.sizes["mark"], 2, n_t, 16)


def test_chip_end_to_end(hp, tmp_path):
    import magnify_amd as mg
    from synth import draw_chip

    kw = dict(shape=(3, 3), min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100, col_dist=100,
              num_iter=5000)
    data = mg.DataArray(data=draw_chip((3, 3), 20), dims=("y", "x"))
    mg.seed(4321)
    pipe = mg.microfluidic_chip_pipe(**kw, profile=2.0)
    pipe.remove_pipe("restore_format")
    xp = pipe(data)
    L = xp.roi.shape[-1]
    r = -(-L // 4)
    want = dataset_oracle(xp, np.arange(r + 1) * 2 * S, own=False)[0]  # a chip: every pixel
    np.testing.assert_array_equal(xp.profile_count.values, want["count"])
    assert xp.profile_sum.values.tobytes() == want["moments"][..., 0].tobytes()
    assert xp.profile_sumsq.values.tobytes() == want["moments"][..., 1].tobytes()
    mg.seed(4321)
    public = mg.microfluidic_chip(data=data, **kw, profile=2.0)
    assert public.profile_sum.dims == ("mark_row", "mark_col", "ring") and public.profile_sum.shape == (3, 3, r)
    assert public.profile_sum.values.reshape(9, r).tobytes() == xp.profile_sum.values[:, 0, 0].tobytes()
    # the button is a disk of radius 10 about the found centre: the inner rings are full of it, the outer ones empty
    mean = public.profile_sum.values / np.maximum(public.profile_count.values, 1)
    assert (mean[:, :, :2] > 900).all() and (mean[:, :, 9:12] == 0).all()
    mg.save(tmp_path / "chip.nc", public)
    back = mg.load(tmp_path / "chip.nc")
    np.testing.assert_array_equal(back.profile_count.values.reshape(9, r), public.profile_count.values.reshape(9, r))
    np.testing.assert_array_equal(back.coords["ring_outer"].values, public.coords["ring_outer"].values)
