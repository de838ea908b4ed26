"""The circle fit on the GPU: mg_roi_refine_circles against tests/refine_ref.py -- d_info equal, d_fit byte for byte --
over every dtype, window length, ray count, reach and polarity, the stride forms, the corners of the rules; determinism;
refusals that write nothing; the public pipelines.  Accuracy against the truth is tests/test_cpu_refine.py's: here the
kernel is held to the oracle."""
import functools

import numpy as np
import pytest

import refine_cases as cases
import refine_ref as ref

pytestmark = pytest.mark.gpu

S = 16
DTYPES = ("uint8", "uint16", "float32", "float64")
LENGTHS = (8, 17, 48, 100)
RAYS = (8, 64, 128)
REACHES = (1, 3, 8)
POLARITIES = (0, 1, -1)
M, N_T = 4, 2
SEEN = set()  # the statuses the sweep met (looked at by the test after it)


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
def painted(L, seed=0):
    """(pictures uint16 (M, N_T, L, L), start circles int32 (M, N_T, 3) in 1/16 pixel): the kinds in rotation, the
    truth at L / 2 +- 1 with a radius of L / 5 .. L / 3, the start the truth moved by up to a pixel in sixteenths."""
    rng = np.random.default_rng([seed, L])
    img = np.empty((M, N_T, L, L), dtype=np.uint16)
    start = np.empty((M, N_T, 3), dtype=np.int32)
    for g in range(M):
        for t in range(N_T):
            cy, cx = L / 2 + rng.uniform(-1, 1, 2)
            r = rng.uniform(L / 5, L / 3)
            img[g, t] = cases.paint(cases.KINDS[(g + t) % 3], L, cy, cx, r, rng)
            start[g, t] = np.rint(np.array([cy, cx, r]) * S) + rng.integers(-S, S + 1, 3)
    img.setflags(write=False)
    start.setflags(write=False)
    return img, start


@functools.lru_cache(maxsize=None)
def planes(dtype_name, L):
    """The pictures of ``painted`` as ``dtype_name`` (M, N_T, L, L), read-only: uint8 a sixteenth of the grey values,
    floats with a fraction added so that no value is a whole number."""
    img = painted(L)[0]
    if dtype_name == "uint16":
        out = img
    elif dtype_name == "uint8":
        out = np.clip(img // 16, 0, 255).astype(np.uint8)
    else:
        frac = np.random.default_rng([7, L]).random(img.shape)
        out = (img.astype(np.float64) + frac).astype(dtype_name)
    out = np.array(out)
    out.setflags(write=False)
    return out


def same(got, want, what=""):
    """(info, fit) from the device against the oracle's: info equal, fit byte for byte (the NaN is the agreed one)."""
    info, fit = got[0].cpu().numpy(), got[1].cpu().numpy()
    np.testing.assert_array_equal(info, want[0], err_msg=str(what))
    assert fit.dtype == np.float64 and fit.tobytes() == want[1].tobytes(), (what, fit, want[1])
    assert np.isnan(fit[info[..., 0] != 0]).all() and np.isfinite(fit[info[..., 0] == 0]).all()


# ---- the sweep -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_sweep(hp, dtype_name, L):
    win, start = planes(dtype_name, L), painted(L)[1]
    d_win, d_start = dev(win), dev(start)
    for k in RAYS:
        cs = ref.direction_table(k)
        for reach in REACHES:
            for pol in POLARITIES:
                want = ref.refine_block(win, start, cs, reach, pol, 1.0, 0.25, None)
                got = hp.refine_circles(d_win, d_start, k, reach, pol, 1.0, 0.25, None)
                same(got, want, (dtype_name, L, k, reach, pol))
                SEEN.update(want[0][..., 0].reshape(-1).tolist())
                if pol == 0 and L >= 48 and k >= 64 and reach == 3:  # the fit itself is exercised, not only refused
                    assert (want[0][..., 0] == 0).all(), want[0]


def test_sweep_met_every_ordinary_status():
    assert {ref.OK, ref.TOO_FEW} <= SEEN, SEEN


# ---- strides -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ("uint16", "float32"))
def test_stride_forms(hp, dtype_name):
    import torch

    L = 48
    win, start = planes(dtype_name, L), painted(L)[1]
    cs = ref.direction_table(64)
    want = ref.refine_block(win, start, cs)
    # a channel view of a (M, C, T, L, L) block, read in place
    block = np.zeros((M, 3, N_T, L, L), dtype=win.dtype)
    block[:, 1] = win
    block[:, 0], block[:, 2] = win[::-1], 0
    d_block = dev(block)
    view = d_block[:, 1]
    assert not view.is_contiguous()
    same(hp.refine_circles(view, dev(start)), want, "channel view")
    same(hp.refine_circles(dev(win), dev(start)), want, "contiguous planes")
    # circles with a time stride of 0: (M, 3), (M, 1, 3) and a view expanded along time
    one = np.ascontiguousarray(start[:, 0])
    want_one = ref.refine_block(win, one, cs)
    assert (want_one[0][:, 1] != want[0][:, 1]).any() or want_one[1][:, 1].tobytes() != want[1][:, 1].tobytes()
    same(hp.refine_circles(dev(win), dev(one)), want_one, "(M, 3)")
    same(hp.refine_circles(dev(win), one), want_one, "(M, 3) from the host")
    same(hp.refine_circles(dev(win), dev(one)[:, None]), want_one, "(M, 1, 3)")
    same(hp.refine_circles(dev(win), dev(one)[:, None].expand(M, N_T, 3)), want_one, "expanded")
    # circles in a wider table: a marker stride of 5
    wide = torch.zeros((M, N_T, 5), dtype=torch.int32, device="cuda")
    wide[..., :3] = dev(start)
    same(hp.refine_circles(dev(win), wide[..., :3]), want, "circle view")
    # one marker, one timepoint
    same(hp.refine_circles(dev(win)[1:2, 1:], dev(start)[1:2, 1:]), (want[0][1:2, 1:], want[1][1:2, 1:]), "1 x 1")


# ---- corners -----------------------------------------------------------------------------------------------------------------------

def corner_windows():
    """name -> (window float64 (L, L), start {cy, cx, r} in pixels, settings)."""
    rng = np.random.default_rng(3)
    L = 32
    disk = cases.paint("bright", L, 16.3, 15.6, 8.4, rng).astype(np.float64)
    small = cases.paint("bright", L, 16.2, 15.9, 2.2, rng, noise=0).astype(np.float64)
    clean = cases.paint("dark", L, 16.0, 16.0, 8.0, rng, noise=0).astype(np.float64)
    holes = disk.copy()
    holes[16, 24], holes[8, 16], holes[22, 10] = np.nan, np.inf, -np.inf  # on the edge: some rays are not usable
    d = dict(rays=64, reach=3, polarity=0, reject=1.0, min_strength=0.25, min_rays=32)
    return {
        "j_lo > 0": (small, (16, 16, 2), d),
        "r = 0": (small, (16, 16, 0), d),
        "near a corner": (disk, (2, 3, 5), d),
        "centre outside": (disk, (-5, 40, 6), d),
        "centre far outside": (disk, (5000, -5000, 3000), d),
        "flat": (np.full((L, L), 3.5), (16, 16, 8), d),
        "ramp": (np.add.outer(np.arange(L), np.arange(L)).astype(np.float64), (16, 16, 8), d),
        "nan and inf": (holes, (16, 16, 8), d),
        "all nan": (np.full((L, L), np.nan), (16, 16, 8), d),
        "2 px off": (disk, (18, 16, 8), d),
        "6 px off": (disk, (16, 22, 8), d),
        "radius 4 px off": (disk, (16, 16, 12.5), d),
        "K = min_rays": (clean, (16, 16, 8), dict(d, rays=8, min_rays=8)),
        "K = min_rays, one ray lost": (holes, (16, 16, 8), dict(d, rays=8, min_rays=8)),
        "min_rays = 3": (disk, (2, 3, 5), dict(d, min_rays=3)),
        "strength gate off": (disk, (16, 16, 8), dict(d, min_strength=0.0)),
        "strength gate full": (disk, (16, 16, 8), dict(d, min_strength=1.0, min_rays=3)),
        "tight reject": (disk, (16, 16, 8), dict(d, reject=0.15)),
        "too tight a reject": (disk, (16, 16, 8), dict(d, reject=0.05)),  # fewer than min_rays would remain: no round
        "derivative overflows": (np.where(cases.blur(cases.shape("bright", L, 16.3, 15.6, 8.4)) > 0.5, 1.5e308, -1.5e308),
                                 (16, 16, 8), d),
        "huge values": (disk * 1e300, (16, 16, 8), d),
        "forced wrong polarity": (disk, (16, 16, 8), dict(d, polarity=1)),
    }


EXPECTED_STATUS = {"j_lo > 0": 0, "flat": 1, "all nan": 1, "centre outside": 1, "centre far outside": 1, "2 px off": 0,
                   "nan and inf": 0, "K = min_rays": 0, "K = min_rays, one ray lost": 1, "strength gate off": 0,
                   "derivative overflows": 2, "min_rays = 3": 3, "tight reject": 0, "too tight a reject": 0}


@pytest.mark.parametrize("name", sorted(corner_windows()))
def test_corners(hp, name):
    win, start, kw = corner_windows()[name]
    # two timepoints: the window and its transpose, with the circle's cy and cx swapped
    block = np.stack([win, win.T])[None]
    start_q = np.rint(np.array([[start, (start[1], start[0], start[2])]]) * S).astype(np.int64)
    start_q = np.clip(start_q, -2**31, 2**31 - 1).astype(np.int32)
    cs = ref.direction_table(kw["rays"])
    args = (kw["reach"], kw["polarity"], kw["reject"], kw["min_strength"], kw["min_rays"])
    want = ref.refine_block(block, start_q, cs, *args)
    got = hp.refine_circles(dev(block), dev(start_q), kw["rays"], *args)
    same(got, want, name)
    if name in EXPECTED_STATUS:
        assert (want[0][..., 0] == EXPECTED_STATUS[name]).all(), (name, want[0])
    if name == "6 px off":
        assert set(want[0][..., 0].reshape(-1).tolist()) <= {ref.TOO_FEW, ref.OUT_OF_REACH}, want[0]
    if name == "j_lo > 0":  # rho_0 = 2 - 3 < 0: the first two samples of every ray do not exist
        assert ref.refine_window(win, start_q[0, 0], cs, *args)["info"][1] >= 32
    if name == "nan and inf":
        assert (want[0][..., 2] < 64).all() and (want[0][..., 2] >= 50).all(), want[0]
    if name in ("tight reject", "too tight a reject"):
        loose = ref.refine_block(block, start_q, cs, 3, 0, 1.0, 0.25, 32)
        if name == "tight reject":  # the rejection round dropped rays and the rest was fitted again
            assert (want[0][..., 1] < loose[0][..., 1]).all() and want[1].tobytes() != loose[1].tobytes()
        else:
            assert (want[0][..., 1] == loose[0][..., 1]).all() and want[1].tobytes() == loose[1].tobytes()


# ---- determinism -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ("uint16", "float64"))
def test_same_bits_on_every_call(hp, dtype_name):
    L = 48
    d_win, d_start = dev(planes(dtype_name, L)), dev(painted(L)[1])
    first = hp.refine_circles(d_win, d_start, 128, 8)
    again = hp.refine_circles(d_win, d_start, 128, 8)
    assert first[0].cpu().numpy().tobytes() == again[0].cpu().numpy().tobytes()
    assert first[1].cpu().numpy().tobytes() == again[1].cpu().numpy().tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_no_markers_and_refusals_write_nothing(hp):
    import torch

    from magnify_amd import _native as nat

    L = 48
    win, start = dev(planes("uint16", L)), dev(painted(L)[1])
    cs = dev(ref.direction_table(64))
    info = torch.full((M, N_T, 4), -7, dtype=torch.int32, device="cuda")
    fit = torch.full((M, N_T, 5), -7.0, dtype=torch.float64, device="cuda")
    fn = nat.lib().mg_roi_refine_circles

    def call(roi_p=win.data_ptr(), dtype=nat.MG_U16, sm=N_T * L * L, st=L * L, circle_p=start.data_ptr(), csm=N_T * 3, cst=3,
             cs_p=cs.data_ptr(), k=64, m=M, t=N_T, length=L, reach=3, pol=0, reject=1.0, strength=0.25, min_rays=32,
             info_p=info.data_ptr(), fit_p=fit.data_ptr()):
        rc = fn(roi_p, dtype, sm, st, circle_p, csm, cst, cs_p, k, m, t, length, reach, pol, reject, strength, min_rays,
                info_p, fit_p, hp._stream())
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((info == -7).all()) and bool((fit == -7.0).all())  # noqa: E731
    assert call(m=0) == 0 and untouched()
    for kw in [dict(roi_p=None), dict(circle_p=None), dict(cs_p=None), dict(info_p=None), dict(fit_p=None), dict(dtype=17),
               dict(m=-1), dict(t=0), dict(length=0), dict(length=1025), dict(m=2 ** 16, t=2 ** 15),
               dict(sm=-1), dict(st=-1), dict(csm=-1), dict(cst=-1), dict(k=7), dict(k=129), dict(reach=0), dict(reach=9),
               dict(pol=2), dict(pol=-2), dict(reject=0.0), dict(reject=-1.0), dict(reject=float("nan")),
               dict(reject=float("inf")), dict(strength=-0.5), dict(strength=1.5), dict(strength=float("nan")),
               dict(min_rays=2), dict(min_rays=65), dict(k=8, min_rays=9)]:
        assert call(**kw) == -1 and untouched(), kw
    assert call() == 0 and not untouched()
    same((info, fit), ref.refine_block(planes("uint16", L), painted(L)[1], ref.direction_table(64)), "the raw call")
    got = hp.refine_circles(win[:0], np.zeros((0, 3), dtype=np.int32))
    assert got[0].shape == (0, N_T, 4) and got[1].shape == (0, N_T, 5)
    for bad in (dict(rays=4), dict(reach=0), dict(polarity=3), dict(reject=0.0), dict(min_strength=2.0), dict(min_rays=100)):
        with pytest.raises(ValueError):
            hp.refine_circles(win, start, **bad)
    with pytest.raises(ValueError):
        hp.refine_circles(win, start[:1])
    with pytest.raises(ValueError):
        hp.refine_circles(win, start[..., :2])
    with pytest.raises(ValueError):
        hp.refine_circles(win[0], start)
    with pytest.raises(TypeError):
        hp.refine_circles(win, start.to(torch.int64))
    with pytest.raises(TypeError):
        hp.refine_circles(torch.zeros((M, N_T, L, L), dtype=torch.int32, device="cuda"), start)


# ---- reduce.refine_circles and the public pipelines ----------------------------------------------------------------------------------

def dataset_oracle(xp, radius, channel=0, rays=64, reach=3, polarity=0):
    """The oracle applied to the dataset's own roi[:, channel], x, y and the finder's radii (before restore_format):
    (info, fit, start circles in 1/16 pixel, top, left)."""
    from magnify_amd.find import _rounded_centres, _window_origin  # (the finder's rule for the window origin)

    roi = xp.roi.values
    L = roi.shape[-1]
    x, y = xp.x.values, xp.y.values
    rc = _rounded_centres(y, x).reshape(x.shape + (2,))
    top, left = _window_origin(rc[..., 0], L, xp.sizes["im_y"]), _window_origin(rc[..., 1], L, xp.sizes["im_x"])
    radius = np.asarray(radius, dtype=np.float64).reshape(x.shape[0], -1)
    circle_q = np.rint(np.stack([y - top, x - left, np.broadcast_to(radius, x.shape)], axis=-1) * 16).astype(np.int32)
    info, fit = ref.refine_block(roi[:, channel], circle_q, ref.direction_table(rays), reach, polarity)
    return info, fit, circle_q, top, left


def check_dataset(xp, radius, **kw):
    info, fit, circle_q, top, left = dataset_oracle(xp, radius, **kw)
    np.testing.assert_array_equal(xp.coords["fit_status"].values, info[..., 0])
    np.testing.assert_array_equal(xp.coords["fit_rays"].values, info[..., 1])
    np.testing.assert_array_equal(xp.coords["fit_polarity"].values, info[..., 3])
    np.testing.assert_array_equal(xp.coords["radius"].values, np.broadcast_to(np.reshape(radius, (info.shape[0], -1)),
                                                                               info.shape[:2]))
    for name in ("fit_status", "fit_rays", "fit_polarity", "radius"):
        assert xp.coords[name].dtype == np.int32 and xp.coords[name].dims == ("mark", "time")
    # bit for bit before the host's square roots, and with them
    want = {"y_fit": (top + circle_q[..., 0] / 16.0) + fit[..., 0], "x_fit": (left + circle_q[..., 1] / 16.0) + fit[..., 1],
            "radius_fit": np.sqrt(fit[..., 2]), "fit_rms": np.sqrt(fit[..., 3]), "fit_strength": fit[..., 4]}
    for name, v in want.items():
        got = xp.coords[name].values
        assert got.dtype == np.float64 and xp.coords[name].dims == ("mark", "time")
        assert got.tobytes() == np.ascontiguousarray(v).tobytes(), (name, got, v)
    return info, fit


BEAD_R = 12
BEAD_CENTRES = np.array([(22, 140), (150, 22), (277, 140), (150, 257), (100, 100), (100, 130), (220, 200)])
BEAD_KW = dict(min_bead_diameter=16, max_bead_diameter=32, overlap=0, num_iter=60000)


def test_beads_end_to_end(hp, tmp_path):
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

    xp, plain = run(refine="edge"), run()
    for name in ("roi", "fg", "bg", "x", "y", "valid"):  # nothing else changes
        assert xp[name].values.tobytes() == plain[name].values.tobytes(), name
    assert not any(k in plain.coords for k in ("x_fit", "radius_fit", "fit_status", "radius"))
    info, fit = check_dataset(xp, plain._cache["radius"])
    assert (info[..., 0] == 0).any()
    # reduce.refine_circles by name: the same; with other settings and with explicit circles: the oracle again
    again = mg.reduce.refine_circles(plain)
    for name, v in again.items():
        assert v.values.tobytes() == xp.coords[name].values.tobytes(), name
    other = plain.assign_coords(mg.reduce.refine_circles(plain, rays=32, reach=5, polarity="darker"))
    check_dataset(other, plain._cache["radius"], rays=32, reach=5, polarity=-1)
    L = xp.roi.shape[-1]
    given = np.tile([L / 2 + 0.25, L / 2 - 0.5, BEAD_R + 0.3], (xp.sizes["mark"], 1))
    got = mg.reduce.refine_circles(plain, circle=given)
    want = ref.refine_block(xp.roi.values[:, 0], np.rint(given * 16).astype(np.int32), ref.direction_table(64))
    np.testing.assert_array_equal(got["fit_status"].values, want[0][..., 0])
    assert got["x_fit"].values.tobytes() == (np.rint(given[:, None, 1] * 16) / 16.0 + want[1][..., 1]).tobytes()
    # the public call: the same numbers after restore_format, and through save / load, where the radii travel along
    mg.seed(99)
    public = mg.beads(data=data, **BEAD_KW, refine="edge")
    assert public.coords["radius_fit"].dims == ("mark",)
    assert public.coords["radius_fit"].values.tobytes() == xp.coords["radius_fit"].values[:, 0].tobytes()
    mg.save(tmp_path / "beads.nc", public)
    back = mg.load(tmp_path / "beads.nc")
    np.testing.assert_array_equal(back.coords["x_fit"].values, public.coords["x_fit"].values)
    np.testing.assert_array_equal(back.coords["radius"].values, public.coords["radius"].values)
    lost = plain.copy()
    del lost._cache["radius"]
    with pytest.raises(ValueError, match="radius="):
        mg.refine.refine_markers(lost)
    found = mg.refine.refine_markers(lost, radius=plain._cache["radius"])
    assert found.coords["x_fit"].values.tobytes() == xp.coords["x_fit"].values.tobytes()


def test_tracked_beads_end_to_end(hp):
    import magnify_amd as mg
    import track_ref as tr

    shape, n_beads, r_lo, r_hi, md, n_t = (256, 240), 12, 5, 12, 6, 3
    image, drawn, offsets = tr.scene(0, shape, n_beads, r_lo, r_hi, md, n_t, channels=2)
    data = mg.DataArray(data=image, dims=("channel", "time", "y", "x"), coords={"channel": ["c0", "c1"]})
    kw = dict(min_bead_diameter=2 * r_lo, max_bead_diameter=2 * r_hi, overlap=0, num_iter=60000, track="ncc", max_drift=md)

    def run(**more):
        mg.seed(99)
        pipe = mg.beads_pipe(**kw, **more)
        pipe.remove_pipe("restore_format")
        return pipe(data)

    xp, plain = run(search_channel="c1", refine="edge"), run(search_channel="c1")
    assert (xp.x.values[:, 0] != xp.x.values[:, -1]).any()  # circles of their own per timepoint
    for name in ("roi", "fg", "bg", "x", "y", "valid"):
        assert xp[name].values.tobytes() == plain[name].values.tobytes(), name
    step = dict(mg.beads_pipe(**kw, search_channel="c1", refine="edge").components)["refine_markers"]
    assert step.keywords["channel"] == "c1"  # the first search channel
    check_dataset(xp, plain._cache["radius"], channel=1)
    by_index = run(search_channel="c1", refine="edge", refine_channel=0, refine_rays=32)
    check_dataset(by_index, plain._cache["radius"], channel=0, rays=32)


def test_chip_end_to_end(hp, tmp_path):
    import magnify_amd as mg
    from synth import draw_chip

    kw = dict(shape=(3, 3), min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100, col_dist=100,
              num_iter=5000)
    data = mg.DataArray(data=draw_chip((3, 3), 20), dims=("y", "x"))

    def run(**more):
        mg.seed(4321)
        pipe = mg.microfluidic_chip_pipe(**kw, **more)
        pipe.remove_pipe("restore_format")
        return pipe(data)

    xp, plain = run(refine="edge"), run()
    for name in ("roi", "fg", "bg", "x", "y", "valid"):
        assert xp[name].values.tobytes() == plain[name].values.tobytes(), name
    radius = plain._cache["radius"].reshape(9, -1)  # (row, col, time)
    check_dataset(xp, radius)
    mg.seed(4321)
    public = mg.microfluidic_chip(data=data, **kw, refine="edge")
    for name in ("x_fit", "y_fit", "radius_fit", "fit_rms", "fit_strength", "fit_rays", "fit_status", "fit_polarity", "radius"):
        assert public.coords[name].dims == ("mark_row", "mark_col") and public.coords[name].shape == (3, 3), name
        assert public.coords[name].values.reshape(9).tobytes() == xp.coords[name].values[:, 0].tobytes(), name
    mg.save(tmp_path / "chip.nc", public)
    back = mg.load(tmp_path / "chip.nc")
    np.testing.assert_array_equal(back.coords["radius_fit"].values.reshape(9), public.coords["radius_fit"].values.reshape(9))
    np.testing.assert_array_equal(back.coords["fit_status"].values.reshape(9), public.coords["fit_status"].values.reshape(9))
