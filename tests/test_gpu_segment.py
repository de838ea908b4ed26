"""segment_rois on the GPU: mg_roi_threshold_masks against tests/segment_ref.py, bit for bit on all five outputs, at the
word boundaries of its bit planes; the component on a hand-built dataset (stale reductions); the public pipelines."""
import functools
import itertools

import numpy as np
import pytest

import segment_ref as ref

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 7, 31, 32, 33, 63, 64, 65, 72, 100, 127, 128)
DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
M, N_T = 5, 2


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def dev(a):
    import torch

    a = np.array(a, order="C")  # (a copy: the scenes are read-only)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


@functools.lru_cache(maxsize=None)
def scene(L, dtype_name, seed=0):
    """roi (M, N_T, L, L) of ``dtype`` and the drawn masks fg0, bg0, allowed (M, N_T, L, L) bool, read-only.  Windows:
    (0,0) a blob under the drawn disk; (0,1) a bar across the window -- it touches column 0 and L - 1, crosses every word
    seam and reaches farther than max_grow from the disk; (1,0) flat; (1,1) two-valued; (2,0) spots in two corners, at the
    centre and on the 31|32, 63|64, 95|96 seams; (2,1) an L along the border; (3,0) two blobs, one of them away from the
    disk; (3,1) only a blob away from the disk (floats: with an infinite pixel); (4,0) uint8 / uint16: the full range of
    the type, floats: all NaN; (4,1) a blob (floats: with NaN pixels, some of them on it)."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([seed, L, dtype.itemsize, dtype.kind == "f"])
    yy, xx = np.mgrid[0:L, 0:L]
    c, q, h = (L - 1) / 2, L // 2, max(L // 8, 1)
    r2 = (yy - c) ** 2 + (xx - c) ** 2
    roi = 100.0 + rng.poisson(20, (M, N_T, L, L))

    def blob(g, t, y0, y1, x0, x1, v=800.0):
        roi[g, t, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] += v

    blob(0, 0, q - h, q + h + 1, q - h, q + h + 1)
    blob(0, 1, q - 1, q + 2, 0, L)
    roi[1, 0] = 7.0
    roi[1, 1] = np.where(r2 <= (L / 3) ** 2, 1000.0, 0.0)
    blob(2, 0, 0, 3, 0, 4)
    blob(2, 0, L - 3, L, L - 4, L)
    blob(2, 0, q - 1, q + 2, q - 1, q + 2)
    for seam in (32, 64, 96):
        if seam < L:
            blob(2, 0, q - 2, q + 2, seam - 2, seam + 2)
    blob(2, 1, 0, L, 0, 3)
    blob(2, 1, 0, 3, 0, L)
    blob(2, 1, q - 1, q + 2, q - 1, q + 2)
    blob(3, 0, q - 2, q + 3, q - 2, q + 3)
    blob(3, 0, 1, 5, L - 6, L - 1)
    blob(3, 1, 1, 6, 1, 6)
    blob(4, 1, q - h, q + h + 1, q - h, q + h + 1)
    if dtype.kind == "u":
        top = np.iinfo(dtype).max
        if dtype.itemsize == 1:
            roi = roi / 4.0
        roi[4, 0].reshape(-1)[0] = 0.0
        roi[4, 0].reshape(-1)[-1] = float(top)
        roi = np.clip(np.rint(roi), 0, top)
    else:
        roi[3, 1].reshape(-1)[L * L // 3] = np.inf if dtype.itemsize == 4 else -np.inf
        roi[4, 0] = np.nan
        roi[4, 1][rng.random((L, L)) < 0.1] = np.nan
    roi = roi.astype(dtype)
    disk = r2 <= (L / 5) ** 2
    fg0 = np.stack([disk, np.roll(disk, 1, axis=1)])[None].repeat(M, axis=0)
    bg0 = np.stack([r2 > (L / 3) ** 2, np.roll(r2 > (L / 3) ** 2, 1, axis=0)])[None].repeat(M, axis=0)
    allowed = rng.random((M, N_T, L, L)) < 0.95
    for a in (roi, fg0, bg0, allowed):
        a.setflags(write=False)
    return roi, fg0, bg0, allowed


def compare(got, want, what):
    names = ("fg", "bg", "threshold", "counts", "segmented")
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        if name == "threshold":  # NaN where the window is unsegmented; every other value bit for bit
            np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: {name}")
            ok = ~np.isnan(w)
            assert g[ok].tobytes() == w[ok].tobytes(), (what, name, g, w)
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def run_and_check(hp, L, dtype, time_real, with_allowed, method, what, **kw):
    """One call on ``scene(L, dtype)`` against the reference; returns the kernel's outputs as NumPy arrays."""
    roi, fg0, bg0, allowed = scene(L, np.dtype(dtype).name)
    if not time_real:
        fg0, bg0, allowed = fg0[:, :1], bg0[:, :1], allowed[:, :1]
    want = ref.segment(roi, fg0, bg0, allowed if with_allowed else None, method=method, **kw)

    def mask(a):  # one mask for all timepoints: a view expanded along time, read in place
        return dev(a) if time_real else dev(a).expand(M, N_T, L, L)

    got = hp.threshold_masks(dev(roi), mask(fg0), mask(bg0), mask(allowed) if with_allowed else None, method=method, **kw)
    got = [g.cpu().numpy() for g in got]
    compare(got, want, what)
    return got


def number_for(dtype):
    return 120 if np.dtype(dtype) == np.uint8 else 500.5


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("L", LENGTHS)
def test_kernel_equals_reference(hp, L, dtype):
    i, j = LENGTHS.index(L), DTYPES.index(dtype)
    time_real, with_allowed, numeric = bool((i + j) % 2), bool((i // 2 + j) % 2), (i + j // 2) % 3 == 0
    method = number_for(dtype) if numeric else "otsu"
    got = run_and_check(hp, L, dtype, time_real, with_allowed, method, f"L={L} {np.dtype(dtype).name} {method}")
    seg = got[4]
    assert not seg[1, 0] and np.isnan(got[2][1, 0])  # the flat window
    if np.dtype(dtype).kind == "f":
        assert not seg[4, 0] and not seg[3, 1]  # all NaN; an infinite pixel
    if L >= 31 and not numeric:
        assert seg[0, 0] and seg[0, 1] and seg[3, 0]


@pytest.mark.parametrize("time_real,with_allowed,numeric", list(itertools.product((False, True), repeat=3)))
def test_every_mask_form_and_method(hp, time_real, with_allowed, numeric):
    for L, dtype in ((33, np.uint16), (72, np.float32)):
        method = number_for(dtype) if numeric else "otsu"
        run_and_check(hp, L, dtype, time_real, with_allowed, method, f"L={L} forms {time_real} {with_allowed} {method}")


@pytest.mark.parametrize("L", (33, 100))
def test_every_radius(hp, L):
    for open_radius, max_grow, bg_guard in itertools.product((0, 1, 3), (0, 1, 4, 32), (0, 2, 16)):
        run_and_check(hp, L, np.uint16, True, True, "otsu", f"L={L} open {open_radius} grow {max_grow} guard {bg_guard}",
                      open_radius=open_radius, max_grow=max_grow, bg_guard=bg_guard)


def test_the_bar_grows_by_max_grow_only(hp):
    L = 100
    seed = run_and_check(hp, L, np.uint16, False, False, "otsu", "grow 0", max_grow=0)
    small = run_and_check(hp, L, np.uint16, False, False, "otsu", "grow 4", max_grow=4)
    large = run_and_check(hp, L, np.uint16, False, False, "otsu", "grow 32", max_grow=32)
    cols = lambda fg: np.nonzero(fg[0, 1].any(axis=0))[0]  # noqa: E731
    # the bar reaches both borders; the mask reaches max_grow columns beyond the drawn disk on either side
    assert cols(seed[0]).min() == 30 and cols(seed[0]).max() == 69
    assert cols(small[0]).min() == 26 and cols(small[0]).max() == 73
    assert cols(large[0]).min() == 0 and cols(large[0]).max() == L - 1
    # the blob away from the drawn disk never becomes foreground; alone in its window it leaves the drawn masks
    assert not small[0][3, 0][:8, -8:].any() and not small[4][3, 1]


def test_min_area_forces_the_fallback(hp):
    roi, fg0, bg0, _ = scene(72, "uint16")
    got = run_and_check(hp, 72, np.uint16, True, False, "otsu", "min_area", min_area=10 ** 6)
    assert not got[4].any()
    np.testing.assert_array_equal(got[0], fg0.astype(np.uint8))
    np.testing.assert_array_equal(got[1], bg0.astype(np.uint8))
    assert np.isnan(got[2][1, 0]) and not np.isnan(np.delete(got[2].reshape(-1), 2)).any()  # the threshold found is kept


def test_two_calls_give_identical_bytes(hp):
    roi, fg0, bg0, allowed = scene(100, "float32")
    args = (dev(roi), dev(fg0), dev(bg0), dev(allowed))
    one = [g.cpu().numpy().tobytes() for g in hp.threshold_masks(*args)]
    two = [g.cpu().numpy().tobytes() for g in hp.threshold_masks(*args)]
    assert one == two


def test_a_channel_view_is_read_in_place(hp):
    import torch

    roi, fg0, bg0, _ = scene(33, "uint16")
    both = torch.stack([torch.zeros_like(dev(roi)), dev(roi)], dim=1)  # (M, C, T, L, L): channel 1 is the scene
    view = both[:, 1]
    assert not view.is_contiguous()
    got = hp.threshold_masks(view, dev(fg0), dev(bg0))
    compare(got, ref.segment(roi, fg0, bg0), "channel view")


def test_no_markers(hp):
    import torch

    empty = torch.empty((0, 2, 9, 9), dtype=torch.float32, device="cuda")
    masks = torch.empty((0, 2, 9, 9), dtype=torch.bool, device="cuda")
    fg, bg, thr, counts, seg = hp.threshold_masks(empty, masks, masks)
    assert fg.shape == (0, 2, 9, 9) and bg.shape == (0, 2, 9, 9) and thr.shape == (0, 2) and counts.shape == (0, 2, 2)
    assert seg.shape == (0, 2) and thr.dtype == torch.float64 and counts.dtype == torch.int32


def test_invalid_arguments_write_nothing(hp):
    import torch

    from magnify_amd import _native as nat

    L, m, n_t = 9, 2, 2
    roi = torch.zeros((m, n_t, L, L), dtype=torch.float32, device="cuda")
    mask = torch.ones((m, n_t, L, L), dtype=torch.uint8, device="cuda")
    outs = {"fg": torch.full((m, n_t, L, L), 0xAB, dtype=torch.uint8, device="cuda"),
            "bg": torch.full((m, n_t, L, L), 0xAB, dtype=torch.uint8, device="cuda"),
            "thr": torch.full((m, n_t), -7.0, dtype=torch.float64, device="cuda"),
            "counts": torch.full((m, n_t, 2), -7, dtype=torch.int32, device="cuda"),
            "seg": torch.full((m, n_t), 0xAB, dtype=torch.uint8, device="cuda")}
    before = {k: v.clone() for k, v in outs.items()}
    n = L * L
    good = dict(roi=roi.data_ptr(), dtype=nat.MG_F32, sm=n_t * n, st=n, fg0=mask.data_ptr(), fsm=n_t * n, fst=n,
                bg0=mask.data_ptr(), bsm=n_t * n, bst=n, allowed=0, asm=0, ast=0, m=m, n_t=n_t, L=L, otsu=1, number=0.0,
                open_radius=1, max_grow=4, bg_guard=2, min_area=1, fg=outs["fg"].data_ptr(), bg=outs["bg"].data_ptr(),
                thr=outs["thr"].data_ptr(), counts=outs["counts"].data_ptr(), seg=outs["seg"].data_ptr())
    bad = [dict(roi=0), dict(fg0=0), dict(bg0=0), dict(fg=0), dict(bg=0), dict(thr=0), dict(counts=0), dict(seg=0),
           dict(dtype=99), dict(m=-1), dict(n_t=0), dict(n_t=-1), dict(L=0), dict(L=129), dict(m=2 ** 16, n_t=2 ** 15),
           dict(sm=-1), dict(st=-1), dict(fsm=-1), dict(fst=-1), dict(bsm=-1), dict(bst=-1), dict(asm=-1), dict(ast=-1),
           dict(open_radius=-1), dict(open_radius=9), dict(max_grow=-1), dict(max_grow=33), dict(bg_guard=-1),
           dict(bg_guard=17), dict(min_area=-1), dict(otsu=0, number=float("nan"))]
    for change in bad:
        with pytest.raises(ValueError):
            hp._call("mg_roi_threshold_masks", *{**good, **change}.values(), hp._stream())
    hp._call("mg_roi_threshold_masks", *{**good, "m": 0}.values(), hp._stream())  # no markers: MG_OK, nothing written
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], before[k]), k
    for bad_kw in (dict(method="li"), dict(open_radius=9), dict(max_grow=33), dict(bg_guard=-1), dict(min_area=-1)):
        with pytest.raises(ValueError):
            hp.threshold_masks(roi, mask, mask, **bad_kw)
    with pytest.raises(ValueError):
        big = torch.zeros((1, 1, 129, 129), dtype=torch.float32, device="cuda")
        hp.threshold_masks(big, big.to(torch.uint8), big.to(torch.uint8))


# ---- the component on a hand-built dataset ----------------------------------------------------------------------------

DIM = ["roi_y", "roi_x"]


@pytest.fixture(scope="module")
def built(hp):
    """A bead-like dataset (no ``tag``) whose cache holds the finder's reductions of the DRAWN masks, and the result of
    ``segment_rois`` on it."""
    import torch

    import magnify_amd as mg

    L = 33
    roi1, fg0, bg0, _ = scene(L, "uint16")
    roi0 = scene(L, "uint16", seed=1)[0]
    roi = np.stack([roi0, roi1], axis=1)  # (M, C, T, L, L): channel "b" decides
    fg0, bg0 = fg0.copy(), bg0.copy()
    fg0[0, :, :, :L // 2 - 1] = False  # the bar's left half is neither drawn fg nor drawn bg: not allowed
    bg0[0, :, :, :L // 2 - 1] = False
    ds = mg.Dataset({"roi": mg.DataArray(dev(roi), ("mark", "channel", "time", "roi_y", "roi_x"))},
                    coords={"fg": (("mark", "time", "roi_y", "roi_x"), dev(fg0)),
                            "bg": (("mark", "time", "roi_y", "roi_x"), dev(bg0)),
                            "valid": (("mark", "time"), np.ones((M, N_T), dtype=bool)),
                            "x": (("mark", "time"), np.zeros((M, N_T))), "y": (("mark", "time"), np.zeros((M, N_T))),
                            "channel": np.array(["a", "b"])})
    both = np.stack([fg0, bg0], axis=-1)  # (M, T, L, L, 2)
    sums = np.einsum("mctyx,mtyxk->mctk", roi.astype(np.float64), both.astype(np.float64))
    ds._cache["roi_sums"] = torch.from_numpy(sums).cuda()
    ds._cache["roi_counts"] = torch.from_numpy(both.sum(axis=(2, 3)).astype(np.int32)).cuda()
    out = mg.segment.segment_rois(ds, channel="b")
    want = ref.segment(roi1, fg0, bg0, fg0 | bg0)
    return ds, out, roi, want


def test_component_replaces_the_masks(built):
    import torch

    ds, out, roi, want = built
    for name, w in (("fg", want[0]), ("bg", want[1])):
        arr = out.coords[name]
        assert arr.dims == ("mark", "time", "roi_y", "roi_x") and isinstance(arr.raw, torch.Tensor) and arr.raw.is_cuda
        assert arr.raw.dtype == torch.bool
        np.testing.assert_array_equal(arr.values, w.astype(bool))
    np.testing.assert_array_equal(out.segmented.values, want[4].astype(bool))
    assert out.segmented.values.dtype == bool and out.seg_threshold.values.dtype == np.float64
    np.testing.assert_array_equal(out.seg_threshold.values, want[2])
    assert out.segmented.dims == ("mark", "time") and out.seg_threshold.dims == ("mark", "time")
    assert want[4].any() and not want[4].all() and (want[0] != ds.fg.values).any()
    assert not want[0][0, :, :, :33 // 2 - 1].any()  # what is not allowed never becomes foreground
    for name in ("valid", "x", "y", "roi"):
        assert out[name].raw is ds[name].raw
    assert ds.fg.values.tobytes() != out.fg.values.tobytes() and "segmented" not in ds.coords  # the input is left alone


def test_no_reduction_answers_for_the_old_masks(built):
    from magnify_amd import reduce

    ds, out, roi, want = built
    assert "roi_sums" in ds._cache and "roi_sums" not in out._cache
    values = roi.astype(np.float64)
    for k, name in enumerate(("fg", "bg")):
        mask = want[k].astype(bool)[:, None]  # (M, 1, T, L, L)
        held = np.where(mask, values, np.nan)
        count = want[k].sum(axis=(-1, -2))
        np.testing.assert_array_equal(reduce.counts(out, name).values, count)
        np.testing.assert_array_equal(count, want[3][..., k])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(mask, values, 0.0).sum(axis=(-1, -2)) / count[:, None]
        np.testing.assert_array_equal(reduce.masked_mean(out, name).values, mean)
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            median, std = np.nanmedian(held, axis=(-1, -2)), np.nanstd(held, axis=(-1, -2))
        np.testing.assert_array_equal(reduce.masked_median(out, name).values, median)
        got = out.roi.where(out[name]).std(dim=DIM).values
        np.testing.assert_allclose(got, std, rtol=1e-12, atol=0, equal_nan=True)
    # and they differ from what the finder had cached
    assert (reduce.counts(out, "fg").values != reduce.counts(ds, "fg").values).any()


def test_new_coordinates_survive_save_and_load(built, tmp_path):
    import magnify_amd as mg

    _, out, _, want = built
    mg.save(tmp_path / "segmented.nc", out)
    back = mg.load(tmp_path / "segmented.nc")
    np.testing.assert_array_equal(back.segmented.values, want[4].astype(bool))
    np.testing.assert_array_equal(back.seg_threshold.values, want[2])
    assert back.segmented.dims == ("mark", "time") and back.seg_threshold.values.dtype == np.float64
    np.testing.assert_array_equal(back.fg.values, want[0].astype(bool))
    np.testing.assert_array_equal(back.bg.values, want[1].astype(bool))


def test_component_channel_lookup_and_no_markers(built):
    import magnify_amd as mg

    ds, out, _, _ = built
    by_index = mg.segment.segment_rois(ds, channel=1)
    assert by_index.fg.values.tobytes() == out.fg.values.tobytes()
    first = mg.segment.segment_rois(ds)
    assert first.fg.values.tobytes() == mg.segment.segment_rois(ds, channel="a").fg.values.tobytes()
    with pytest.raises(ValueError):
        mg.segment.segment_rois(ds, channel="gfp")
    with pytest.raises(ValueError):
        mg.segment.segment_rois(ds, open_radius=9)
    L = ds.sizes["roi_y"]
    empty = mg.Dataset({"roi": mg.DataArray(np.zeros((0, 2, N_T, L, L), dtype=np.uint16),
                                            ("mark", "channel", "time", "roi_y", "roi_x"))},
                       coords={"fg": (("mark", "time", "roi_y", "roi_x"), np.zeros((0, N_T, L, L), dtype=bool)),
                               "bg": (("mark", "time", "roi_y", "roi_x"), np.zeros((0, N_T, L, L), dtype=bool))})
    none = mg.segment.segment_rois(empty)
    assert none.segmented.values.shape == (0, N_T) and none.segmented.values.dtype == bool
    assert none.seg_threshold.values.shape == (0, N_T) and none.fg.values.shape[0] == 0


# ---- end to end: the public pipelines ------------------------------------------------------------------------------------

CHIP_KW = dict(shape=(4, 4), min_button_diameter=16, max_button_diameter=32, overlap=0, row_dist=100, col_dist=100,
               num_iter=5000, search_channel="button")
ELLIPTICAL = {(0, 1), (1, 2), (2, 0), (3, 3), (2, 2)}
BLANK = (1, 1)


@pytest.fixture(scope="module")
def chip_runs(hp):
    """A noise-free two-channel chip: round buttons in "button"; in "bound" spots at the same centres, elliptical
    (semi-axes 15 x 5) on some chambers, round on others, nothing on one."""
    import magnify_amd as mg
    from synth import draw_chip

    buttons = draw_chip((4, 4), 20)
    bound = np.zeros_like(buttons)
    yy, xx = np.mgrid[0:buttons.shape[0], 0:buttons.shape[1]]
    for i, j in itertools.product(range(4), range(4)):
        cy, cx = 100 * (i + 1), 100 * (j + 1)
        if (i, j) == BLANK:
            continue
        if (i, j) in ELLIPTICAL:
            bound[((yy - cy) / 5.0) ** 2 + ((xx - cx) / 15.0) ** 2 <= 1.0] = 1000
        else:
            bound[(yy - cy) ** 2 + (xx - cx) ** 2 <= 100] = 1000
    data = mg.DataArray(data=np.stack([buttons, bound]), dims=("channel", "y", "x"), coords={"channel": ["button", "bound"]})

    def run(**kw):  # (before restore_format squeezes the time axis the filters want)
        mg.seed(4321)
        pipe = mg.microfluidic_chip_pipe(**CHIP_KW, **kw)
        pipe.remove_pipe("restore_format")
        return pipe(data)

    mg.seed(4321)
    public = mg.microfluidic_chip(data=data, **CHIP_KW, segment="otsu", segment_channel="bound")
    mg.seed(4321)
    public_plain = mg.microfluidic_chip(data=data, **CHIP_KW, segment=None)
    return run(segment="otsu", segment_channel="bound"), run(segment=None), run(), public, public_plain


def test_chip_end_to_end(chip_runs):
    import magnify_amd as mg

    seg, plain, today, public, public_plain = chip_runs
    for name in ("fg", "bg", "roi", "x", "y", "valid"):  # segment=None: the bytes of today's call
        assert plain[name].values.tobytes() == today[name].values.tobytes(), name
        assert public_plain[name].values.tobytes() == today[name].values.tobytes(), name
        assert public[name].values.tobytes() == seg[name].values.tobytes(), name
    assert "segmented" not in plain.coords and "seg_threshold" not in plain.coords
    assert public.segmented.values.tobytes() == seg.segmented.values.tobytes()
    for name in ("roi", "x", "y", "valid"):
        assert seg[name].values.tobytes() == plain[name].values.tobytes(), name
    s, p = seg.unstack().transpose("mark_row", "mark_col", ...), plain.unstack().transpose("mark_row", "mark_col", ...)
    roi = s.roi.values  # (4, 4, C, T, L, L)
    L = roi.shape[-1]
    fg0, bg0 = p.fg.values.reshape(16, 1, L, L), p.bg.values.reshape(16, 1, L, L)
    want = ref.segment(roi[:, :, 1].reshape(16, 1, L, L), fg0, bg0)  # (chips: no `allowed`)
    np.testing.assert_array_equal(s.fg.values.reshape(16, 1, L, L), want[0].astype(bool))
    np.testing.assert_array_equal(s.bg.values.reshape(16, 1, L, L), want[1].astype(bool))
    np.testing.assert_array_equal(s.segmented.values.reshape(16, 1), want[4].astype(bool))
    np.testing.assert_array_equal(s.seg_threshold.values.reshape(16, 1), want[2])
    segmented = s.segmented.values[:, :, 0]
    assert not segmented[BLANK] and segmented.sum() == 15
    assert s.fg.values[BLANK].tobytes() == p.fg.values[BLANK].tobytes()
    assert s.bg.values[BLANK].tobytes() == p.bg.values[BLANK].tobytes()
    for ij in ELLIPTICAL:
        assert s.fg.values[ij].sum() != p.fg.values[ij].sum()
    np.testing.assert_array_equal(mg.reduce.counts(seg, "fg").values.reshape(4, 4), s.fg.values.sum(axis=(-1, -2, -3)))
    # filter_nonround, as it stands, now has something to reject
    kept = mg.filter.filter_nonround(seg).unstack().transpose("mark_row", "mark_col", ...).valid.values[:, :, 0]
    for i, j in itertools.product(range(4), range(4)):
        assert kept[i, j] == ((i, j) not in ELLIPTICAL), (i, j)
    assert mg.filter.filter_nonround(plain).valid.values.all()


BEAD_R = 12
BEAD_CENTRES = np.array([(60, 60), (60, 170), (160, 60), (160, 85), (250, 200), (240, 110)])  # beads 2 and 3 touch
BEAD_KW = dict(min_bead_diameter=16, max_bead_diameter=32, overlap=0, num_iter=60000)


@pytest.fixture(scope="module")
def bead_runs(hp):
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

    mg.seed(99)
    public = mg.beads(data=data, **BEAD_KW, segment="otsu")
    return run(segment="otsu"), run(), public


def test_beads_end_to_end(bead_runs):
    seg, plain, public = bead_runs
    assert public.fg.values.tobytes() == seg.fg.values.tobytes() and "segmented" in public.coords
    np.testing.assert_array_equal(seg.x.values, plain.x.values)
    np.testing.assert_array_equal(seg.y.values, plain.y.values)
    assert seg.roi.values.tobytes() == plain.roi.values.tobytes()
    found = np.stack([seg.y.values[:, 0], seg.x.values[:, 0]], axis=1)
    dist = np.linalg.norm(found[:, None] - BEAD_CENTRES[None], axis=2)
    which = dist.argmin(axis=0)  # the found bead of every drawn one
    assert (dist.min(axis=0) <= 3).all(), dist.min(axis=0)
    fg, bg, fg0, bg0 = seg.fg.values, seg.bg.values, plain.fg.values, plain.bg.values
    roi = seg.roi.values
    want = ref.segment(roi[:, 0], fg0, bg0, fg0 | bg0)
    np.testing.assert_array_equal(fg, want[0].astype(bool))
    np.testing.assert_array_equal(bg, want[1].astype(bool))
    assert seg.segmented.values[which].all()
    assert not (fg & ~(fg0 | bg0)).any() and not (bg & ~bg0).any()
    L = fg.shape[-1]
    yy, xx = np.mgrid[0:L, 0:L]
    radius = np.asarray(seg._cache["radius"])
    for a, b in ((2, 3), (3, 2)):  # in the window of bead a, nothing of its mask lies in the (found) disk of bead b
        i, j = which[a], which[b]
        dy, dx = found[j] - found[i]
        other = (yy - (L // 2 + dy)) ** 2 + (xx - (L // 2 + dx)) ** 2 <= (radius[j] - 1) ** 2
        on = roi[i, 0, 0] > seg.seg_threshold.values[i, 0]
        assert (on & other).sum() > 150 and not (fg[i, 0] & other).any()
        area = fg[i, 0].sum()
        assert 0.8 * np.pi * BEAD_R ** 2 < area < 1.2 * np.pi * BEAD_R ** 2


def test_tracked_beads_end_to_end(hp):
    import magnify_amd as mg
    import track_ref as tr

    shape, n_beads, r_lo, r_hi, md, n_t = (256, 240), 12, 5, 12, 6, 3
    image, drawn, offsets = tr.scene(0, shape, n_beads, r_lo, r_hi, md, n_t, channels=2)
    data = mg.DataArray(data=image, dims=("channel", "time", "y", "x"), coords={"channel": ["c0", "c1"]})
    kw = dict(min_bead_diameter=2 * r_lo, max_bead_diameter=2 * r_hi, overlap=0, num_iter=60000, search_channel="c0",
              track="ncc", max_drift=md)

    def run(**more):
        mg.seed(99)
        pipe = mg.beads_pipe(**kw, **more)
        pipe.remove_pipe("restore_format")
        return pipe(data)

    seg, plain = run(segment="otsu", segment_channel="c0"), run()
    assert plain.coords["fg"].data.stride(1) != 0  # masks of their own per timepoint on input
    np.testing.assert_array_equal(seg.x.values, plain.x.values)
    fg0, bg0 = plain.fg.values, plain.bg.values
    want = ref.segment(seg.roi.values[:, 0], fg0, bg0, fg0 | bg0)
    np.testing.assert_array_equal(seg.fg.values, want[0].astype(bool))
    np.testing.assert_array_equal(seg.bg.values, want[1].astype(bool))
    np.testing.assert_array_equal(seg.segmented.values, want[4].astype(bool))
    assert seg.segmented.values.shape == (len(fg0), n_t) and seg.segmented.values.any()
    np.testing.assert_array_equal(mg.reduce.counts(seg, "fg").values, want[3][..., 0])
    np.testing.assert_array_equal(seg.track_score.values, plain.track_score.values)
