"""``find_beads(track="ncc")`` on the device against its NumPy restatement (tests/track_ref.py): the sums, scores and
picks of mg_track_beads, and the component end to end on the scenes of tests/test_cpu_track.py.

Tolerances.  Integer-valued pixels: sums and fixed equal bit for bit (every float64 partial sum is an exact integer
below 2^53, in any order); fractional float pixels: |err| <= 4 n 2^-53 |sum| per entry, the bound for two differently
ordered float64 sums of n non-negative terms.  Scores: one ulp of the restatement's operations on the same sums (fractional
pixels: on the sums the device made).  Shifts: equal wherever the restatement's best two scores differ by more than 4 ulp
(fractional pixels: by more than 1e-6); the inputs are built so that this is every (bead, time)."""
import numpy as np
import pytest

import track_ref as tr
from oracle import ref_numeric as rn
from oracle import ref_pipeline as rp

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "uint16", "float32", "float64"]
# interior; near the corner; clipped on two sides; the last pixel; nowhere near the image (an empty patch for every
# half); one whose patch overlaps the first one's
BEADS = np.array([[48, 40, 6], [3, 4, 5], [90, 5, 7], [95, 79, 5], [-40, 30, 6], [50, 43, 8]])
CONFIGS = [(4, 1), (12, 3), (12, 8)]  # (half, m): 9, 49 and 289 displacements -- the last more than one pass of 256


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return magnify_amd


def _moved_planes(rng, top, shape=(96, 80), moves=((0, 0), (1, -1), (-3, 2))):
    """T planes of integers in [0, top]: plane t is plane 0 rolled by moves[t], a tenth of the pixels drawn afresh."""
    base = rng.integers(0, top + 1, size=shape)
    planes = []
    for dy, dx in moves:
        p = np.roll(base, (dy, dx), axis=(0, 1))
        fresh = rng.random(shape) < 0.1
        planes.append(np.where(fresh, rng.integers(0, top + 1, size=shape), p))
    return np.stack(planes)


_VALUES, _WANT = {}, {}


def _values(top):
    if top not in _VALUES:
        _VALUES[top] = _moved_planes(np.random.default_rng(top), top)
    return _VALUES[top]


def _want(top, half, m, t_ref):
    """The restatement on the integer planes, made once per (values, configuration) and shared by the dtypes."""
    key = (top, half, m, t_ref)
    if key not in _WANT:
        _WANT[key] = tr.track(_values(top).astype(np.uint16), BEADS, half, m, t_ref)
    return _WANT[key]


def _device(planes, beads, half, m, t_ref=0):
    """mg_track_beads twice: the same bits; the results on the host."""
    import torch

    from magnify_amd import track

    dev = planes if isinstance(planes, torch.Tensor) else torch.from_numpy(planes).cuda()
    first = {k: v.cpu().numpy() for k, v in track.track_beads(dev, beads, half, m, t_ref, want_sums=True).items()}
    again = track.track_beads(dev, beads, half, m, t_ref, want_sums=True)
    for k, v in first.items():
        assert v.tobytes() == again[k].cpu().numpy().tobytes(), k
    plain = track.track_beads(dev, beads, half, m, t_ref)  # the product's call: no sums
    assert set(plain) == {"shift", "score"}
    for k in plain:
        assert first[k].tobytes() == plain[k].cpu().numpy().tobytes(), k
    return first


def _compare(got, want, what, exact=True, min_gap=None):
    m_beads, n_t = want["score"].shape
    assert got["shift"].shape == (m_beads, n_t, 2) and got["shift"].dtype == np.int32, what
    assert got["score"].shape == (m_beads, n_t) and got["score"].dtype == np.float64, what
    assert got["sums"].shape == want["sums"].shape and got["fixed"].shape == want["fixed"].shape, what
    if exact:
        np.testing.assert_array_equal(got["sums"], want["sums"].astype(got["sums"].dtype), err_msg=what)
        np.testing.assert_array_equal(got["fixed"], want["fixed"].astype(got["fixed"].dtype), err_msg=what)
    else:
        n = want["fixed"][:, 0]
        np.testing.assert_array_equal(got["fixed"][:, 0], n, err_msg=what)
        for name, count in (("sums", n[:, None, None, None, None]), ("fixed", n[:, None])):
            err = np.abs(got[name] - want[name])
            bound = 4 * count * 2.0**-53 * np.abs(want[name])
            print(what, name, "max error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (what, name)
    # scores: the restatement's operations on the restatement's sums -- or, where the sums may differ in the last bits
    # (fractional pixels), on the device's own
    want_score = want["score"] if exact else tr.pick(tr.scores(got["sums"], got["fixed"]), int(np.argmax(np.isinf(want["gap"][0]))))[1]
    ulp = np.spacing(np.abs(want_score))
    err = np.abs(got["score"] - want_score)
    print(what, "score error in ulp, max", float(np.max(err / ulp)))
    assert np.all(err <= ulp), what
    # shifts: wherever the best score leads (row t_ref: gap = inf); and where every score is 0 (flat or empty patches),
    # which the tie-break decides
    clear = (want["gap"] > (4 * ulp if min_gap is None else min_gap)) | (want["z"] == 0).all(axis=(-1, -2))
    print(what, "pairs compared", int(clear.sum()), "of", clear.size)
    assert clear.all(), what  # (at most 1 % may be left out; the inputs leave none out)
    np.testing.assert_array_equal(got["shift"][clear], want["shift"][clear], err_msg=what)


# ---- 1. sums, scores and picks ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_scores_and_picks_equal_the_restatement(mg, dtype):
    top = 255 if dtype == "uint8" else 4000
    planes = _values(top).astype(dtype)
    for half, m in CONFIGS:
        for t_ref in (0, 2):
            got = _device(planes, BEADS, half, m, t_ref)
            want = _want(top, half, m, t_ref)
            integer = np.dtype(dtype).kind == "u"
            assert got["sums"].dtype == got["fixed"].dtype == (np.int64 if integer else np.float64)
            _compare(got, want, f"{dtype} half={half} m={m} t_ref={t_ref}")
            # what the scene is: the interior bead follows the rolls
            moves = np.array([(0, 0), (1, -1), (-3, 2)])
            within = (np.abs(moves - moves[t_ref]) <= m).all(axis=1)
            np.testing.assert_array_equal(got["shift"][0][within], (moves - moves[t_ref])[within])
            # the empty patch
            assert not got["fixed"][4].any() and not got["sums"][4].any() and not got["shift"][4].any()
            assert got["score"][4].tolist() == [1.0 if t == t_ref else 0.0 for t in range(3)]


# ---- 2. the largest supported shape ------------------------------------------------------------------------------------


def test_the_largest_patch_and_window_at_full_scale_values(mg):
    """half = 47, m = 16 on 160 x 160 uint16 with values up to 65535: 95^2 template, 127^2 window, 1089 displacements;
    plane 2 is 65535 everywhere, so sum A^2 (and, with t_ref = 2, sum A B) reaches 9025 * 65535^2."""
    rng = np.random.default_rng(65535)
    planes = _moved_planes(rng, 65535, (160, 160), ((0, 0), (5, -7), (0, 0)))
    planes[2] = 65535
    planes[0, 80, 80] = 65535
    planes = planes.astype(np.uint16)
    bead = np.array([[80, 80, 40]])
    for t_ref in (0, 2):
        got = _device(planes, bead, 47, 16, t_ref)
        want = tr.track(planes, bead, 47, 16, t_ref)
        _compare(got, want, f"largest t_ref={t_ref}")
    assert got["sums"][0, 2, 16, 16].tolist() == [9025 * 65535, 9025 * 65535**2, 9025 * 65535**2]
    first = _device(planes, bead, 47, 16, 0)
    assert first["shift"][0].tolist() == [[0, 0], [5, -7], [0, 0]] and first["score"][0, 2] == 0.0


# ---- 3. fractional float pixels -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fractional_float_pixels(mg, dtype):
    rng = np.random.default_rng(3)
    planes = (_moved_planes(rng, 4000) + rng.random((3, 96, 80))).astype(dtype)  # non-negative
    for half, m in ((12, 3), (12, 8)):
        got = _device(planes, BEADS, half, m)
        want = tr.track(planes, BEADS, half, m)
        _compare(got, want, f"fractional {dtype} half={half} m={m}", exact=False, min_gap=1e-6)


# ---- 4. a plane-strided view ----------------------------------------------------------------------------------------------


def test_a_channel_of_a_larger_tensor_is_read_where_it_lies(mg):
    import torch

    from magnify_amd import track

    rng = np.random.default_rng(4)
    image = np.stack([_moved_planes(rng, 4000), _moved_planes(rng, 4000)]).astype(np.uint16)  # (2, 3, 96, 80)
    dev = torch.from_numpy(image).cuda()
    view = dev[1]
    assert view.data_ptr() != dev.data_ptr() and view.stride(0) == 96 * 80
    every_other = torch.from_numpy(np.ascontiguousarray(image.transpose(1, 0, 2, 3))).cuda()[:, 1]  # plane stride 2 h w
    assert every_other.stride(0) == 2 * 96 * 80 and not every_other.is_contiguous()
    want = _device(np.ascontiguousarray(image[1]), BEADS, 12, 3)
    for planes in (view, every_other):
        got = track.track_beads(planes, BEADS, 12, 3, want_sums=True)
        for k, v in want.items():
            assert v.tobytes() == got[k].cpu().numpy().tobytes(), k


# ---- 5. ties and flat planes -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(tr.TIES))
def test_an_exact_tie_goes_to_the_smaller_displacement(mg, name):
    planes, want_shift = tr.TIES[name]
    got = _device(planes, tr.TIE_BEAD, tr.TIE_HALF, tr.TIE_M)
    want = tr.track(planes, tr.TIE_BEAD, tr.TIE_HALF, tr.TIE_M)
    np.testing.assert_array_equal(got["sums"], want["sums"])
    assert tuple(got["shift"][0, 1]) == want_shift == tuple(want["shift"][0, 1]), name
    assert got["score"][0, 1] == want["score"][0, 1], name


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_planes_and_empty_patches_give_shift_0_and_score_0(mg, dtype):
    flat = np.full((3, 48, 40), 77, dtype=dtype)
    got = _device(flat, np.array([[24, 20, 5]]), 6, 3)
    assert not got["shift"].any() and got["score"][0].tolist() == [1.0, 0.0, 0.0] and got["fixed"][0, 0] == 169
    planes = np.random.default_rng(0).integers(0, 200, size=(2, 48, 40)).astype(dtype)
    got = _device(planes, np.array([[0, 0, 5]]), 4, 8)  # rows / columns <= 4 and >= 8: an empty patch
    assert not got["fixed"].any() and not got["sums"].any() and not got["shift"].any()
    assert got["score"][0].tolist() == [1.0, 0.0]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------


def test_the_entry_point_refuses_what_it_cannot_do(mg):
    import torch

    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    planes = torch.from_numpy(_values(4000).astype(np.uint16)).cuda()
    beads = torch.from_numpy(BEADS.astype(np.int32)).cuda()
    shift = torch.full((6, 3, 2), 99, dtype=torch.int32, device="cuda")
    score = torch.full((6, 3), -5.0, dtype=torch.float64, device="cuda")

    def call(dtype=nat.MG_U16, n_t=3, h=96, w=80, t_ref=0, m=6, half=12, md=3, p=planes, b=beads, sh=shift, sc=score):
        return nat.lib().mg_track_beads(p.data_ptr() if p is not None else 0, dtype, n_t, 96 * 80, h, w, t_ref,
                                        b.data_ptr() if b is not None else 0, m, half, md,
                                        sh.data_ptr() if sh is not None else 0, sc.data_ptr() if sc is not None else 0, 0, 0,
                                        hotpath._stream())

    bad = [dict(md=0), dict(md=17), dict(half=0), dict(half=48), dict(half=47, md=17), dict(half=48, md=16), dict(t_ref=-1),
           dict(t_ref=3), dict(n_t=0), dict(h=0), dict(w=0), dict(m=-1), dict(dtype=7), dict(p=None), dict(b=None),
           dict(sh=None), dict(sc=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (shift == 99).all() and (score == -5.0).all()  # nothing was launched
    assert call(m=0) == 0
    torch.cuda.synchronize()
    assert (shift == 99).all() and (score == -5.0).all()
    assert call(n_t=1) == 0  # a single timepoint: row t_ref of every bead
    torch.cuda.synchronize()
    flat_shift, flat_score = shift.reshape(-1), score.reshape(-1)
    assert not flat_shift[:12].any() and (flat_shift[12:] == 99).all()
    assert (flat_score[:6] == 1.0).all() and (flat_score[6:] == -5.0).all()
    assert call(half=47, md=16) == 0 and call(t_ref=2) == 0


# ---- 7 - 9. end to end ---------------------------------------------------------------------------------------------------

SHAPE, N_BEADS, R_LO, R_HI, M, N_T = (256, 240), 12, 5, 12, 6, 4  # the first scene of tests/test_cpu_track.py
KW = dict(min_bead_diameter=2 * R_LO, max_bead_diameter=2 * R_HI, overlap=0, num_iter=60000, search_channel="c0")


def _beads(mg, image, restore=False, **kw):
    data = mg.DataArray(data=image, dims=("channel", "time", "y", "x"), coords={"channel": ["c0", "c1"]})
    mg.seed(99)
    if restore:
        return mg.beads(data=data, **KW, **kw)
    pipe = mg.beads_pipe(**KW, **kw)
    pipe.remove_pipe("restore_format")
    return pipe(data)


@pytest.fixture(scope="module")
def followed(mg):
    image, drawn, offsets = tr.scene(0, SHAPE, N_BEADS, R_LO, R_HI, M, N_T, channels=2)
    return image, drawn, offsets, _beads(mg, image, track="ncc", max_drift=M)


def _match(xp, drawn):
    """Index of the drawn bead under every found one (time 0)."""
    found = np.stack([xp.y.values[:, 0], xp.x.values[:, 0]], axis=1)
    dist = np.linalg.norm(found[:, None] - drawn[None, :, :2], axis=2)
    which = dist.argmin(axis=1)
    assert (dist.min(axis=1) <= 3).all() and len(set(which.tolist())) == len(which)
    assert len(which) >= 3 * len(drawn) // 4
    return which


def _oracle_rois(image_t, table, L):
    """The oracle's single-timepoint bead ROI path (oracle/ref_pipeline.py find_beads: circle_labels, bounding_box, the
    == i / == -1 tests) on ``image_t (C, h, w)`` with the bead table ``table``."""
    n_c, h, w = image_t.shape
    labels = rn.circle_labels(table.astype(int), h, w)
    roi = np.zeros((len(table), n_c, L, L), dtype=image_t.dtype)
    fg, bg = np.zeros((len(table), L, L), dtype=bool), np.zeros((len(table), L, L), dtype=bool)
    for i, (row, col, _) in enumerate(table):
        top, bottom, left, right = rn.bounding_box(round(float(col)), round(float(row)), L, w, h)
        roi[i], fg[i], bg[i] = image_t[:, top:bottom, left:right], labels[top:bottom, left:right] == i, labels[top:bottom, left:right] == -1
    return roi, fg, bg


def test_followed_beads_end_to_end(mg, followed):
    import torch

    image, drawn, offsets, xp = followed
    which = _match(xp, drawn)
    x, y = xp.x.values, xp.y.values
    np.testing.assert_array_equal(y - y[:, :1], offsets[which][..., 0])
    np.testing.assert_array_equal(x - x[:, :1], offsets[which][..., 1])
    np.testing.assert_array_equal(xp.track_shift_y.values, offsets[which][..., 0])
    np.testing.assert_array_equal(xp.track_shift_x.values, offsets[which][..., 1])
    assert xp.track_shift_y.values.dtype == np.int32 and xp.track_score.values.dtype == np.float64
    assert xp.valid.values.all() and (xp.track_score.values > 0.99).all()
    assert xp.fg.dims == ("mark", "time", "roi_y", "roi_x") and xp.roi.dims == ("mark", "channel", "time", "roi_y", "roi_x")
    m, L = len(which), 2 * 2 * R_HI
    radius = xp._cache["radius"]
    roi, fg, bg = xp.roi.values, xp.fg.values, xp.bg.values
    assert fg.shape == (m, N_T, L, L) and fg.dtype == bool
    sums, counts = xp._cache["roi_sums"].cpu().numpy(), xp._cache["roi_counts"].cpu().numpy()
    assert sums.shape == (m, 2, N_T, 2) and counts.shape == (m, N_T, 2)
    for t in range(N_T):
        table = np.column_stack([y[:, t], x[:, t], radius]).astype(np.int64)
        want_roi, want_fg, want_bg = _oracle_rois(image[:, t], table, L)
        assert roi[:, :, t].tobytes() == want_roi.tobytes(), t
        assert fg[:, t].tobytes() == want_fg.tobytes() and bg[:, t].tobytes() == want_bg.tobytes(), t
        red = rp.roi_reduce(want_roi[:, :, None], want_fg[:, None], want_bg[:, None], medians=False)
        np.testing.assert_array_equal(sums[:, :, t, 0], red["fg_sum"][:, :, 0])
        np.testing.assert_array_equal(sums[:, :, t, 1], red["bg_sum"][:, :, 0])
        np.testing.assert_array_equal(counts[:, t, 0], red["fg_count"][:, 0])
        np.testing.assert_array_equal(counts[:, t, 1], red["bg_count"][:, 0])
    np.testing.assert_array_equal(mg.reduce.counts(xp, "fg").values, fg.sum(axis=(-1, -2)))
    # the moved beads are really elsewhere: the time-0 geometry would miss them
    assert (fg[:, 1:] != fg[:, :1]).any() or (offsets[which][:, 1:] == 0).all()
    # track=None: what the call returns today
    plain = _beads(mg, image)
    np.testing.assert_array_equal(plain.x.values, np.repeat(x[:, :1], N_T, axis=1))
    np.testing.assert_array_equal(plain.y.values, np.repeat(y[:, :1], N_T, axis=1))
    assert "track_score" not in plain.coords and "track_shift_y" not in plain.coords and plain.valid.values.all()
    plain_fg = plain.coords["fg"].data
    assert isinstance(plain_fg, torch.Tensor) and plain_fg.stride(1) == 0  # one geometry, expanded over time
    assert plain.roi.values[:, :, 0].tobytes() == roi[:, :, 0].tobytes() and plain.fg.values[:, 0].tobytes() == fg[:, 0].tobytes()
    assert plain._cache["roi_counts"].shape == (m, 2)


def test_the_second_channel_can_be_the_one_that_is_followed(mg, followed):
    image, drawn, offsets, xp = followed
    other = _beads(mg, image, track="ncc", max_drift=M, track_channel="c1", track_patch=R_HI + 3)
    np.testing.assert_array_equal(other.x.values, xp.x.values)
    np.testing.assert_array_equal(other.y.values, xp.y.values)


def test_a_bead_painted_out_is_not_followed(mg, followed):
    image, drawn, offsets, xp = followed
    which = _match(xp, drawn)
    g = 0
    row, col = (drawn[which[g], :2] + offsets[which[g], 2]).astype(int)
    gone = image.copy()
    rng = np.random.default_rng(8)
    window = (slice(None), 2, slice(row - R_HI - 2, row + R_HI + 3), slice(col - R_HI - 2, col + R_HI + 3))
    gone[window] = np.clip(np.rint(100 + rng.poisson(20.0, size=gone[window].shape) + rng.normal(0, 3.0, size=gone[window].shape)),
                           0, 65535).astype(np.uint16)
    out = _beads(mg, gone, track="ncc", max_drift=M)
    np.testing.assert_array_equal(out.x.values[:, 0], xp.x.values[:, 0])  # the same beads: time 0 is unchanged
    valid = out.valid.values
    assert not valid[g, 2] and valid.sum() == valid.size - 1
    assert out.track_score.values[g, 2] < 0.5
    assert out.x.values[g, 2] == out.x.values[g, 0] and out.y.values[g, 2] == out.y.values[g, 0]
    keep = np.ones(valid.shape, dtype=bool)
    keep[g, 2] = False
    np.testing.assert_array_equal(out.x.values[keep], xp.x.values[keep])
    np.testing.assert_array_equal(out.y.values[keep], xp.y.values[keep])


def test_the_results_survive_save_and_load(mg, followed, tmp_path):
    image, _, offsets, _ = followed
    out = _beads(mg, image, restore=True, track="ncc", max_drift=M)
    mg.save(tmp_path / "followed.nc", out)
    back = mg.load(tmp_path / "followed.nc")
    for name in ("track_shift_y", "track_shift_x", "track_score", "x", "y", "fg", "bg", "valid", "roi"):
        assert back[name].dims == out[name].dims, name
        np.testing.assert_array_equal(back[name].values, out[name].values, err_msg=name)
    assert back["track_shift_y"].values.dtype == np.int32 and back["track_score"].values.dtype == np.float64
    assert back["fg"].values.shape[1] == N_T and (back["fg"].values[:, 1:] != back["fg"].values[:, :1]).any()
    assert back["track_shift_y"].values.any()
