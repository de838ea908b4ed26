"""``find_beads(track="ncc", stage_drift=D)`` on the device against its NumPy restatement (tests/drift_ref.py): the
binned planes of mg_bin_planes, the sums, scores and picks of mg_track_beads_based, the coarse pass and its vote, and
the component end to end on the scenes of tests/test_cpu_drift.py.

Tolerances.  Binned planes: integer pixels bit for bit (a block's sum is below 2^24); fractional float pixels within one
float32 ulp of the float64 NumPy sum (the device sums in float64 in another order -- an error of a few 2^-53 -- and
rounds once: at most half an ulp plus that).  Based tracking: the rules of tests/test_gpu_track.py -- integer-valued
pixels: sums and fixed equal bit for bit; fractional float pixels: |err| <= 4 n 2^-53 |sum| per entry; scores: one ulp of
the restatement's operations on the same sums; shifts: equal wherever the restatement's best two scores differ by more
than 4 ulp (fractional pixels: 1e-6), which the inputs make every (bead, time)."""
import numpy as np
import pytest

import drift_ref as dr
import track_ref as tr
from oracle import ref_numeric as rn
from oracle import ref_pipeline as rp

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "uint16", "float32", "float64"]


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return magnify_amd


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. mg_bin_planes --------------------------------------------------------------------------------------------------

BIN_SHAPES = [(3, 50, 44), (2, 17, 1037)]  # no side a multiple of 8; rows start at odd alignments; vector runs and a tail


def _bin_values(shape, dtype, fractional):
    rng = np.random.default_rng(sum(shape))
    top = 255 if dtype == "uint8" else 65535
    values = rng.integers(0, top + 1, size=shape).astype(np.float64)
    if fractional:
        values = values / 16 + rng.random(shape)
    return values.astype(dtype)


@pytest.mark.parametrize("shape", BIN_SHAPES, ids=["3x50x44", "2x17x1037"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binned_planes_equal_the_restatement(mg, dtype, shape):
    from magnify_amd import track

    for fractional in ((False, True) if dtype.startswith("float") else (False,)):
        planes = _bin_values(shape, dtype, fractional)
        dev = _cuda(planes)
        for b in (2, 4, 8):
            got = track.bin_planes(dev, b)
            assert got.dtype.is_floating_point and got.element_size() == 4
            assert tuple(got.shape) == (shape[0], shape[1] // b, shape[2] // b) and got.is_contiguous()
            first = got.cpu().numpy()
            assert first.tobytes() == track.bin_planes(dev, b).cpu().numpy().tobytes()  # the same bits on every call
            if not fractional:
                assert first.tobytes() == dr.bin_planes(planes, b).tobytes(), (dtype, shape, b)
            else:
                hb, wb = shape[1] // b, shape[2] // b
                want = planes[:, :hb * b, :wb * b].astype(np.float64).reshape(shape[0], hb, b, wb, b).sum(axis=(2, 4))
                err = np.abs(first.astype(np.float64) - want)
                ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                print(dtype, shape, b, "error in float32 ulp, max", float(np.max(err / ulp)))
                assert np.all(err <= ulp), (dtype, shape, b)


def test_the_largest_block_sum_is_exact(mg):
    from magnify_amd import track

    full = np.full((1, 24, 40), 65535, dtype=np.uint16)
    got = track.bin_planes(_cuda(full), 8).cpu().numpy()
    assert got.shape == (1, 3, 5) and (got == 4194240.0).all() and 64 * 65535 == 4194240


def test_binning_reads_strided_planes_where_they_lie(mg):
    from magnify_amd import track

    image = np.random.default_rng(5).integers(0, 65536, size=(2, 3, 50, 44)).astype(np.uint16)
    dev = _cuda(image)
    view = dev[1]
    assert view.data_ptr() != dev.data_ptr() and view.stride(0) == 50 * 44
    every_other = _cuda(image.transpose(1, 0, 2, 3))[:, 1]
    assert every_other.stride(0) == 2 * 50 * 44 and not every_other.is_contiguous()
    for b in (2, 4, 8):
        want = dr.bin_planes(image[1], b)
        for planes in (view, every_other):
            assert track.bin_planes(planes, b).cpu().numpy().tobytes() == want.tobytes(), b


def test_binning_refuses_what_it_cannot_do(mg):
    import torch

    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    planes = _cuda(_bin_values((3, 50, 44), "uint16", False))
    out = torch.full((3, 25, 22), -7.0, dtype=torch.float32, device="cuda")

    def call(dtype=nat.MG_U16, n_t=3, h=50, w=44, b=2, p=planes, o=out):
        return nat.lib().mg_bin_planes(p.data_ptr() if p is not None else 0, dtype, n_t, 50 * 44, h, w, b,
                                       o.data_ptr() if o is not None else 0, hotpath._stream())

    for kw in (dict(b=0), dict(b=1), dict(b=3), dict(b=16), dict(b=-2), dict(b=8, h=7), dict(b=8, w=7), dict(b=4, h=3),
               dict(n_t=0), dict(n_t=-1), dict(dtype=7), dict(dtype=-1), dict(p=None), dict(o=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == -7.0).all()  # nothing was launched
    assert call() == 0 and call(b=8, h=8, w=8, n_t=1) == 0
    torch.cuda.synchronize()
    assert (out.reshape(-1)[1:3 * 25 * 22] != -7.0).all()


# ---- 2. mg_track_beads_based -------------------------------------------------------------------------------------------

SHAPE_T = (96, 80)
SMALL = np.array([(0, 0), (1, -1), (-3, 2)])
BASES = np.array([(0, 0), (5, -4), (-20, 13)])
# interior; near the corner; clipped on two sides; the last pixel; nowhere near the image; overlapping the first; two
# whose patch the bases cut (rows 8 and 90: with by = -20 the rows y + by >= md start at 20 + md, with by = 5 the rows
# y + by < h - md end at 90 - md)
BEADS = np.array([[48, 40, 6], [3, 4, 5], [90, 5, 7], [95, 79, 5], [-40, 30, 6], [50, 43, 8], [8, 40, 6], [90, 70, 6]])
CONFIGS = [(4, 1), (12, 3), (12, 8)]


def _moved_planes(rng, top, shape, moves):
    """T planes of integers in [0, top]: plane t is plane 0 rolled by moves[t], a tenth of the pixels drawn afresh."""
    first = rng.integers(0, top + 1, size=shape)
    planes = []
    for dy, dx in moves:
        p = np.roll(first, (dy, dx), axis=(0, 1))
        fresh = rng.random(shape) < 0.1
        planes.append(np.where(fresh, rng.integers(0, top + 1, size=shape), p))
    return np.stack(planes)


_VALUES, _WANT = {}, {}


def _values(top):
    if top not in _VALUES:
        _VALUES[top] = _moved_planes(np.random.default_rng(1000 + top), top, SHAPE_T, BASES + SMALL)
    return _VALUES[top]


def _want(top, half, m, t_ref):
    """The restatement on the integer planes, made once per (values, configuration) and shared by the dtypes."""
    key = (top, half, m, t_ref)
    if key not in _WANT:
        _WANT[key] = dr.track_based(_values(top).astype(np.uint16), BEADS, half, m, BASES, t_ref)
    return _WANT[key]


def _device(planes, beads, half, m, base, t_ref=0):
    """mg_track_beads_based twice: the same bits; without sums: the same shifts and scores; the results on the host."""
    import torch

    from magnify_amd import track

    dev = planes if isinstance(planes, torch.Tensor) else _cuda(planes)
    first = {k: v.cpu().numpy() for k, v in track.track_beads(dev, beads, half, m, t_ref, want_sums=True, base=base).items()}
    again = track.track_beads(dev, beads, half, m, t_ref, want_sums=True, base=_cuda(np.asarray(base, dtype=np.int32)))
    for k, v in first.items():
        assert v.tobytes() == again[k].cpu().numpy().tobytes(), k
    plain = track.track_beads(dev, beads, half, m, t_ref, base=base)
    assert set(plain) == {"shift", "score"}
    for k in plain:
        assert first[k].tobytes() == plain[k].cpu().numpy().tobytes(), k
    return first


def _compare(got, want, what, t_ref, exact=True, min_gap=None):
    m_beads, n_t = want["score"].shape
    assert got["shift"].shape == (m_beads, n_t, 2) and got["shift"].dtype == np.int32, what
    assert got["score"].shape == (m_beads, n_t) and got["score"].dtype == np.float64, what
    assert got["sums"].shape == want["sums"].shape and got["fixed"].shape == want["fixed"].shape == (m_beads, n_t, 3), what
    if exact:
        np.testing.assert_array_equal(got["sums"], want["sums"].astype(got["sums"].dtype), err_msg=what)
        np.testing.assert_array_equal(got["fixed"], want["fixed"].astype(got["fixed"].dtype), err_msg=what)
    else:
        n = want["fixed"][..., 0]
        np.testing.assert_array_equal(got["fixed"][..., 0], n, err_msg=what)
        for name, count in (("sums", n[:, :, None, None, None]), ("fixed", n[:, :, None])):
            err = np.abs(got[name] - want[name])
            bound = 4 * count * 2.0**-53 * np.abs(want[name])
            print(what, name, "max error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (what, name)
    # scores: the restatement's operations on the restatement's sums -- or, where the sums may differ in the last bits
    # (fractional pixels), on the device's own
    if exact:
        want_score = want["score"]
    else:
        z = np.stack([tr.scores(got["sums"][:, t:t + 1], got["fixed"][:, t])[:, 0] for t in range(n_t)], axis=1)
        want_score = tr.pick(z, t_ref)[1]
    ulp = np.spacing(np.abs(want_score))
    err = np.abs(got["score"] - want_score)
    print(what, "score error in ulp, max", float(np.max(err / ulp)))
    assert np.all(err <= ulp), what
    # shifts: wherever the best score leads (row t_ref: gap = inf); and where every score is 0 (flat or empty patches),
    # which the tie-break decides
    clear = (want["gap"] > (4 * ulp if min_gap is None else min_gap)) | (want["z"] == 0).all(axis=(-1, -2))
    print(what, "pairs compared", int(clear.sum()), "of", clear.size)
    assert clear.all(), what  # every pair is compared: the inputs leave none out
    np.testing.assert_array_equal(got["shift"][clear], want["shift"][clear], err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_all_zero_base_is_the_plain_search(mg, dtype):
    from magnify_amd import track

    top = 255 if dtype == "uint8" else 4000
    dev = _cuda(_values(top).astype(dtype))
    for half, m in CONFIGS:
        for t_ref in (0, 2):
            plain = {k: v.cpu().numpy() for k, v in track.track_beads(dev, BEADS, half, m, t_ref, want_sums=True).items()}
            got = _device(dev, BEADS, half, m, np.zeros((3, 2), dtype=np.int32), t_ref)
            for k in ("shift", "score", "sums"):
                assert got[k].tobytes() == plain[k].tobytes(), (k, half, m, t_ref)
            assert got["fixed"].shape == (len(BEADS), 3, 3) and got["fixed"].dtype == plain["fixed"].dtype
            for t in range(3):
                assert got["fixed"][:, t].tobytes() == plain["fixed"].tobytes(), (half, m, t_ref, t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_based_sums_scores_and_picks_equal_the_restatement(mg, dtype):
    top = 255 if dtype == "uint8" else 4000
    planes = _values(top).astype(dtype)
    for half, m in CONFIGS:
        for t_ref in (0, 2):
            got = _device(planes, BEADS, half, m, BASES, t_ref)
            want = _want(top, half, m, t_ref)
            integer = np.dtype(dtype).kind == "u"
            assert got["sums"].dtype == got["fixed"].dtype == (np.int64 if integer else np.float64)
            _compare(got, want, f"{dtype} half={half} m={m} t_ref={t_ref}", t_ref)
            if t_ref == 0:
                # what the scene is: the interior bead follows base + small move, as a total
                within = (np.abs(SMALL) <= m).all(axis=1)
                np.testing.assert_array_equal(got["shift"][0][within], (BASES + SMALL)[within])
            # the bead outside the image: empty at every timepoint
            assert not got["fixed"][4].any() and not got["sums"][4].any() and not got["shift"][4].any()
            assert got["score"][4].tolist() == [1.0 if t == t_ref else 0.0 for t in range(3)]
    # the base cuts the patch of the beads near the border differently at every timepoint
    n = _device(planes, BEADS, 12, 3, BASES)["fixed"][..., 0]
    assert len(set(n[6].tolist())) > 1 and len(set(n[7].tolist())) > 1 and len(set(n[0].tolist())) == 1


def test_a_base_far_outside_the_image_gives_an_empty_patch(mg):
    planes = _values(4000).astype(np.uint16)
    h, w = SHAPE_T
    base = np.array([(0, 0), (h + 50, 0), (-3 * w, 7)])
    got = _device(planes, BEADS, 12, 3, base)
    assert not got["shift"][:, 1:].any() and not got["score"][:, 1:].any()
    assert not got["sums"][:, 1:].any() and not got["fixed"][:, 1:].any()
    assert (got["score"][:, 0] == 1.0).all() and got["fixed"][0, 0, 0] == 25 * 25
    want = dr.track_based(planes, BEADS, 12, 3, base)
    assert want["empty"][:, 1:].all()
    np.testing.assert_array_equal(got["shift"], want["shift"])
    far = np.array([(0, 0), (2**31 - 1, -2**31), (-2**31, 2**31 - 1)])  # the geometry is made in 64 bits
    got = _device(planes, BEADS, 12, 3, far)
    assert not got["shift"].any() and not got["score"][:, 1:].any() and not got["fixed"][:, 1:].any()


def test_the_largest_patch_and_window_around_a_base(mg):
    """half = 47, md = 16 on 200 x 200 uint16 with values up to 65535 and base (10, -12): 95^2 template, 127^2 window,
    1089 displacements."""
    rng = np.random.default_rng(65535)
    planes = _moved_planes(rng, 65535, (200, 200), ((0, 0), (15, -19), (9, -12))).astype(np.uint16)
    bead = np.array([[100, 100, 40]])
    base = np.array([(0, 0), (10, -12), (10, -12)])
    for t_ref in (0, 2):
        got = _device(planes, bead, 47, 16, base, t_ref)
        want = dr.track_based(planes, bead, 47, 16, base, t_ref)
        _compare(got, want, f"largest t_ref={t_ref}", t_ref)
        assert got["fixed"][0, :, 0].tolist() == [9025] * 3
    first = _device(planes, bead, 47, 16, base, 0)
    assert first["shift"][0].tolist() == [[0, 0], [15, -19], [9, -12]]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_based_tracking_of_fractional_float_pixels(mg, dtype):
    rng = np.random.default_rng(3)
    planes = (_moved_planes(rng, 4000, SHAPE_T, BASES + SMALL) + rng.random((3,) + SHAPE_T)).astype(dtype)  # non-negative
    for half, m in ((12, 3), (12, 8)):
        got = _device(planes, BEADS, half, m, BASES)
        want = dr.track_based(planes, BEADS, half, m, BASES)
        _compare(got, want, f"fractional {dtype} half={half} m={m}", 0, exact=False, min_gap=1e-6)


def test_the_based_entry_refuses_what_it_cannot_do(mg):
    import torch

    from magnify_amd import _native as nat
    from magnify_amd import hotpath, track

    planes = _cuda(_values(4000).astype(np.uint16))
    beads = _cuda(BEADS.astype(np.int32))
    base = _cuda(BASES.astype(np.int32))
    n_b = len(BEADS)
    shift = torch.full((n_b, 3, 2), 99, dtype=torch.int32, device="cuda")
    score = torch.full((n_b, 3), -5.0, dtype=torch.float64, device="cuda")

    def call(dtype=nat.MG_U16, n_t=3, h=96, w=80, t_ref=0, m=n_b, half=12, md=3, p=planes, b=beads, bs=base, sh=shift, sc=score):
        ptr = lambda x: x.data_ptr() if x is not None else 0  # noqa: E731
        return nat.lib().mg_track_beads_based(ptr(p), dtype, n_t, 96 * 80, h, w, t_ref, ptr(b), m, half, md, ptr(bs), ptr(sh),
                                              ptr(sc), 0, 0, hotpath._stream())

    bad = [dict(md=0), dict(md=17), dict(half=0), dict(half=48), dict(half=47, md=17), dict(half=48, md=16), dict(t_ref=-1),
           dict(t_ref=3), dict(n_t=0), dict(h=0), dict(w=0), dict(m=-1), dict(dtype=7), dict(p=None), dict(b=None),
           dict(sh=None), dict(sc=None), dict(bs=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (shift == 99).all() and (score == -5.0).all()  # nothing was launched
    assert call(m=0) == 0
    torch.cuda.synchronize()
    assert (shift == 99).all() and (score == -5.0).all()
    assert call(half=47, md=16) == 0 and call(t_ref=2) == 0
    torch.cuda.synchronize()
    assert (score[:, 2] == 1.0).all()
    with pytest.raises(ValueError):
        track.track_beads(planes, BEADS, 12, 3, base=np.zeros((2, 2), dtype=np.int32))  # a base per timepoint


# ---- 3. the coarse pass and its vote -----------------------------------------------------------------------------------

_SCENES = {}


def _scene(index, seed, channels=None, n=dr.N_BEADS):
    key = (index, seed, channels, n)
    if key not in _SCENES:
        shape, drifts, border, D = dr.SCENES[index]
        image, beads, offsets = dr.scene(seed, shape, n, dr.R_LO, dr.R_HI, dr.JITTER, drifts, D=border, channels=channels)
        _SCENES[key] = (image, beads, offsets, D)
    return _SCENES[key]


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("index", range(len(dr.SCENES)), ids=["384x352", "288x320"])
def test_the_stage_offset_equals_the_restatement(mg, index, seed):
    from magnify_amd import track

    planes, beads, offsets, D = _scene(index, seed)
    want = dr.stage_drift(planes, D, 0.5)
    got = track.stage_drift(_cuda(planes), D, 0.5)
    assert got["shift"].dtype == np.int32 and got["agree"].dtype == np.float64 and got["bin"] == want["bin"]
    np.testing.assert_array_equal(got["anchors"], want["anchors"])
    np.testing.assert_array_equal(got["picks"], want["picks"])
    np.testing.assert_array_equal(got["shift"], want["shift"])
    np.testing.assert_array_equal(got["agree"], want["agree"])
    ulp = np.spacing(np.abs(want["scores"]))
    assert np.all(np.abs(got["scores"] - want["scores"]) <= ulp)
    # and the beads are then followed to where they were drawn
    res = track.track_beads(_cuda(planes), beads, dr.HALF, dr.MAX_DRIFT, base=got["shift"])
    np.testing.assert_array_equal(res["shift"].cpu().numpy(), offsets)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------

# The (384, 352) scene with six beads, seed 2.  Without stage_drift every bead of a timepoint that drifted beyond
# max_drift has to come out as not followed, so the scene is one where the plain search sees nothing but background
# there: no disk -- another bead's or the bead's own, moved -- may reach the window the search reads,
# max_drift + half pixels about the time-0 centre.  _far_from_every_window states that in the drawn geometry; with
# twelve beads on this image and drifts of 40 a moved bead always lands in some other bead's window (and where it
# lands within max_drift of its centre, the plain search follows the wrong bead with a score of 1).
N_T, E2E_BEADS, E2E_SEED = 4, 6, 2


def _far_from_every_window(drawn, offsets, far):
    pos = drawn[:, :2]
    for t in np.flatnonzero(far):
        apart = np.abs((pos + offsets[:, t])[:, None] - pos[None]).max(axis=2)  # Chebyshev, a bead's own move included
        if apart.min() <= dr.MAX_DRIFT + dr.HALF + dr.R_HI:
            return False
    return True
KW = dict(min_bead_diameter=2 * dr.R_LO, max_bead_diameter=2 * dr.R_HI, overlap=0, num_iter=60000, search_channel="c0")
DRIFT_KW = dict(track="ncc", stage_drift=40, max_drift=dr.MAX_DRIFT)


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
    image, drawn, offsets, D = _scene(0, E2E_SEED, channels=2, n=E2E_BEADS)
    assert image.shape == (2, N_T, 384, 352) and D == 40 and len(drawn) == E2E_BEADS
    return image, drawn, offsets, _beads(mg, image, **DRIFT_KW)


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


def test_a_drifted_stage_end_to_end(mg, followed):
    image, drawn, offsets, xp = followed
    which = _match(xp, drawn)
    x, y = xp.x.values, xp.y.values
    np.testing.assert_array_equal(y - y[:, :1], offsets[which][..., 0])
    np.testing.assert_array_equal(x - x[:, :1], offsets[which][..., 1])
    np.testing.assert_array_equal(xp.track_shift_y.values, offsets[which][..., 0])
    np.testing.assert_array_equal(xp.track_shift_x.values, offsets[which][..., 1])
    assert xp.track_shift_y.values.dtype == np.int32 and xp.track_score.values.dtype == np.float64
    assert xp.valid.values.all()
    stage = dr.stage_drift(image[0], 40, 0.5)
    assert xp.stage_shift_y.dims == xp.stage_shift_x.dims == xp.stage_agree.dims == ("time",)
    assert xp.stage_shift_y.values.dtype == xp.stage_shift_x.values.dtype == np.int32 and xp.stage_agree.values.dtype == np.float64
    np.testing.assert_array_equal(xp.stage_shift_y.values, stage["shift"][:, 0])
    np.testing.assert_array_equal(xp.stage_shift_x.values, stage["shift"][:, 1])
    np.testing.assert_array_equal(xp.stage_agree.values, stage["agree"])
    assert np.abs(stage["shift"]).max() > dr.MAX_DRIFT  # the stage did move beyond the per-bead search
    assert xp.fg.dims == ("mark", "time", "roi_y", "roi_x") and xp.roi.dims == ("mark", "channel", "time", "roi_y", "roi_x")
    m, L = len(which), 2 * 2 * dr.R_HI
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


def test_without_stage_drift_the_drifted_timepoints_are_lost(mg, followed):
    image, drawn, offsets, xp = followed
    plain = _beads(mg, image, track="ncc", max_drift=dr.MAX_DRIFT)
    for name in ("stage_shift_y", "stage_shift_x", "stage_agree"):
        assert name not in plain.coords, name
    np.testing.assert_array_equal(plain.x.values[:, 0], xp.x.values[:, 0])  # the same beads
    drifts = np.asarray(dr.SCENES[0][1])
    far = np.abs(drifts).max(axis=1) > dr.MAX_DRIFT
    assert far.tolist() == [False, True, True, False] and _far_from_every_window(drawn, offsets, far)
    valid = plain.valid.values
    assert not valid[:, far].any() and valid[:, ~far].all()
    np.testing.assert_array_equal(plain.x.values[:, ~far], xp.x.values[:, ~far])
    np.testing.assert_array_equal(plain.y.values[:, ~far], xp.y.values[:, ~far])


def test_a_timepoint_of_noise_falls_back_and_is_not_followed(mg, followed):
    image, drawn, offsets, xp = followed
    rng = np.random.default_rng(8)
    gone = image.copy()
    shape = gone[:, 2].shape
    gone[:, 2] = np.clip(np.rint(100 + rng.poisson(20.0, size=shape) + rng.normal(0, 3.0, size=shape)), 0, 65535).astype(np.uint16)
    out = _beads(mg, gone, **DRIFT_KW)
    stage = dr.stage_drift(gone[0], 40, 0.5)
    voters = (stage["scores"][:, 2] >= 0.5).sum()
    n_agree = stage["agree"][2] * len(stage["anchors"])
    assert 2 * n_agree < max(voters, 1)  # below half the voters: not trusted
    np.testing.assert_array_equal(out.stage_agree.values, stage["agree"])
    assert out.stage_agree.values[2] < 0.5
    assert out.stage_shift_y.values[2] == 0 and out.stage_shift_x.values[2] == 0
    valid = out.valid.values
    assert not valid[:, 2].any()
    keep = [0, 1, 3]
    assert valid[:, keep].all()
    for name in ("x", "y", "track_shift_y", "track_shift_x"):
        np.testing.assert_array_equal(out[name].values[:, keep], xp[name].values[:, keep], err_msg=name)
    for name in ("stage_shift_y", "stage_shift_x", "stage_agree"):
        np.testing.assert_array_equal(out[name].values[keep], xp[name].values[keep], err_msg=name)
    np.testing.assert_array_equal(out.x.values[:, 2], out.x.values[:, 0])  # the time-0 window, as under track="ncc" today
    np.testing.assert_array_equal(out.y.values[:, 2], out.y.values[:, 0])


def test_the_stage_coordinates_survive_save_and_load(mg, followed, tmp_path):
    image, _, offsets, xp = followed
    out = _beads(mg, image, restore=True, **DRIFT_KW)
    mg.save(tmp_path / "drifted.nc", out)
    back = mg.load(tmp_path / "drifted.nc")
    for name in ("stage_shift_y", "stage_shift_x", "stage_agree", "track_shift_y", "track_shift_x", "track_score", "x", "y",
                 "valid"):
        assert back[name].dims == out[name].dims, name
        np.testing.assert_array_equal(back[name].values, out[name].values, err_msg=name)
    assert out["stage_shift_y"].dims == ("time",)
    assert back["stage_shift_y"].values.dtype == np.int32 and back["stage_shift_x"].values.dtype == np.int32
    assert back["stage_agree"].values.dtype == np.float64
    np.testing.assert_array_equal(back["stage_shift_y"].values, xp.stage_shift_y.values)
    assert np.abs(back["stage_shift_y"].values).max() > dr.MAX_DRIFT
