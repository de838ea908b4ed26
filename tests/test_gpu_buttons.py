"""The chip path's oldest device code on the GPU: mg_cluster1d_costs against the exact costs of tests/buttons_ref.py
within the derived rounding bound -- at 1 .. 130 and 4096 clusters, points on boundaries, no points, offsets without any
point, a crowded cluster, exact ties --, mg_button_masks byte for byte against the vectorised cv.circle oracle at every
window length, radius, centre and annulus that matters, the refusals of both entry points, and ``ButtonFinder.refine`` /
``ButtonFinder.__call__`` against ``oracle.ref_pipeline.find_rois`` with all of its outputs: windows shifted into the image,
estimates at x.5, a blank chamber, no search at all, competing search channels, a float32 image."""
import numpy as np
import pytest

import buttons_ref as ref
from oracle import ref_pipeline as rp
from synth import draw_chip

pytestmark = pytest.mark.gpu

WORST = {"cost": 0.0, "same_bits": 0, "costs": 0}  # largest error / bound; costs bit-equal to the sequential restatement


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


@pytest.fixture(scope="module")
def mg(hp):
    import magnify_amd

    return magnify_amd


# ---- cluster costs -------------------------------------------------------------------------------------------------------

SENTINEL = -7.0


def device_costs(hp, points, n_offsets, n_clusters, cluster_length, ideal, penalty, expect=0):
    """mg_cluster1d_costs as ``hotpath.cluster_1d`` calls it, into a buffer filled with SENTINEL."""
    import torch

    from magnify_amd import _native as nat

    pts = np.sort(np.asarray(points, dtype=np.float64))
    d_pts = torch.from_numpy(pts).cuda() if len(pts) else torch.zeros(1, dtype=torch.float64, device="cuda")
    d_ideal = torch.from_numpy(np.asarray(ideal, dtype=np.float64)).cuda()
    costs = torch.full((n_offsets,), SENTINEL, dtype=torch.float64, device="cuda")
    rc = nat.lib().mg_cluster1d_costs(d_pts.data_ptr(), len(pts), n_offsets, n_clusters, float(cluster_length),
                                      d_ideal.data_ptr(), float(penalty), costs.data_ptr(), hp._stream())
    torch.cuda.synchronize()
    assert rc == expect
    return costs.cpu().numpy()


def sequential_costs(points, n_offsets, n_clusters, cluster_length, ideal, penalty):
    """The kernel's order of operations in NumPy float64 scalars: each cluster's squares added one by one, the terms of
    the clusters added in order."""
    pts = np.sort(np.asarray(points, dtype=np.float64))
    ideal = np.asarray(ideal, dtype=np.float64)
    out = np.empty(n_offsets, dtype=np.float64)
    for off in range(n_offsets):
        bounds, centres = ref.boundaries(n_clusters, cluster_length, off)
        spans = np.searchsorted(pts, bounds, side="left")
        var = np.zeros(n_clusters)
        for k in range(n_clusters):
            s = np.float64(0.0)
            for p in pts[spans[k]: spans[k + 1]]:
                s = s + (p - centres[k]) * (p - centres[k])
            if spans[k + 1] > spans[k]:
                var[k] = s / np.float64(spans[k + 1] - spans[k])
        count = np.diff(spans)
        var[count == 0] = var.max()
        total = np.float64(0.0)
        for k in range(n_clusters):
            miss = ideal[k] - np.float64(count[k])
            total = total + (var[k] * np.sqrt(ideal[k]) + np.float64(penalty) * miss * miss)
        out[off] = total
    return out


def hold_costs(have, s, what):
    ratio = ref.error_ratio(have, s["exact"], s["bound"])
    WORST["cost"] = max(WORST["cost"], ratio)
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("n_clusters", ref.CLUSTERS)
@pytest.mark.parametrize("cluster_length", ref.LENGTHS)
def test_costs_match_exact_oracle(hp, n_clusters, cluster_length):
    """Every cost of every offset within ``cost_bound`` of the exact one; the same bits on a second call; where no cluster
    holds a point, exactly penalty * sum(ideal**2)."""
    for n_offsets in ref.OFFSETS:
        for penalty in ref.PENALTIES:
            for s in ref.point_sets(n_clusters, cluster_length, n_offsets, penalty):
                what = (s["name"], n_clusters, cluster_length, n_offsets, penalty)
                have = device_costs(hp, s["points"], n_offsets, n_clusters, cluster_length, s["ideal"], penalty)
                hold_costs(have, s, what)
                again = device_costs(hp, s["points"], n_offsets, n_clusters, cluster_length, s["ideal"], penalty)
                assert have.tobytes() == again.tobytes(), what
                if s["name"] in ("left", "right", "none"):
                    assert (have == float(penalty * int((s["ideal"] ** 2).sum()))).all(), what
                if s["name"] != "long" and n_clusters <= 65:  # (the restatement is a Python loop)
                    same = have == sequential_costs(s["points"], n_offsets, n_clusters, cluster_length, s["ideal"], penalty)
                    WORST["same_bits"] += int(same.sum())
                    WORST["costs"] += n_offsets


@pytest.mark.parametrize("n_clusters", ref.CLUSTERS)
def test_cluster_1d_labels_equal_the_reference(hp, n_clusters):
    """``hotpath.cluster_1d`` on every separated set (tests/test_cpu_buttons.py holds them to the condition), points in
    the order they were drawn."""
    for cluster_length in ref.LENGTHS:
        for n_offsets in ref.OFFSETS:
            for penalty in ref.PENALTIES:
                total = n_offsets + round(n_clusters * cluster_length)
                for s in ref.point_sets(n_clusters, cluster_length, n_offsets, penalty):
                    if s["separated"] or s["name"] in ("left", "right", "boundaries"):
                        have = hp.cluster_1d(s["points"], total, n_clusters, cluster_length, s["ideal"], penalty)
                        want = rp.cluster_1d(s["points"], total, n_clusters, cluster_length, s["ideal"], penalty)
                        np.testing.assert_array_equal(have, want, str((s["name"], cluster_length, n_offsets, penalty)))
                    if s["name"] in ("left", "right"):  # every offset costs the same: the first one wins
                        assert (have == -1).all()


def test_points_on_boundaries_belong_to_the_cluster_that_starts_there(hp):
    """Every boundary of one offset as a point, the first one four times: at that offset cluster 0 holds those four, every
    other cluster its own left boundary, and the last boundary is outside -- var (L / 2)**2 everywhere, nothing missing."""
    ideal = np.array([4, 1, 1, 1, 1])
    for length in ref.LENGTHS:
        for offset in (0, 3):
            bounds = ref.boundaries(5, length, offset)[0]
            points = np.concatenate([bounds, bounds[:1].repeat(3)])
            have = device_costs(hp, points, offset + 1, 5, length, ideal, 50)
            _, exact = ref.cluster_costs_exact(points, offset + 1, 5, length, ideal, 50)
            assert ref.error_ratio(have, exact, ref.cost_bound(points, offset + 1, 5, length)) <= 1.0
            if length != 33.3:  # (33.3 * k is rounded; the other lengths are exact and so is every operation on them)
                assert exact[offset] == (2 + 4) * ref.Fraction(length / 2) ** 2 and have[offset] == float(exact[offset])
            labels = hp.cluster_1d(points, offset + 1 + round(5 * length), 5, length, ideal, 50)
            np.testing.assert_array_equal(labels, ref.labels_of(points, 5, length, int(np.argmin(have))))
            if offset == 0:
                np.testing.assert_array_equal(labels, [0, 1, 2, 3, 4, -1, 0, 0, 0])


@pytest.mark.parametrize("case", ref.TIES)
def test_hand_made_ties(hp, case):
    """Two offsets whose costs are bit-equal in the reference: bit-equal here, and the first one wins."""
    points, total, k, length, ideal, penalty, (a, b) = case
    n_off = ref.tie_offsets(total, k, length)
    have = device_costs(hp, points, n_off, k, length, ideal, penalty)
    _, exact = ref.cluster_costs_exact(points, n_off, k, length, ideal, penalty)
    hold_costs(have, dict(exact=exact, bound=ref.cost_bound(points, n_off, k, length)), case)
    assert have[a] == have[b] == have.min() and int(np.argmin(have)) == a
    np.testing.assert_array_equal(hp.cluster_1d(points, total, k, length, ideal, penalty),
                                  rp.cluster_1d(points, total, k, length, ideal, penalty))
    np.testing.assert_array_equal(hp.cluster_1d(points, total, k, length, ideal, penalty), ref.labels_of(points, k, length, a))


def test_cluster_limit(hp):
    """4096 clusters (the most that fit the staging in LDS) are accepted and correct; 4097 are refused and nothing is
    written; ``hotpath.cluster_1d`` raises when the clusters do not fit into the total length."""
    rng = np.random.default_rng(4096)
    k, length, n_off = 4096, 2.5, 3
    points = np.concatenate([rng.uniform(0, k * length + n_off, 2 * k), rng.integers(0, int(k * length), k)])
    ideal = rng.integers(0, 6, k)
    have = device_costs(hp, points, n_off, k, length, ideal, 50)
    _, exact = ref.cluster_costs_exact(points, n_off, k, length, ideal, 50)
    bound = ref.cost_bound(points, n_off, k, length)
    hold_costs(have, dict(exact=exact, bound=bound), "4096 clusters")
    assert ref.separation(exact, bound)
    total = n_off + round(k * length)
    np.testing.assert_array_equal(hp.cluster_1d(points, total, k, length, ideal, 50),
                                  rp.cluster_1d(points, total, k, length, ideal, 50))
    more = np.append(ideal, 1)
    assert (device_costs(hp, points, n_off, k + 1, length, more, 50, expect=-1) == SENTINEL).all()
    assert (device_costs(hp, points, n_off, 0, length, ideal, 50, expect=-1) == SENTINEL).all()
    with pytest.raises(ValueError):
        hp.cluster_1d(points, total, k + 1, length, more, 50)
    for too_short in (20, 19, 3):
        with pytest.raises(ValueError, match="do not fit"):
            hp.cluster_1d([1.0, 2.0], too_short, 2, 10.0, [1, 1], 50)
    np.testing.assert_array_equal(hp.cluster_1d([1.0, 12.0, 21.0], 21, 2, 10.0, [1, 1], 50), [0, 1, -1])  # one offset


def test_worst_cost_error_is_reported(hp):
    """Last of the cost tests: the figures of the whole sweep."""
    print(f"\ncluster costs, worst |error| / bound over the sweep: {WORST['cost']:.3e}; "
          f"{WORST['same_bits']} of {WORST['costs']} costs bit-equal to the sequential float64 restatement")
    assert WORST["cost"] <= 1.0


# ---- button masks -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("L", ref.MASK_LENGTHS)
@pytest.mark.parametrize("inner_r,outer_r", ref.MASK_PAIRS)
def test_masks_equal_the_oracle_byte_for_byte(hp, L, inner_r, outer_r):
    batches = ref.mask_batches(L, outer_r) + [(np.array([[L // 2, L - 1]]), np.array([15]))]  # m = 300 twice, m = 1
    for centers, radii in batches:
        fg, bg = hp.button_masks(centers, radii, L, outer_r, inner_r)
        want_fg, want_bg = ref.button_masks_ref(centers, radii, L, outer_r, inner_r)
        have_fg, have_bg = fg.cpu().numpy(), bg.cpu().numpy()
        assert have_fg.dtype == np.uint8 and have_fg.shape == (len(radii), L, L) == have_bg.shape
        assert have_fg.tobytes() == want_fg.tobytes(), np.argwhere((have_fg != want_fg).any(axis=(1, 2))).ravel()[:5]
        assert have_bg.tobytes() == want_bg.tobytes(), np.argwhere((have_bg != want_bg).any(axis=(1, 2))).ravel()[:5]
        assert have_fg.max(initial=0) <= 1 and have_bg.max(initial=0) <= 1  # viewed as bool later
    fg, bg = hp.button_masks(np.zeros((0, 2)), [], L, outer_r, inner_r)
    assert fg.shape == bg.shape == (0, L, L) and fg.dtype == bg.dtype


def test_mask_refusals_write_nothing(hp):
    import torch

    from magnify_amd import _native as nat

    m, L, top = 3, 9, 30
    tab = hp._cv_table(top, "cuda")
    assert tab.shape == (top + 1, top + 1)
    centers = torch.tensor([[4, 4], [0, 8], [-3, 20]], dtype=torch.int32, device="cuda")
    radii = torch.tensor([2, 5, 30], dtype=torch.int32, device="cuda")
    fg = torch.full((m, L, L), 7, dtype=torch.uint8, device="cuda")
    bg = torch.full((m, L, L), 7, dtype=torch.uint8, device="cuda")

    def call(c=centers.data_ptr(), r=radii.data_ptr(), n=m, length=L, outer=30, inner=15, t=tab.data_ptr(), stride=top + 1,
             max_r=top, f=fg.data_ptr(), b=bg.data_ptr()):
        rc = nat.lib().mg_button_masks(c, r, n, length, outer, inner, t, stride, max_r, f, b, hp._stream())
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((fg == 7).all()) and bool((bg == 7).all())  # noqa: E731
    for kw in [dict(outer=top + 1), dict(inner=top + 1), dict(outer=-1), dict(inner=-1), dict(stride=top), dict(stride=0),
               dict(max_r=29, outer=30), dict(length=0), dict(length=-9), dict(n=-1), dict(c=None), dict(r=None),
               dict(t=None), dict(f=None), dict(b=None)]:
        assert call(**kw) == -1 and untouched(), kw
    assert call(n=0) == 0 and untouched()
    assert call() == 0
    want_fg, want_bg = ref.button_masks_ref(centers.cpu().numpy(), radii.cpu().numpy(), L, 30, 15)
    assert fg.cpu().numpy().tobytes() == want_fg.tobytes() and bg.cpu().numpy().tobytes() == want_bg.tobytes()


# ---- stages -----------------------------------------------------------------------------------------------------------------

# 2 x 3 buttons 30 px from every border of a 160 x 260 image, windows of 72: those of the border chambers do not fit about
# their centres and are shifted into the image; the middle column's fit
CHIP = dict(row_dist=100, col_dist=100, min_button_diameter=16, max_button_diameter=32, chamber_diameter=60, roi_length=72)
MIN_R, MAX_R, CHAMBER_R, LENGTH = 8, 16, 30, 72
SHAPE = (2, 3)


def border_chip(diameter=20, offset=(0, 0)):
    return draw_chip(SHAPE, diameter, offset=offset)[70:230, 70:330].copy()


def tags(*blanks):
    tag = np.full(SHAPE, "default", dtype="<U200")
    for where in blanks:
        tag[where] = ""
    return tag


# estimates at x.5 on both sides of the even 30 and 130 (round-half-to-even: 29.5 and 30.5 -> 30, 129.5 and 130.5 -> 130)
EST_Y = np.array([[29.5, 30.5, 31.5], [130.5, 128.5, 131.0]])
EST_X = np.array([[30.5, 130.5, 229.5], [28.5, 129.5, 232.0]])


def _set_tags(xp, tag):
    return xp.assign_coords(tag=(("mark_row", "mark_col"), tag))


def run_both(mg, monkeypatch, planes, tag, num_iter, search=None, est=(EST_X, EST_Y), seed=2024):
    """``planes`` (C, H, W) through the chip pipeline with ``find_centers`` replaced by the hand-made estimates, through
    ``ButtonFinder.refine`` on its own, and through the oracle's ``find_rois`` with the seed that ``__call__`` draws."""
    import torch

    from magnify_amd import utils
    from magnify_amd.find import ButtonFinder

    gx, gy = est
    names = [f"c{k}" for k in range(len(planes))]
    search = names if search is None else search
    search_idx = [names.index(c) for c in search]
    monkeypatch.setattr(ButtonFinder, "find_centers", lambda self, p, t, seeds: (gx.copy(), gy.copy()))
    mg.seed(seed)
    drawn = [utils.next_seed() for _ in range(len(search) + 1)]  # one per search channel, then the one of refine
    mg.seed(seed)
    pipe = mg.microfluidic_chip_pipe(shape=SHAPE, overlap=0, num_iter=num_iter, search_channel=search, **CHIP)
    pipe.add_pipe(_set_tags, name="set_tags", after="identify_buttons", tag=tag)
    xp = pipe(mg.DataArray(data=planes, dims=("channel", "y", "x"), coords={"channel": names}))
    mg.seed(None)
    xp = xp.unstack().transpose("mark_row", "mark_col", ...)
    bf = ButtonFinder(top_chamber=None, left_chamber=None, low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=num_iter,
                      min_roundness=0.2, cluster_penalty=50, progress_bar=False, search_timestep=0, search_channel=search,
                      interactive=False, **CHIP)
    assert (bf.min_button_radius, bf.max_button_radius, bf.chamber_radius, bf.roi_length) == (MIN_R, MAX_R, CHAMBER_R, LENGTH)
    x, y, radius = bf.refine(torch.from_numpy(planes).cuda(), gx, gy, tag, search_idx, drawn[-1])
    want = rp.find_rois(planes, gx, gy, tag, search_idx, MIN_R, MAX_R, CHAMBER_R, LENGTH, 0.1, num_iter, 0.2, seed=drawn[-1])
    return xp, (x, y, radius), want


def hold_to_oracle(xp, refined, want, n_c):
    roi_o, fg_o, bg_o, x_o, y_o = want
    x, y, radius = refined
    np.testing.assert_array_equal(x, x_o)
    np.testing.assert_array_equal(y, y_o)
    np.testing.assert_array_equal(np.asarray(xp.x.values).reshape(SHAPE), x_o)
    np.testing.assert_array_equal(np.asarray(xp.y.values).reshape(SHAPE), y_o)
    fg, bg, roi = np.asarray(xp.fg.values), np.asarray(xp.bg.values), np.asarray(xp.roi.values)
    assert fg.dtype == bool and bg.dtype == bool and roi.dtype == roi_o.dtype
    if n_c > 1:
        assert xp.roi.dims == ("mark_row", "mark_col", "channel", "roi_y", "roi_x")
    np.testing.assert_array_equal(fg.reshape(fg_o.shape), fg_o)
    np.testing.assert_array_equal(bg.reshape(bg_o.shape), bg_o)
    np.testing.assert_array_equal(roi.reshape(roi_o.shape), roi_o)
    # the oracle's fg is cv.circle's disk of the refined radius about the refined centre: the radii are the oracle's too
    rel = np.stack([np.rint(y_o).astype(int) - ref_origin(y_o, roi_o.shape[-1], 160),
                    np.rint(x_o).astype(int) - ref_origin(x_o, roi_o.shape[-1], 260)], axis=-1).reshape(-1, 2)
    np.testing.assert_array_equal(ref.button_masks_ref(rel, radius.reshape(-1), LENGTH, CHAMBER_R, MAX_R)[0].astype(bool),
                                  fg_o.reshape(-1, LENGTH, LENGTH))


def ref_origin(c, L, size):
    """First row / column of the reference's window about round(c) (``oracle.ref_numeric.bounding_box``)."""
    from oracle import ref_numeric as rn

    return np.array([rn.bounding_box(int(round(v)), int(round(v)), L, size, size)[0] for v in np.asarray(c).reshape(-1)]).reshape(np.shape(c))


def test_refine_on_shifted_windows_and_half_estimates(mg, monkeypatch):
    """x, y, radii, fg, bg and the gathered roi of a chip whose border windows are shifted into the image, from grid
    estimates at x.5; one chamber is blank: it keeps its estimate (at x.5, in an unshifted column: its final window hangs
    on the rounding) and ``max_button_radius``."""
    img = border_chip()
    img[img > 0] += 37
    tag = tags((0, 1))
    xp, refined, want = run_both(mg, monkeypatch, img[None], tag, 6000)
    hold_to_oracle(xp, refined, want, 1)
    x, y, radius = refined
    assert x[0, 1] == 130.5 and y[0, 1] == 30.5 and radius[0, 1] == MAX_R
    found = tag != ""
    assert (np.abs(x - [[30, 130, 230]] * 2)[found] <= 1).all() and (np.abs(y - [[30] * 3, [130] * 3])[found] <= 1).all()
    assert (radius[found] >= 9).all() and (radius[found] <= 11).all()
    centre = np.asarray(xp.fg.values).reshape(SHAPE + (LENGTH, LENGTH))
    assert centre[0, 0, 22, 30] and not centre[0, 0, 44, 36]  # window (0, 0) starts at the image's corner, not 6 px outside
    assert centre[1, 2, 72 - 30, 72 - 30] and centre[1, 1, 72 - 30, 36]


def test_no_search_when_num_iter_is_below_the_chamber_count(mg, monkeypatch):
    """5 iterations for 6 chambers: none per chamber.  The oracle accepts that (no picks, no circles): positions stay the
    estimates and every radius is ``max_button_radius``."""
    img = border_chip()
    xp, refined, want = run_both(mg, monkeypatch, img[None], tags(), 5)
    hold_to_oracle(xp, refined, want, 1)
    x, y, radius = refined
    np.testing.assert_array_equal(x, EST_X)
    np.testing.assert_array_equal(y, EST_Y)
    assert (radius == MAX_R).all()


def competing_channels():
    """Channel 0: buttons of 20 px, speckled away in the right column.  Channel 1: buttons of 24 px, 3 px lower and 2 px to
    the left, at a third of the brightness, speckled in the left column.  Channel 2: channel 0 one pixel to the right."""
    rng = np.random.default_rng(5)
    a, b = border_chip(), border_chip(24, offset=(3, -2))
    a[:, 180:][rng.random(a[:, 180:].shape) < 0.35] = 0
    b[:, :80][rng.random(b[:, :80].shape) < 0.35] = 0
    return np.stack([a, b // 3, np.roll(a, 1, axis=1)])


@pytest.mark.parametrize("search", [["c0", "c1"], ["c1", "c0"], ["c0", "c1", "c2"], ["c2", "c0"]])
def test_search_channels_compete_by_score(mg, monkeypatch, search):
    """Every chamber takes the circle of the best score over the search channels, the earlier channel on a tie: the
    oracle's pick, which here comes from different channels in different chambers."""
    planes = competing_channels()
    est = (np.array([[31.0, 130.0, 229.0], [30.0, 131.0, 230.0]]), np.array([[30.0, 31.0, 29.0], [131.0, 130.0, 129.0]]))
    xp, refined, want = run_both(mg, monkeypatch, planes, tags(), 6000, search=search, est=est, seed=7)
    hold_to_oracle(xp, refined, want, 3)
    if search == ["c0", "c1"]:  # (the oracle alone: the input does what it is meant to)
        names = ["c0", "c1", "c2"]
        alone = [rp.find_rois(planes, est[0], est[1], tags(), [names.index(c)], MIN_R, MAX_R, CHAMBER_R, LENGTH, 0.1, 6000,
                              0.2, seed=0)[3] for c in search]
        x_o = want[3]
        assert (np.abs(x_o - alone[0]) <= 1).sum() >= 1 and (np.abs(x_o - alone[1]) <= 1).sum() >= 1
        assert (np.abs(alone[0] - alone[1]) >= 2).all()


def test_float32_image(mg, monkeypatch):
    img = border_chip().astype(np.float32) * np.float32(0.37) + np.float32(11.5)
    xp, refined, want = run_both(mg, monkeypatch, img[None], tags((1, 0)), 6000)
    assert np.asarray(xp.roi.values).dtype == np.float32
    hold_to_oracle(xp, refined, want, 1)
    assert refined[2][1, 0] == MAX_R and (refined[2][tags((1, 0)) != ""] <= 11).all()
