"""``find_beads(track="ncc")`` without a GPU: the NumPy restatement (tests/track_ref.py) recovers drawn offsets and
breaks ties as specified; the host side of magnify_amd/track.py (tables, refusals); the keywords and the binding.

The scenes of ``SCENES`` are the ones tests/test_gpu_track.py compares the kernel on: the restatement's best score
leads the second best by more than 1e-6 at every (bead, time), so no comparison there has to leave a case out."""
import inspect

import numpy as np
import pytest

import track_ref as tr

# (shape, beads, r_lo, r_hi, m, T)
SCENES = [((256, 240), 12, 5, 12, 6, 4), ((200, 312), 10, 8, 20, 8, 3)]


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("case", SCENES, ids=["256x240", "200x312"])
def test_the_restatement_recovers_every_drawn_offset(case, seed):
    shape, n, r_lo, r_hi, m, n_t = case
    planes, beads, offsets = tr.scene(seed, shape, n, r_lo, r_hi, m, n_t)
    assert n // 2 <= len(beads) <= n and offsets[:, 1:].any()  # (the rejection sampler may place fewer than asked)
    res = tr.track(planes, beads, r_hi + 2, m)
    print(case, seed, "smallest score", res["score"].min(), "smallest gap", res["gap"].min())
    np.testing.assert_array_equal(res["shift"], offsets)
    assert (res["gap"] > 1e-6).all() and (res["score"] > 0.99).all()
    tables, followed = tr.tables(beads, res["shift"], res["score"], 0.5, *shape)
    assert followed.all()
    np.testing.assert_array_equal(tables[..., :2], (beads[None, :, :2] + offsets.transpose(1, 0, 2)))


@pytest.mark.parametrize("name", sorted(tr.TIES))
def test_an_exact_tie_goes_to_the_smaller_displacement(name):
    from magnify_amd import register

    planes, want = tr.TIES[name]
    res = tr.track(planes, tr.TIE_BEAD, tr.TIE_HALF, tr.TIE_M)
    z = res["z"][0, 1]
    assert (z == z.max()).sum() > 1 and z.max() == pytest.approx(1.0, abs=1e-12), name
    assert tuple(res["shift"][0, 1]) == want and res["gap"][0, 1] == 0.0, name
    delta, best = register.pick_displacements(z)  # the order the kernel restates
    assert tuple(delta) == want and best == z.max(), name


def test_degenerate_patches_give_shift_0_and_score_0():
    flat = np.full((3, 48, 40), 777, dtype=np.uint16)
    res = tr.track(flat, np.array([[24, 20, 5]]), 6, 3)
    assert not res["shift"].any() and list(res["score"][0]) == [1.0, 0.0, 0.0] and res["fixed"][0, 0] == 13 * 13
    rng = np.random.default_rng(0)
    planes = rng.integers(0, 4000, size=(2, 48, 40)).astype(np.uint16)
    res = tr.track(planes, np.array([[0, 0, 5]]), 4, 8)  # rows / columns <= 4 and >= 8: nothing
    assert not res["fixed"].any() and not res["sums"].any()
    assert not res["shift"].any() and list(res["score"][0]) == [1.0, 0.0]


def test_tracked_tables_clamp_and_fall_back():
    from magnify_amd import track

    beads = np.array([[5, 5, 3], [2, 90, 4], [47, 99, 6]])
    shift = np.array([[[0, 0], [-8, 3]], [[0, 0], [1, 20]], [[0, 0], [6, 6]]])
    score = np.array([[1.0, 0.9], [1.0, 0.2], [1.0, 0.5]])
    tables, followed = track.tracked_tables(beads, shift, score, 0.5, 50, 100)
    assert tables.dtype == np.int32 and tables.shape == (2, 3, 3)
    np.testing.assert_array_equal(tables[0], beads)
    np.testing.assert_array_equal(tables[1], [[0, 8, 3], [2, 90, 4], [49, 99, 6]])  # clamped; below min_score; clamped
    np.testing.assert_array_equal(followed, [[True, True], [True, False], [True, True]])
    want, want_followed = tr.tables(beads, shift, score, 0.5, 50, 100)
    np.testing.assert_array_equal(tables, want)
    np.testing.assert_array_equal(followed, want_followed)
    empty = track.tracked_tables(np.empty((0, 3)), np.empty((0, 4, 2)), np.empty((0, 4)), 0.5, 50, 100)
    assert empty[0].shape == (4, 0, 3) and empty[1].shape == (0, 4)


def test_check_track_refusals():
    from magnify_amd import track

    assert track.TRACK_MODES == (None, "ncc")
    assert track.check_track(None) is None and track.check_track("ncc", 16, 47) == "ncc"  # 95 + 32 = 127: the largest
    for bad in (dict(track="phase"), dict(track="ncc", max_drift=0), dict(track="ncc", max_drift=17),
                dict(track="ncc", max_drift=2.5), dict(track="ncc", max_drift=8, half=48),
                dict(track="ncc", max_drift=8, half=0),
                dict(track="ncc", max_drift=16, half=48),    # 2 half + 1 + 2 max_drift = 129
                dict(track="ncc", max_drift=17, half=47)):   # 129 the other way
        with pytest.raises(ValueError):
            track.check_track(**bad)


def test_the_keywords_exist_and_reach_the_finder():
    import magnify_amd as mg

    defaults = dict(track=None, max_drift=8, track_min_score=0.5, track_channel=None, track_patch=None)
    factory = mg.registry.components.get("find_beads")
    for fn in (mg.beads, mg.beads_pipe, mg.mrbles, mg.mrbles_pipe, factory):
        params = inspect.signature(fn).parameters
        for name, value in defaults.items():
            assert name in params and params[name].default == value, (fn, name)
    pipe = mg.beads_pipe(track="ncc", max_drift=6, track_min_score=0.7, track_channel="egfp", track_patch=11)
    finder = dict(pipe.components)["find_beads"]
    assert (finder.track, finder.max_drift, finder.track_min_score, finder.track_channel, finder.track_patch) == \
        ("ncc", 6, 0.7, "egfp", 11)
    plain = factory(min_bead_diameter=5, max_bead_diameter=25, low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=100,
                    min_roundness=0.3, roi_length=None, search_channel=None, interactive=False)
    assert plain.track is None and plain.max_drift == 8
    with pytest.raises(ValueError):
        mg.beads_pipe(track="phase")
    with pytest.raises(ValueError):
        mg.beads_pipe(track="ncc", max_drift=17)
    with pytest.raises(ValueError):
        mg.beads_pipe(track="ncc", max_bead_diameter=100)  # half = 52: the patch would be 105 wide


def test_the_binding_has_a_64_bit_plane_stride():
    import ctypes

    from magnify_amd import _native as nat

    args = nat.PROTOTYPES["mg_track_beads"]
    assert len(args) == 16 and args[3] is ctypes.c_int64 and nat.RESTYPES["mg_track_beads"] is ctypes.c_int
    assert args[0] is ctypes.c_void_p and args[2] is ctypes.c_int and args[-1] is ctypes.c_void_p
