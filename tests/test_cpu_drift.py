"""``find_beads(track="ncc", stage_drift=D)`` without a GPU: the NumPy restatement (tests/drift_ref.py) recovers drawn
offsets far beyond max_drift; the host side of magnify_amd/track.py (anchors, vote, refusals) against it; the keywords
and the binding.

The scenes of ``drift_ref.SCENES`` are the ones tests/test_gpu_drift.py runs the device on."""
import inspect

import numpy as np
import pytest

import drift_ref as dr


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("case", dr.SCENES, ids=["384x352", "288x320"])
def test_the_restatement_recovers_every_drawn_offset(case, seed):
    shape, drifts, border, D = case
    planes, beads, offsets = dr.scene(seed, shape, dr.N_BEADS, dr.R_LO, dr.R_HI, dr.JITTER, drifts, D=border)
    assert dr.N_BEADS // 2 <= len(beads) <= dr.N_BEADS  # (the rejection sampler may place fewer than asked)
    assert (np.abs(offsets).max(axis=(0, 2))[1:] > dr.MAX_DRIFT).any()  # the plain search could not follow
    stage, res = dr.follow(planes, beads, dr.HALF, dr.MAX_DRIFT, D)
    print(case, seed, "stage", stage["shift"].tolist(), "agree", stage["agree"].tolist(), "smallest score", res["score"].min(),
          "smallest gap", res["gap"].min())
    np.testing.assert_array_equal(res["shift"], offsets)
    assert (res["score"] > 0.99).all() and (res["gap"] > 1e-6).all()
    # the coarse offset is within the fine search's reach of the drift, with room for the bead's own motion
    assert (np.abs(stage["shift"] - np.asarray(drifts)) <= dr.MAX_DRIFT - dr.JITTER).all()
    assert (stage["agree"] >= 0.5).all() and not stage["shift"][0].any()
    # today's search (base 0) loses the timepoints that drifted by more than max_drift (a bead may land on another
    # one's place and score there: most, not all)
    plain = dr.track_based(planes, beads, dr.HALF, dr.MAX_DRIFT, np.zeros((len(drifts), 2), dtype=int))
    far = np.abs(np.asarray(drifts)).max(axis=1) > dr.MAX_DRIFT + dr.JITTER
    assert far.any() and np.median(plain["score"][:, far]) < 0.5 and (plain["shift"][:, far] != offsets[:, far]).any(axis=-1).all()


def test_anchor_tables_of_known_shapes():
    from magnify_amd import track

    for fn in (dr.anchors, track.stage_anchors):
        a = fn(96, 88, 10)
        assert a.shape == (4, 3) and (a[:, 2] == 16).all()
        assert a[:, 0].tolist() == [26, 26, 59, 59] and a[:, 1].tolist() == [26, 59, 26, 59]
        a = fn(512, 512, 16)
        assert a.shape == (25, 3) and (a[:, 2] == 47).all()
        assert sorted(set(a[:, 0].tolist())) == sorted(set(a[:, 1].tolist())) == [63, 158, 253, 348, 443]
        assert a[:6, 0].tolist() == [63] * 5 + [158] and a[:6, 1].tolist() == [63, 158, 253, 348, 443, 63]  # raster order
        with pytest.raises(ValueError):
            fn(40, 40, 16)
    assert track.stage_anchors(96, 88, 10).dtype == np.int32
    # every shape: unclipped, disjoint, within what mg_track_beads takes
    for hb, wb, mc in ((96, 88, 10), (512, 512, 16), (72, 80, 10), (131, 300, 13), (50, 50, 16)):
        a = track.stage_anchors(hb, wb, mc)
        np.testing.assert_array_equal(a, dr.anchors(hb, wb, mc))
        half = int(a[0, 2])
        assert len(a) >= 1 and 2 * half + 1 + 2 * mc <= 127 and half >= 4
        assert (a[:, 0] - half >= mc).all() and (a[:, 0] + half < hb - mc).all()
        assert (a[:, 1] - half >= mc).all() and (a[:, 1] + half < wb - mc).all()
        rows, cols = np.unique(a[:, 0]), np.unique(a[:, 1])
        assert (np.diff(rows) >= 2 * half + 1).all() and (np.diff(cols) >= 2 * half + 1).all()


def test_stage_bins():
    from magnify_amd import track

    for D in (1, 2, 31, 32, 33, 64, 65, 100, 127, 128):
        b, mc = track.stage_bin(D)
        assert (b, mc) == dr.stage_bin(D) and mc <= 16 and b * mc >= D
    assert [track.stage_bin(D) for D in (32, 33, 64, 65, 128)] == [(2, 16), (4, 9), (4, 16), (8, 9), (8, 16)]


# picks (A, T, 2) and scores (A, T) with T = 2, time 1 under test: name -> (picks at t = 1, scores at t = 1, shift, agree)
VOTES = {
    "all agree": ([(3, -2)] * 4, [0.9] * 4, (12, -8), 1.0),
    "an even k takes the lower median": ([(2, 5), (3, 5), (2, 6), (3, 6)], [0.9] * 4, (8, 20), 1.0),
    "no voter": ([(3, -2)] * 4, [0.2] * 4, (0, 0), 0.0),
    "a split vote is not trusted": ([(0, 0), (9, 9), (-9, 4), (5, -7)], [0.9] * 4, (0, 0), 0.25),
    "one bin off still agrees": ([(4, 4), (5, 3), (3, 5), (4, 4)], [0.9] * 4, (16, 16), 1.0),
    "two bins off does not": ([(4, 4), (6, 4), (4, 4), (4, 2)], [0.9] * 4, (16, 16), 0.5),
    "half the voters is enough": ([(4, 4), (4, 4), (9, 9), (-9, -9)], [0.9] * 4, (16, 16), 0.5),
    "less than half is not": ([(4, 4), (4, 4), (9, 9), (-9, -9), (-5, 20)], [0.9] * 5, (0, 0), 0.4),
    "anchors below min_score do not vote": ([(4, 4), (9, 9), (9, 9), (4, 4)], [0.9, 0.1, 0.49, 0.5], (16, 16), 0.5),
    "one voter": ([(7, 7), (-3, 2), (1, 1)], [0.1, 0.8, 0.1], (-12, 8), 1 / 3),
}


@pytest.mark.parametrize("name", sorted(VOTES))
def test_the_vote(name):
    from magnify_amd import track

    at_1, score_1, want_shift, want_agree = VOTES[name]
    n_a = len(at_1)
    picks = np.zeros((n_a, 3, 2), dtype=np.int32)
    scores = np.ones((n_a, 3))
    picks[:, 1], scores[:, 1] = at_1, score_1
    picks[:, 2], scores[:, 2] = (5, 5), 0.0  # row t_ref = 2 below: its picks and scores do not count
    for t_ref in (0, 2):
        shift, agree = track.stage_vote(picks, scores, 4, 0.5, t_ref)
        ref_shift, ref_agree, _ = dr.vote(picks, scores, 4, 0.5, t_ref)
        assert shift.dtype == np.int32 and shift.shape == (3, 2) and agree.dtype == np.float64 and agree.shape == (3,)
        np.testing.assert_array_equal(shift, ref_shift, err_msg=name)
        np.testing.assert_array_equal(agree, ref_agree, err_msg=name)
        assert tuple(shift[1]) == want_shift and agree[1] == want_agree, name
        assert tuple(shift[t_ref]) == (0, 0) and agree[t_ref] == 1.0, name
    assert tuple(track.stage_vote(picks, scores, 4, 0.5, 0)[0][2]) == (0, 0)  # no voter at t = 2


def test_check_stage_drift_refusals():
    import magnify_amd as mg
    from magnify_amd import track

    assert track.check_stage_drift(None, None) is None and track.check_stage_drift(None, "ncc", 1) is None
    assert track.check_stage_drift(40, "ncc", 8) == (4, 10) and track.check_stage_drift(128, "ncc", 8) == (8, 16)
    assert track.check_stage_drift(32, "ncc", 2) == (2, 16) and track.check_stage_drift(np.int64(100), "ncc", 8) == (8, 13)
    assert track.check_stage_drift(40, "ncc", 8, (384, 352)) == (4, 10)
    for bad in (dict(stage_drift=40, track=None), dict(stage_drift=0, track="ncc"), dict(stage_drift=129, track="ncc"),
                dict(stage_drift=-3, track="ncc"), dict(stage_drift=40.0, track="ncc"), dict(stage_drift=True, track="ncc"),
                dict(stage_drift="40", track="ncc"),
                dict(stage_drift=100, track="ncc", max_drift=4),   # b = 8
                dict(stage_drift=40, track="ncc", max_drift=3),    # b = 4
                dict(stage_drift=20, track="ncc", max_drift=1),    # b = 2
                dict(stage_drift=40, track="ncc", max_drift=8, shape=(384, 100)),    # 25 binned columns: half_c = 0
                dict(stage_drift=128, track="ncc", max_drift=8, shape=(320, 320))):  # 40 x 40 binned, mc = 16
        with pytest.raises(ValueError):
            track.check_stage_drift(**bad)
    with pytest.raises(ValueError, match="at least 152"):
        track.check_stage_drift(40, "ncc", 8, (151, 400))  # 4 * (18 + 20): the side that would do
    assert track.check_stage_drift(40, "ncc", 8, (152, 400)) == (4, 10)
    for kw in (dict(stage_drift=40), dict(track="ncc", stage_drift=0), dict(track="ncc", stage_drift=129),
               dict(track="ncc", stage_drift=100, max_drift=4)):
        with pytest.raises(ValueError):
            mg.beads_pipe(**kw)


def test_the_keyword_exists_and_reaches_the_finder():
    import magnify_amd as mg

    factory = mg.registry.components.get("find_beads")
    for fn in (mg.beads, mg.beads_pipe, mg.mrbles, mg.mrbles_pipe, factory):
        params = inspect.signature(fn).parameters
        assert "stage_drift" in params and params["stage_drift"].default is None, fn
    pipe = mg.beads_pipe(track="ncc", max_drift=8, stage_drift=40)
    assert dict(pipe.components)["find_beads"].stage_drift == 40
    pipe = mg.mrbles_pipe(spectra=None, codes=None, track="ncc", max_drift=8, stage_drift=100)
    assert dict(pipe.components)["find_beads"].stage_drift == 100
    plain = factory(min_bead_diameter=5, max_bead_diameter=25, low_edge_quantile=0.1, high_edge_quantile=0.9, num_iter=100,
                    min_roundness=0.3, roi_length=None, search_channel=None, interactive=False)
    assert plain.stage_drift is None
    assert dict(mg.beads_pipe(track="ncc").components)["find_beads"].stage_drift is None


def test_the_bindings():
    import ctypes

    from magnify_amd import _native as nat

    args = nat.PROTOTYPES["mg_track_beads_based"]
    assert len(args) == 17 and args[3] is ctypes.c_int64 and nat.RESTYPES["mg_track_beads_based"] is ctypes.c_int
    assert args[11] is ctypes.c_void_p and args[10] is ctypes.c_int and args[-1] is ctypes.c_void_p
    args = nat.PROTOTYPES["mg_bin_planes"]
    assert len(args) == 9 and args[3] is ctypes.c_int64 and nat.RESTYPES["mg_bin_planes"] is ctypes.c_int
    assert args[6] is ctypes.c_int and args[7] is ctypes.c_void_p and args[-1] is ctypes.c_void_p
    assert len(nat.PROTOTYPES["mg_track_beads"]) == 16  # the plain entry is as it was
    for name in ("mg_track_beads_based", "mg_bin_planes"):
        assert hasattr(nat.lib(), name)
