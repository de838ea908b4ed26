"""``stitch(register="ncc")`` without a GPU: the NumPy restatement (tests/register_ref.py) recovers drawn tile errors,
the host parts of magnify_amd/register.py (score, pick, solve) equal it, the refusals, and the keywords on the public
functions."""
import inspect

import numpy as np
import pytest

import blend_ref as br
import register_ref as rr
from synth import noisy_bead_image

R, CC, TY, TX, V, M, PAD = 3, 3, 96, 112, 24, 4, 8


@pytest.fixture(scope="module")
def jittered():
    """The 3 x 3 case of tests/test_gpu_register.py: (scene, e, tiles)."""
    rng = np.random.default_rng(11)
    hy, hx = TY - V, TX - V
    scene, _ = noisy_bead_image(1, (R * hy + V + 2 * PAD, CC * hx + V + 2 * PAD), 40, r_lo=4, r_hi=8)
    e = rr.draw_errors(rng, R, CC, M)
    return scene, e, rr.cut_jittered(scene, R, CC, TY, TX, V, e, PAD)


def test_the_restatement_recovers_the_drawn_errors(jittered):
    from magnify_amd import register

    scene, e, tiles = jittered
    shift, delta, best, used, clipped = rr.register(tiles, V, M)
    # ... and so do the host parts of the package on the restatement's sums
    sums, fixed, _, _ = rr.seam_sums(tiles, V, M)
    solved = register.solve_shifts(R, CC, register.pick_displacements(register.seam_scores(sums, fixed)), 0.5, V // 2)
    np.testing.assert_array_equal(solved[0], shift)
    want, g = rr.expected_table(e)
    assert used.all() and clipped == 0 and best.min() >= 0.99
    np.testing.assert_array_equal(shift, want)
    for s, (a, b) in enumerate(rr.seams(R, CC)):
        np.testing.assert_array_equal(delta[s], e[b] - e[a])
    crop = rr.scene_crop(scene, R, CC, TY, TX, V, PAD, e[0, 0], g)
    np.testing.assert_array_equal(rr.stitch(tiles, V, shift), crop)
    assert (br.plain(tiles, V) != crop).any()  # the unregistered stitch does not show the scene


def test_host_parts_equal_the_restatement(jittered):
    from magnify_amd import register

    _, _, tiles = jittered
    sums, fixed, _, _ = rr.seam_sums(tiles, V, M)
    np.testing.assert_array_equal(register.seam_list(R, CC),
                                  [a + b for a, b in rr.seams(R, CC)])
    z = register.seam_scores(sums, fixed)
    np.testing.assert_array_equal(z, rr.scores(sums, fixed))
    delta, best = register.pick_displacements(z)
    want_delta, want_best = rr.pick(z)
    np.testing.assert_array_equal(delta, want_delta)
    np.testing.assert_array_equal(best, want_best)
    shift, used, clipped = register.solve_shifts(R, CC, (delta, best), 0.5, V // 2)
    want = rr.solve(R, CC, want_delta, want_best, 0.5, V // 2)
    np.testing.assert_array_equal(shift, want[0])
    np.testing.assert_array_equal(used, want[1])
    assert clipped == want[2] == 0 and shift.dtype == np.int32


def test_float_tiles_score_like_integer_tiles(jittered):
    from magnify_amd import register

    _, _, tiles = jittered
    si, fi, _, _ = rr.seam_sums(tiles[:1, :2], V, 2)
    sf, ff, mag, fmag = rr.seam_sums(tiles[:1, :2].astype(np.float64), V, 2)
    assert sf.dtype == np.float64 and mag.shape == sf.shape and fmag.shape == ff.shape
    np.testing.assert_allclose(register.seam_scores(sf, ff), register.seam_scores(si, fi), rtol=0, atol=1e-9)


def test_an_exact_tie_goes_to_the_smaller_displacement():
    from magnify_amd import register

    z = np.zeros((1, 5, 5))
    z[0, 2 + 1, 2 + 1] = z[0, 2 - 1, 2 + 0] = z[0, 2 + 0, 2 - 1] = z[0, 2 + 2, 2 - 2] = 0.75
    delta, best = register.pick_displacements(z)  # |(-1, 0)| = |(0, -1)| = 1: the smaller dy wins
    assert delta.tolist() == [[-1, 0]] and best.tolist() == [0.75]
    np.testing.assert_array_equal(delta, rr.pick(z)[0])
    z[0, 2, 2] = 0.75
    assert register.pick_displacements(z)[0].tolist() == [[0, 0]] == rr.pick(z)[0].tolist()


def test_a_flat_patch_scores_zero_and_its_seam_is_unused():
    from magnify_amd import register

    rng = np.random.default_rng(2)
    tiles = rng.integers(0, 4000, size=(1, 3, 40, 48)).astype(np.uint16)
    tiles[0, 2, :, :20] = 700  # B of the second seam: flat where the patch lies
    sums, fixed, _, _ = rr.seam_sums(tiles, 16, 4)
    z = register.seam_scores(sums, fixed)
    np.testing.assert_array_equal(z, rr.scores(sums, fixed))
    assert (z[1] == 0).all() and (z[0] != 0).any()
    delta, best = register.pick_displacements(z)
    assert delta[1].tolist() == [0, 0] and best[1] == 0.0
    shift, used, _ = register.solve_shifts(1, 3, (delta, np.array([0.9, 0.0])), 0.5, 8)
    assert used.tolist() == [True, False] and shift[0, 2].tolist() == [0, 0]
    nan = np.full_like(sums, np.nan, dtype=np.float64)
    assert (register.seam_scores(nan, fixed.astype(np.float64)) == 0).all()


def test_two_components_an_isolated_tile_and_clipping():
    from magnify_amd import register

    # 2 x 3: tiles (0, 0) - (0, 1) - (1, 1) - (1, 0) form one component through three used seams, (0, 2) hangs on (1, 2)
    # alone in a second one ... and with min_score raised past its seam, (0, 2) and (1, 2) are isolated
    seams = rr.seams(2, 3)
    delta = np.zeros((len(seams), 2), dtype=np.int64)
    score = np.zeros(len(seams))
    def put(a, b, d, z):
        s = seams.index((a, b))
        delta[s], score[s] = d, z
    put((0, 0), (0, 1), (3, -2), 0.9)
    put((0, 1), (1, 1), (-1, 4), 0.9)
    put((1, 0), (1, 1), (2, 2), 0.9)
    put((0, 2), (1, 2), (6, -6), 0.7)
    for min_score in (0.5, 0.8):
        shift, used, clipped = register.solve_shifts(2, 3, (delta, score), min_score, 12)
        want = rr.solve(2, 3, delta, score, min_score, 12)
        np.testing.assert_array_equal(shift, want[0])
        np.testing.assert_array_equal(used, want[1])
        assert clipped == want[2] == 0
        # first component: e00 = 0, e01 = (3, -2), e11 = (2, 2), e10 = (0, 0); g = ((0 + 3) // 2, (-2 + 2) // 2) = (1, 0)
        assert shift[0, 0].tolist() == [-1, 0] and shift[0, 1].tolist() == [2, -2]
        assert shift[1, 1].tolist() == [1, 2] and shift[1, 0].tolist() == [-1, 0]
        if min_score == 0.5:  # second component: (0, 0) and (6, -6), g = (3, -3)
            assert used.sum() == 4 and shift[0, 2].tolist() == [-3, 3] and shift[1, 2].tolist() == [3, -3]
        else:                 # isolated tiles keep 0
            assert used.sum() == 3 and shift[0, 2].tolist() == [0, 0] == shift[1, 2].tolist()
    shift, used, clipped = register.solve_shifts(2, 3, (delta, score), 0.5, 2)  # a table that needs clipping
    want = rr.solve(2, 3, delta, score, 0.5, 2)
    np.testing.assert_array_equal(shift, want[0])
    assert clipped == want[2] == 4 and np.abs(shift).max() == 2  # (-3, 3) and (3, -3) of the second component


def test_refusals():
    import magnify_amd as mg
    from magnify_amd.stitch import Stitcher

    for kw in (dict(register="fft"), dict(register="ncc", max_shift=0), dict(max_shift=0),
               dict(register="ncc", overlap=24, max_shift=7), dict(register="ncc", register_time="all")):
        with pytest.raises(ValueError):
            Stitcher(**kw)
        with pytest.raises(ValueError):
            mg.components.get("stitch")(**kw)
    with pytest.raises(ValueError, match="register"):
        mg.image_pipe(register="fft")
    with pytest.raises(ValueError, match="max_shift"):
        mg.image_pipe(overlap=16, register="ncc", max_shift=5)
    st = Stitcher(overlap=24, register="ncc", max_shift=6, register_time="each", register_channel="egfp", min_score=0.3)
    assert (st.register, st.max_shift, st.register_time, st.register_channel, st.min_score) == ("ncc", 6, "each", "egfp", 0.3)
    assert Stitcher(overlap=3).register is None  # the default max_shift binds only when registering


def test_the_keywords_are_on_the_public_functions_and_reach_the_stitcher():
    import magnify_amd as mg
    from magnify_amd.stitch import Stitcher

    defaults = dict(register=None, max_shift=8, register_channel=None)
    for f in (mg.image, mg.beads, mg.mrbles, mg.microfluidic_chip, mg.image_pipe, mg.beads_pipe, mg.mrbles_pipe,
              mg.microfluidic_chip_pipe):
        p = inspect.signature(f).parameters
        for name, value in defaults.items():
            assert name in p and p[name].default == value, (f, name)
    p = inspect.signature(Stitcher).parameters
    assert [(k, p[k].default) for k in list(p)[2:]] == [("register", None), ("max_shift", 8), ("register_channel", None),
                                                        ("register_time", 0), ("min_score", 0.5)]
    pipes = (mg.image_pipe, mg.beads_pipe, mg.microfluidic_chip_pipe, lambda **kw: mg.mrbles_pipe(None, None, **kw))
    for make in pipes:
        stitch = dict(make(overlap=40, register="ncc", max_shift=3, register_channel=1).components)["stitch"]
        assert (stitch.register, stitch.max_shift, stitch.register_channel) == ("ncc", 3, 1)
        assert dict(make().components)["stitch"].register is None
