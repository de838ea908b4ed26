"""The skew oracle alone (tests/skew_ref.py): it finds the tilt of every shared chip within one pixel at
the rim of the inscribed disk, tells a chip from a plane without a grid by the confidence, and keeps its bin indices in
range at the steepest angles.  The kernel and ``magnify_amd.skew`` are held to it by tests/test_gpu_skew.py."""
import numpy as np
import pytest

pytest.importorskip("scipy")

import skew_cases as sc  # noqa: E402
import skew_ref as sr  # noqa: E402


@pytest.mark.parametrize("name", list(sc.chips()))
def test_oracle_finds_the_tilt(name):
    plane, feature, tilt = sc.chips()[name]
    rotation, confidence = sr.estimate_rotation(plane, feature)
    print(name, plane.dtype, plane.shape, "rotation", rotation, "confidence", confidence, "tolerance", sc.tolerance(plane))
    assert abs(rotation + tilt) <= sc.tolerance(plane)
    assert confidence >= 2.5


@pytest.mark.parametrize("name", list(sc.blanks()))
def test_oracle_has_no_confidence_in_a_plane_without_a_grid(name):
    plane, feature, _ = sc.blanks()[name]
    _, confidence = sr.estimate_rotation(plane, feature)
    print(name, "confidence", confidence)
    assert confidence <= 1.5


@pytest.mark.parametrize("shape", [(8, 8), (33, 47), (128, 61)])
def test_bin_indices_stay_in_range_at_the_steepest_angles(shape):
    h, w = shape
    nb = min(h, w) + 2
    for angle in (-44.9, 44.9, 0.0):
        kr, kc, inside = sr.bin_indices(h, w, sr.angle_table([angle])[0])
        assert inside.any()
        for k in (kr, kc):
            k = np.broadcast_to(k, (h, w))[inside]
            assert 0 <= k.min() and k.max() < nb, (shape, angle, k.min(), k.max())
    # every pixel of the disk is counted once per axis, whatever the angle
    plane = np.random.default_rng(1).integers(0, 65536, size=shape).astype(np.uint16)
    sums, counts = sr.profiles(plane, [-44.9, 0.0, 44.9])
    n = int(sr.bin_indices(h, w, (32768, 0))[2].sum())
    assert (counts.sum(axis=-1) == n).all() and (sums.sum(axis=-1) == sums[0, 0].sum()).all()


def test_float_planes_are_quantised_over_their_range():
    plane = np.array([[-1.5, 0.0], [2.5, np.nan]], dtype=np.float64)
    q, valid = sr.quantise(plane, lo=0.0, scale=65535.0 / 2.0)
    np.testing.assert_array_equal(q[valid], [0, 0, 65535])
    np.testing.assert_array_equal(valid, [[True, True], [True, False]])
    assert sr.float_range(np.array([[3.0, 3.0]]))[1] == 0.0
    with pytest.raises(ValueError):
        sr.float_range(plane)


def test_policy_numbers():
    assert [sr.coarse_bin(f) for f in (4, 15.9, 16, 31, 32, 64, 200)] == [1, 1, 2, 2, 4, 8, 8]
    step, angles = sr.coarse_angles(16, 2, 550, 10.0)
    assert step == np.degrees(8 / 1100) and len(angles) == 49 and angles[24] == 0.0 and angles[-1] >= 10.0
    assert sr.vertex(np.array([0.0, 3.0, 4.0, 3.0]), np.array([0.0, 1.0, 2.0, 3.0])) == 2.0
    assert sr.vertex(np.array([5.0, 3.0, 1.0]), np.array([0.0, 1.0, 2.0])) == 0.0  # (at the table's end: as it is)


def _rotate_step(pipe):
    return dict(pipe.components)["rotate"]


def test_pipelines_pass_the_settings_of_the_estimate_to_rotate():
    """Host side only, nothing launched: what the builders hand to ``rotate`` and what they refuse."""
    import magnify_amd as mg
    from magnify_amd import skew

    assert mg.skew is skew and "skew" in mg.__all__
    assert _rotate_step(mg.microfluidic_chip_pipe()).keywords == {"rotation": 0}  # a numeric rotation: as it was
    assert _rotate_step(mg.image_pipe(rotation=-3.5, rotation_max=99)).keywords == {"rotation": -3.5}
    chip = _rotate_step(mg.microfluidic_chip_pipe(rotation="auto", min_button_diameter=12, search_channel=["egfp", "bf"],
                                                  search_timestep=[3, 1], rotation_max=5.0)).keywords
    assert chip == {"rotation": "auto", "rotation_feature": 12, "rotation_max": 5.0, "rotation_channel": "egfp",
                    "rotation_min_confidence": 2.0, "rotation_time": 1}
    chip = _rotate_step(mg.microfluidic_chip_pipe(rotation="auto", rotation_feature=20)).keywords
    assert chip["rotation_feature"] == 20 and chip["rotation_channel"] is None and chip["rotation_time"] == 0
    image = _rotate_step(mg.image_pipe(rotation="auto", rotation_channel="bf", rotation_min_confidence=3)).keywords
    assert image == {"rotation": "auto", "rotation_feature": 16, "rotation_max": 10.0, "rotation_channel": "bf",
                     "rotation_min_confidence": 3, "rotation_time": 0}
    bad = [dict(rotation_max=0), dict(rotation_max=45), dict(rotation_max=float("nan")), dict(rotation_feature=3.9),
           dict(rotation_feature="wide"), dict(rotation_feature=True), dict(rotation_min_confidence=-1),
           dict(rotation="straight")]
    for settings in bad:
        for build in (mg.image_pipe, mg.microfluidic_chip_pipe):
            with pytest.raises(ValueError):
                build(**{"rotation": "auto", **settings})
    assert skew.check_rotation("auto", 4, 44.9, 0) is True and skew.check_rotation(12.5) is False
    with pytest.raises(ValueError):
        skew.check_rotation(float("inf"))


def test_host_policy_equals_the_oracles():
    from magnify_amd import _native as nat
    from magnify_amd import skew

    angles = np.linspace(-44.9, 44.9, 77)
    np.testing.assert_array_equal(skew.angle_table(angles), sr.angle_table(angles))
    assert [skew.coarse_bin(f) for f in (4, 15.9, 16, 32, 64)] == [sr.coarse_bin(f) for f in (4, 15.9, 16, 32, 64)]
    for args in ((16, 2, 550, 10.0), (10, 1, 160, 10.0), (12, 1, 235, 44.0)):
        got, want = skew.coarse_angles(*args), sr.coarse_angles(*args)
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])
    rng = np.random.default_rng(2)
    sums = rng.integers(1, 1 << 40, size=(5, 2, 63)).astype(np.uint64)
    counts = rng.integers(1, 1 << 20, size=(5, 2, 63)).astype(np.uint32)
    np.testing.assert_array_equal(skew.score(sums, counts), sr.score(sums, counts))
    assert (skew.MAX_ANGLES, skew.MAX_SIDE, nat.DEFINES["MG_SKEW_TILE"]) == (64, 32768, 64)
    assert len(nat.PROTOTYPES["mg_skew_profiles"]) == 12


def test_the_entry_refuses_on_the_host():
    """Every refusal comes before anything touches the device, so it can be asked for here (the pointers are never
    read); tests/test_gpu_skew.py repeats them with real buffers and looks at the outputs."""
    from magnify_amd import _native as nat

    good = dict(d_plane=4096, dtype=nat.MG_U16, h=40, w=48, row_stride=48, lo=0.0, scale=0.0, d_cs=8192, n_angles=3,
                d_sums=16384, d_counts=32768, stream=0)
    bad = [dict(d_plane=0), dict(d_plane=4097), dict(d_cs=0), dict(d_cs=8194), dict(d_sums=0), dict(d_sums=16388),
           dict(d_counts=0), dict(d_counts=32770), dict(dtype=17), dict(dtype=-1), dict(h=7), dict(w=7), dict(h=32769),
           dict(w=32769), dict(row_stride=47), dict(n_angles=0), dict(n_angles=65), dict(lo=float("nan")),
           dict(lo=float("inf")), dict(scale=float("nan")), dict(scale=float("-inf"))]
    for override in bad:
        assert nat.lib().mg_skew_profiles(*{**good, **override}.values()) == -1, override
