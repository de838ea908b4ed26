"""tests/flatfield_ref.py against the oracle, and every fixture against the condition it was built for -- from the
reference and the simulation alone, no device: what tests/test_gpu_flatfield_limits.py runs is what it claims to be."""
import numpy as np
import pytest

import flatfield_ref as fr
from oracle import ref_pipeline as rp
from synth import vignette

DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


# ---- the reference is the oracle's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", ["scalar", "image_flat", "image_dark"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_with_its_own_maxima_is_the_oracle(dtype, operands):
    rng = np.random.default_rng(5)
    shape = (2, 3, 2, 2, 24, 40)
    top = 255 if dtype == np.uint8 else 60000
    tiles = (rng.random(shape) * top).astype(dtype)
    dark_level = 10.0 if dtype == np.uint8 else 100.0
    flat = 0.8 if operands == "scalar" else vignette(shape[-2:])
    dark = rng.integers(0, 2 * int(dark_level), size=shape[-2:]).astype(np.uint16) if operands == "image_dark" else dark_level
    max2 = fr.maxima(tiles, flat, dark, 1)
    assert max2.shape == (1, 2) and max2.dtype == np.float64
    want = rp.flatfield_correct(tiles, flat, dark)
    got = fr.correct(tiles, flat, dark, max2, 6)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert fr.representable(tiles, flat, dark, max2, 6).all()
    # per group: the oracle on each block of planes
    max3 = fr.maxima(tiles, flat, dark, 3)
    got = fr.correct(tiles, flat, dark, max3, 2)
    flat6 = got.reshape((3, 2) + shape[2:])
    for g in range(3):
        block = tiles.reshape((3, 2) + shape[2:])[g]
        assert flat6[g].tobytes() == rp.flatfield_correct(block, flat, dark).tobytes()


def test_maxima_have_numpys_nan_and_inf():
    tiles = np.array([[[[5, 0]]], [[[0, 0]]], [[[7, 3]]]], dtype=np.uint16)  # three groups of one 1 x 2 tile
    got = fr.maxima(tiles, np.array([[1.0, 0.0]], dtype=np.float32), 0.0, 3)
    assert got[:, 0].tolist() == [5.0, 0.0, 7.0]
    assert np.isnan(got[0, 1]) and np.isnan(got[1, 1]) and got[2].tolist() == [7.0, np.inf]
    assert fr.same_maxima(got, got.copy()) and not fr.same_maxima(got, np.nan_to_num(got))
    neg = np.copysign(np.float64(np.nan), -1.0)
    assert fr.same_maxima(np.array([neg, 1.0]), np.array([np.nan, 1.0]))
    assert not fr.same_maxima(np.array([0.0]), np.array([-0.0]))


def test_representable_leaves_out_what_the_cast_does_not_define():
    tiles = np.array([10, 10, 10, 10, 0, 60000], dtype=np.uint16).reshape(1, 1, 1, 1, 1, 6)
    flat = np.array([[1.0, 0.0, np.nan, -1.0, 0.0, 0.5]], dtype=np.float32)
    rep = fr.representable(tiles, flat, 0.0, [(1.0, 1.0)], 1).reshape(-1)
    assert rep.tolist() == [True, False, False, False, False, False]  # 10, inf, NaN, -10, 0 / 0, 120000
    assert fr.representable(tiles.astype(np.float32), flat, 0.0, [(1.0, 1.0)], 1).all()


# ---- pass 2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_all_values_tile_and_ratio_flat(dtype):
    tile = fr.all_values_tile(dtype)
    n = np.iinfo(dtype).max + 1
    assert tile.shape == ((256, 256) if dtype == np.uint16 else (16, 16)) and tile.dtype == dtype
    assert np.array_equal(np.sort(tile.reshape(-1)), np.arange(n))
    assert not np.array_equal(tile.reshape(-1), np.arange(n)) and np.array_equal(tile, fr.all_values_tile(dtype))
    flat = fr.ratio_flat(tile.shape)
    assert flat.dtype == np.float32 and flat.shape == tile.shape
    bands = fr.band_rows(tile.shape[0])
    assert len(bands) == 9 and bands[0][0] == 0 and bands[-1][1] == tile.shape[0]
    for (lo, hi), value in zip(bands, fr.RATIO_FLATS):
        assert hi > lo and (flat[lo:hi] == np.float32(value)).all()
    lo, hi = bands[-1]
    assert np.array_equal(flat[lo:hi], vignette(tile.shape)[lo:hi]) and len(np.unique(flat[lo:hi])) > 8
    assert fr.RATIO_FLATS[-1] == float(np.float32(0.6)) != 0.6
    # rolled tiles: with eleven of them or more every value has been under every band
    tiles = fr.all_values_tiles(dtype, 4)
    assert tiles.shape == (4, 1, 2, 2) + tile.shape
    flat_tiles = tiles.reshape((-1,) + tile.shape)
    for lo, hi in bands[:8]:
        assert len(np.unique(flat_tiles[:, lo:hi])) == n


@pytest.mark.parametrize("fl", fr.SWITCH_FLATS)
def test_a_reciprocal_one_ulp_low_truncates_wrongly(fl):
    """Ratio flat: with r = prev(1 / fl) and M1 == M2 the fast product alone is wrong for at least 1000 of the 65535
    non-zero pixel values -- and every one of them lies within 1e-6 of an integer: the margin the switch rests on."""
    t = np.arange(1, 65536)
    wrong = fr.naive_wrong(t, fl, 60000.0, 60000.0, "prev")
    assert wrong.sum() >= 1000, int(wrong.sum())
    assert (fr.distance_to_integer(t, fl, 60000.0, 60000.0)[wrong] < 1e-6).all()


def test_the_exact_reciprocal_truncates_wrongly_too():
    """With r = rn(1 / fl) and M2 = M1 / fl: at least 1000 wrong values for at least three of the flats."""
    t = np.arange(1, 65536)
    counts = {fl: int(fr.naive_wrong(t, fl, 60000.0, 60000.0 / fl, "rn").sum()) for fl in fr.SWITCH_FLATS}
    assert sum(c >= 1000 for c in counts.values()) >= 3, counts


@pytest.mark.parametrize("dark", [0.0, 100.0, 99.5])
@pytest.mark.parametrize("max2", fr.SWITCH_MAX2)
def test_every_naive_wrong_pixel_is_within_the_margin(max2, dark):
    """For every flat of the ratio image, every reciprocal one ulp around 1 / fl and every pair of maxima the device
    tests put in: a pixel the fast product gets wrong lies within 1e-6 of an integer (where the result is a uint16)."""
    x = np.arange(0, 65536)
    t = np.clip(x - dark, 0, None)
    flats = list(fr.RATIO_FLATS) + [float(v) for v in np.unique(fr.ratio_flat((256, 256))[fr.band_rows(256)[-1][0]:])[::97]]
    total = 0
    for fl in flats:
        v = ((t / fl) * max2[0]) / max2[1]
        for r in ("prev", "rn", "next"):
            wrong = fr.naive_wrong(t, fl, max2[0], max2[1], r) & (v <= 65535)
            total += int(wrong.sum())
            assert (fr.distance_to_integer(t, fl, *max2)[wrong] < 1e-6).all(), (fl, r)
    assert total > 0


def test_switch_scene_has_pixels_only_the_switch_gets_right():
    """In the device test's scene, with the correctly rounded reciprocal: every flat of 3, 5, 0.75 and 1.5 has its pair of
    maxima (M2 = M1 / fl) under which at least 100 representable pixels of its band are truncated wrongly by the fast
    product alone -- 1512 wrong values (the fewest: flat 5) x 16 tiles x 28 / 256 of a tile's rows under the band is
    over 2000; the bound leaves room for the values beyond 65535."""
    tiles = fr.all_values_tiles(np.uint16, 4)
    flat = fr.ratio_flat((256, 256))
    assert tiles.shape[0] * tiles.shape[2] * tiles.shape[3] == 16
    for fl, pair in ((3.0, fr.SWITCH_MAX2[1]), (0.75, fr.SWITCH_MAX2[4]), (1.5, fr.SWITCH_MAX2[5]), (5.0, fr.SWITCH_MAX2[6])):
        assert pair[1] == pair[0] / fl
        lo, hi = fr.band_rows(256)[fr.RATIO_FLATS.index(fl)]
        risk = fr.at_risk(tiles, flat, 0.0, [pair, pair], 2, "rn")[..., lo:hi, :]
        assert risk.sum() >= 100, (fl, int(risk.sum()))
        near = fr.distance_to_integer(tiles[..., lo:hi, :], fl, *pair)
        assert (near[risk] < 1e-6).all()


def test_switch_scene_meets_the_wrong_truncations():
    """In the scene of the device test (all-values tiles under the ratio flat) each of the five flats sees at least 500
    representable pixels per plane block that a reciprocal one ulp low would truncate wrongly: 7653 wrong values (the
    fewest: flat 5) x 16 tiles x 28 / 256 of a tile's rows under each band, well above it."""
    tiles = fr.all_values_tiles(np.uint16, 4)
    flat = fr.ratio_flat((256, 256))
    for (lo, hi), fl in zip(fr.band_rows(256), fr.SWITCH_FLATS):
        t = tiles[..., lo:hi, :].astype(np.float64)
        wrong = fr.naive_wrong(t, fl, 60000.0, 60000.0, "prev") & (t / fl <= 65535)
        assert wrong.sum() >= 500, (fl, int(wrong.sum()))
        assert (flat[lo:hi] == np.float32(fl)).all()


# ---- pass 1: near-ties ------------------------------------------------------------------------------------------------
TIE_CASES = [("uint16", 100.0), ("uint16", 99.5), ("uint8", 100.0), ("uint8", 99.5), ("uint16", 0.1)]


@pytest.mark.parametrize("dtype,dark", TIE_CASES)
def test_the_search_finds_every_band(dtype, dark):
    pairs = fr.near_tie_pairs(dtype, dark)
    assert set(pairs) == set(fr.GAP_BANDS)
    for band, ((xa, fla), (xb, flb)) in pairs.items():
        lo, hi = fr.gap_bands(dtype)[band]
        qa = max(xa - dark, 0.0) / np.float64(fla)
        qb = max(xb - dark, 0.0) / np.float64(flb)
        gap = fr.rel_gap(qa, qb)
        assert fla.dtype == np.float32 and 0.5 <= fla < 2 and 0.5 <= flb < 2 and 0 <= xa <= np.iinfo(dtype).max
        if band == "tie":
            assert qa == qb and xa != xb and fla != flb
        else:
            assert qa < qb and lo <= gap <= hi, (band, gap)
    steps = fr.staircase(dtype, dark)
    q = [max(x - dark, 0.0) / np.float64(fl) for x, fl in steps]
    assert len(q) == fr.STAIRS == 8
    for a, b in zip(q, q[1:]):
        assert 2e-6 <= fr.rel_gap(a, b) <= 8e-6


SCENE_CASES = TIE_CASES + [("float32", 100.0), ("float64", 100.0)]


@pytest.mark.parametrize("pixels,dark", SCENE_CASES)
def test_near_tie_scenes(pixels, dark):
    """Every band, both orders, all three placements: the pair decides group 1's maximum, the pixel met first is the
    one the order names, every other quotient of the group is at most half the maximum, the groups differ."""
    for band in fr.GAP_BANDS:
        for order in fr.ORDERS:
            for placement in fr.PLACEMENTS:
                tiles, flat, info = fr.near_tie_scene(pixels, dark, band, order, placement)
                assert tiles.shape == (3, 6, 32, 64) and tiles.dtype == np.dtype(pixels) and flat.dtype == np.float32
                q = fr.quotients(tiles, flat, dark)[1].reshape(6, -1)
                (t0, p0), (t1, p1) = info["spots"]
                (xa, fla), (xb, flb) = info["pair"]
                qa, qb = max(xa - dark, 0.0) / np.float64(fla), max(xb - dark, 0.0) / np.float64(flb)
                assert (t0, p0) < (t1, p1) if placement != "tiles" else t0 < t1
                first, second = (qa, qb) if order == "lower_first" else (qb, qa)
                assert q[t0, p0] == first and q[t1, p1] == second and q.max() == qb
                rest = q.copy()
                rest[t0, p0] = rest[t1, p1] = 0
                assert rest.max() <= 0.5 * q.max()
                n = 16 // np.dtype(pixels).itemsize
                if placement == "chunk":
                    assert t0 == t1 and (p0 // 8 == p1 // 8)
                elif placement == "tiles":
                    assert (t0, t1) == (0, 5) and p0 // 8 == p1 // 8 and t0 // 4 != t1 // 4
                else:
                    assert t0 == t1 and p0 // n == 0 and p1 // n == tiles[0, 0].size // n - 1
                if np.dtype(pixels).kind == "u":  # the decoy: the largest pixel of the second chunk, a small quotient
                    td, pd = info["decoy"]
                    chunk = slice(pd // n * n, pd // n * n + n)
                    assert td == t1 and p1 // n == pd // n
                    px = tiles[1].reshape(6, -1)[td, chunk]
                    assert px.argmax() == pd - chunk.start and flat.reshape(-1)[chunk].max() == flat.reshape(-1)[pd]
                    assert flat.reshape(-1)[chunk].min() >= 0.5 and q[td, pd] <= 0.5 * qb
                m = fr.maxima(tiles, flat, dark, 3)
                assert m[1, 1] == qb and len(set(m[:, 1])) == 3 and len(set(m[:, 0])) >= 2


@pytest.mark.parametrize("dtype,dark", SCENE_CASES)
def test_staircase_scene(dtype, dark):
    tiles, flat, info = fr.staircase_scene(dtype, dark)
    q = fr.quotients(tiles, flat, dark)[1].reshape(6, -1)
    steps = [q[t, p] for t, p in info["spots"]]
    assert len(steps) == 8 and [t for t, _ in info["spots"]] == [0, 1, 2, 3, 4, 5, 5, 5]
    assert len({p // 8 for _, p in info["spots"][:6]}) == 1 and info["spots"][6][1] // 8 == info["spots"][0][1] // 8 + 1
    for a, b in zip(steps, steps[1:]):
        assert 2e-6 <= fr.rel_gap(a, b) <= 8e-6
    rest = q.copy()
    for t, p in info["spots"]:
        rest[t, p] = 0
    assert q.max() == steps[-1] and rest.max() <= 0.5 * steps[0]


# ---- special flats ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dark", [100.0, 99.5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_scenes(dtype, dark, flat_dtype):
    """ "all": a 0 / 0, a t / 0 with t > 0 and a NaN flat in every group that has them; M2 is NaN there.  The other cases
    take the largest special quotient away one by one: every case has its own M2, and group 1 (dark under every special)
    differs from the groups around it wherever no NaN hides it."""
    seen = {}
    for case in fr.SPECIAL_CASES:
        tiles, flat, where = fr.special_scene(dtype, dark, case, flat_dtype=flat_dtype)
        assert tiles.dtype == np.dtype(dtype) and flat.dtype == np.dtype(flat_dtype) and tiles.shape == (3, 5, 32, 128)
        t = fr.dark_subtracted(tiles, dark)
        m = fr.maxima(tiles, flat, dark, 3)
        for y, x, k, row in where:
            assert flat[y, x] == fr.SPECIAL_FLATS[k] or k == fr.NAN and np.isnan(flat[y, x])
            assert (t[:, :, y, x] == 0).all() if row == "dark" else ((t[0, :, y, x] > 0).all() and (t[1, :, y, x] == 0).all())
        if case == "all":
            at = {(k, row): (y, x) for y, x, k, row in where}
            y, x = at[(fr.ZERO, "dark")]
            assert flat[y, x] == 0 and (t[:, :, y, x] == 0).all()                   # 0 / 0
            y, x = at[(fr.ZERO, "above")]
            assert flat[y, x] == 0 and (t[0, :, y, x] > 0).all()                    # t / 0
            assert np.isnan(flat[at[(fr.NAN, "dark")]]) and np.isnan(flat[at[(fr.NAN, "above")]])
            assert np.isnan(m[:, 1]).all() and np.isfinite(m[:, 0]).all()
        seen[case] = m[:, 1]
    assert np.isinf(seen["zero"][[0, 2]]).all() and np.isnan(seen["zero"][1])
    for case, scale in (("denormal", 1e40), ("tiny", 1e30), ("two_tiny", 5e29)):
        assert (seen[case][[0, 2]] > 0.5 * scale).all() and np.isfinite(seen[case]).all() and seen[case][1] < 1e6
    assert (seen["small"] < 1e6).all()
    assert seen["denormal"][0] > seen["tiny"][0] > seen["two_tiny"][0] > seen["small"][0]
