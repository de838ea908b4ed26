"""The flat-field passes at their margins, against tests/flatfield_ref.py (NumPy float64): the four maxima kernels of
pass 1 on near-ties and out-of-range flats, the truncation switch of integer pass 2 on every pixel value against flats
whose reciprocal is not a float64, and the same arithmetic in the fused ROI gather.  Every comparison is exact: the
maxima bit for bit (`flatfield_ref.same_maxima`: one NaN is as good as another -- 0 / 0 has the sign bit set on x86 and
clear on the device, and numpy.max hands back whichever it meets), the images byte for byte wherever NumPy's cast is
defined (`flatfield_ref.representable`).  tests/test_cpu_flatfield_ref.py holds the fixtures to their conditions.

Which kernel a case reaches (launch_max / launch_apply of mg_flatfield.hip, restated in `max_route` / `apply_route` and
asserted in every test):

pass 1
  * "int"     k_flatfield_max_int: integer pixels, no dark image, no flat image, 0 < flat < 1e300, |dark| < 1e300, tiles
              on 16 bytes and a group of a multiple of 16 bytes.  test_integer_kernel (a group of 3 x 5 x 7 uint16 is 210
              bytes: the same operands then reach "generic").
  * "lean"    k_flatfield_max_lean: integer pixels, no dark image, a float32 flat image on 16 bytes, tile_elems % N == 0,
              a dark that is a float32 (|dark| < 2^24) AND scratch of tile_elems / N floats -- hotpath.flatfield_max always
              brings it.  SHARE (a lane also tests against the group's published maximum) is on while a lane has fewer than
              512 chunks: on for groups of 6 tiles of 32 x 64 (one workgroup, which publishes), off for 512 tiles;
              `lean_share` computes the flag from walk_shapes.flatfield_max.  At these sizes a lane makes one trip and
              never looks at the published value (that needs a tile of more than 2 x 1536 x 256 chunks, 12 MiB: the
              second trip is tests/test_gpu_walks.py's).
  * "fast"    k_flatfield_max_fast: the same conditions without scratch -- the bare mg_flatfield_max of a C caller.
  * "generic" k_flatfield_max: everything else -- a float64 flat image, a dark of 0.1 (no float32), a dark image, float
              pixels, a ragged group.
pass 2
  * "aligned" k_apply_stitch_aligned: integer pixels, hx % N == 0, tx % N == 0, clip % N == 0, every base on 16 bytes:
              2 x 2 tiles of 256 x 256 uint16 with overlap 0 and 16, 16 x 16 uint8 with overlap 0.  INT_DARK when the dark
              is a scalar integer in [0, 65535] (0, 100), else float64 subtraction (99.5, a dark image).  Two groups with
              different maxima share one block of 8 planes: the factors are made again inside it.
  * "generic" k_stitch<BL_FLAT> (mg_stitch_kernel.h, correct_pixel): overlap 7.
  * blend="linear" and a shifts table go through mg_blendop.h's correct_pixel.
  * hotpath.flatfield_apply_planes: the SUBSET instances of both.
fused gather: k_roi_u16_even<1> (dark 100) and <2> (dark 99.5) through correct_chunk_rk<uint16_t, 2>.

Min/max rows are compared with those of the expected image; where a pixel's reference value is not representable the
expected image holds what the kernel wrote (nothing else is defined there), so the rows are checked everywhere."""
import numpy as np
import pytest

import blend_ref as br
import flatfield_ref as fr
import walk_shapes as ws
from oracle import ref_numeric as rn
from oracle import ref_pipeline as rp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def aligned16(t):
    return t.data_ptr() % 16 == 0


# ---- routes, restated from the launchers ------------------------------------------------------------------------------
def max_route(d_tiles, tiles_per_group, flat, dark, scratch):
    """launch_max: flat / dark are Python scalars or device tensors."""
    size = d_tiles.element_size()
    n = 16 // size
    elems = d_tiles.shape[-2] * d_tiles.shape[-1]
    integer = d_tiles.dtype in (torch.uint8, torch.uint16)
    flat_image, dark_image = isinstance(flat, torch.Tensor), isinstance(dark, torch.Tensor)
    if integer and not dark_image and not flat_image and 0.0 < flat < 1e300 and abs(dark) < 1e300 and aligned16(d_tiles) \
            and (tiles_per_group * elems * size) % 16 == 0:
        return "int"
    if integer and not dark_image and flat_image and flat.dtype == torch.float32 and elems % n == 0 and aligned16(flat) \
            and aligned16(d_tiles) and abs(dark) < 16777216.0 and float(np.float32(dark)) == dark:
        return "lean" if scratch else "fast"
    return "generic"


def apply_route(d_tiles, overlap, flat, dark, d_image):
    """launch_apply."""
    n = 16 // d_tiles.element_size()
    ty, tx = d_tiles.shape[-2:]
    clip, _, hx = overlap // 2, ty - overlap, tx - overlap
    integer = d_tiles.dtype in (torch.uint8, torch.uint16)
    bases = [d_tiles, d_image] + [f for f in (flat, dark) if isinstance(f, torch.Tensor)]
    return "aligned" if integer and hx % n == 0 and tx % n == 0 and clip % n == 0 and all(aligned16(b) for b in bases) else "generic"


def lean_share(dtype, n_groups, tiles_per_group, tile_elems):
    """launch_max's SHARE flag, from the grid walk_shapes.flatfield_max states: (chunks, 2 x lanes) of the lean walk."""
    cvec, two_lanes = ws.flatfield_max(dtype, "lean", n_groups, tiles_per_group, tile_elems)["items"]
    return ws.cdiv(cvec, two_lanes // 2) * tiles_per_group < 512


def run_max(hp, d_tiles, n_groups, flat, dark, scratch=True):
    """Pass 1 through hotpath.flatfield_max, or as a C caller without scratch (scalar dark, float32 flat image)."""
    if scratch:
        return hp.flatfield_max(d_tiles, flat, dark, n_groups).cpu().numpy()
    from magnify_amd import _native as nat

    ty, tx = d_tiles.shape[-2:]
    n_tiles = d_tiles.numel() // (ty * tx)
    max2 = torch.full((n_groups, 2), -np.inf, dtype=torch.float64, device="cuda")
    nat.check(nat.lib().mg_flatfield_max(d_tiles.data_ptr(), nat.dtype_code(d_tiles.dtype), n_tiles, n_groups, ty, tx, float(dark),
                                         0, 0, 0.0, flat.data_ptr(), nat.MG_F32, max2.data_ptr(), 0, 0, hp._stream()),
              "mg_flatfield_max")
    return max2.cpu().numpy()


def check_max(hp, tiles, flat, dark, route, what):
    """One scene (n_groups, tiles_per_group, ty, tx) through the route it is meant for, against `maxima`."""
    n_groups, tpg = tiles.shape[:2]
    d_tiles = dev(tiles)
    d_flat = dev(flat) if isinstance(flat, np.ndarray) else flat
    d_dark = dev(dark) if isinstance(dark, np.ndarray) else dark
    assert max_route(d_tiles, tpg, d_flat, d_dark, route != "fast") == route, what
    got = run_max(hp, d_tiles, n_groups, d_flat, d_dark, scratch=route != "fast")
    want = fr.maxima(tiles, flat, dark, n_groups)
    assert fr.same_maxima(got, want), (what, got, want)
    return want


# ---- pass 1: near-ties ------------------------------------------------------------------------------------------------
# (pixels, dark, flat type, route)
TIE_ROUTES = [(px, dark, "float32", route) for px in ("uint16", "uint8") for dark in (100.0, 99.5) for route in ("lean", "fast")]
TIE_ROUTES += [("uint16", 100.0, "float64", "generic"), ("uint16", 0.1, "float32", "generic"),
               ("float32", 100.0, "float32", "generic"), ("float64", 100.0, "float32", "generic")]


@pytest.mark.parametrize("pixels,dark,flat_type,route", TIE_ROUTES)
def test_near_ties(hp, pixels, dark, flat_type, route):
    """Three groups of six 32 x 64 tiles; group 1's maximum is decided between two pixels whose exact quotients differ by
    each band of relative gap (down to an exact tie), met in either order, in one chunk, in the same chunk of tiles 0
    and 5 (one lane, two four-tile trips) and in a tile's first and last chunk; then eight rising steps of
    [2e-6, 8e-6] along one lane.  Integer pixels: the chunk of the second pixel has its largest pixel on a flat of 8
    (the d_rcmax filter must take the chunk's largest reciprocal, not that pixel's)."""
    if route == "lean":
        assert lean_share(pixels, 3, fr.TIE_TILES, 32 * 64)  # SHARE on (uint16: 256 chunks, 256 lanes -- workgroup 0 publishes)
    for band in fr.GAP_BANDS:
        for order in fr.ORDERS:
            for placement in fr.PLACEMENTS:
                tiles, flat, info = fr.near_tie_scene(pixels, dark, band, order, placement)
                want = check_max(hp, tiles, flat.astype(flat_type), dark, route, (band, order, placement))
                (xb, flb) = info["pair"][1]
                assert want[1, 1] == max(xb - dark, 0.0) / np.float64(flb)
    tiles, flat, info = fr.staircase_scene(pixels, dark)
    want = check_max(hp, tiles, flat.astype(flat_type), dark, route, "staircase")
    x, fl = info["steps"][-1]
    assert want[1, 1] == max(x - dark, 0.0) / np.float64(fl)


@pytest.mark.parametrize("dark", [100.0, 99.5])
def test_near_ties_without_the_shared_maximum(hp, dark):
    """One group of 512 tiles of 32 x 64 uint16 (2 MiB): 512 chunks a lane, the lean kernel without SHARE -- both values
    of the flag occur in this file.  The pair sits in one chunk, in tiles 0 and 511, in a tile's first and last chunk."""
    assert not lean_share("uint16", 1, 512, 32 * 64) and lean_share("uint16", 3, fr.TIE_TILES, 32 * 64)
    for band in fr.GAP_BANDS:
        for order in fr.ORDERS:
            for placement in fr.PLACEMENTS:
                tiles, flat, info = fr.near_tie_scene("uint16", dark, band, order, placement, n_groups=1, tiles_per_group=512)
                assert tiles.nbytes == 2 << 20
                if placement == "tiles":
                    assert [t for t, _ in info["spots"]] == [0, 511]
                want = check_max(hp, tiles, flat, dark, "lean", (band, order, placement))
                (xb, flb) = info["pair"][1]
                assert want[0, 1] == max(xb - dark, 0.0) / np.float64(flb)


# ---- pass 1: the integer kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_integer_kernel(hp, dtype):
    """Scalar flat and scalar dark: a dark above every pixel (maxima 0, 0), a negative and a fractional one; uint8 has 16
    pixels a vector.  Groups of 3 tiles of 5 x 7 are no multiple of 16 bytes: the generic kernel, the same answer."""
    rng = np.random.default_rng(61)
    top = np.iinfo(dtype).max
    for shape, route in (((3, 4, 40, 48), "int"), ((3, 3, 5, 7), "generic"), ((2, 1, 1, 16), "int")):
        tiles = rng.integers(top // 8, top // 2, size=shape).astype(dtype)
        tiles[1, -1, -1, -3] = top - 1
        assert ((shape[1] * shape[2] * shape[3] * tiles.itemsize) % 16 == 0) == (route == "int")
        for flat in (0.8, 3.0, float(np.float32(0.6)), 1e-40, 1e299):
            for dark in (float(top), float(top) + 0.5, -7.0, -0.25, 33.75, 0.0, top // 4 + 0.5):
                want = check_max(hp, tiles, flat, dark, route, (shape, flat, dark))
                if dark >= top:
                    assert want.tolist() == [[0.0, 0.0]] * shape[0]
                else:
                    assert (want[:, 0] > 0).all() and (want[:, 1] == want[:, 0] / flat).all()


# ---- pass 1: special flats --------------------------------------------------------------------------------------------
SPECIAL_ROUTES = [("lean", "float32"), ("fast", "float32"), ("generic", "float32"), ("generic", "float64")]


@pytest.mark.parametrize("route,flat_type", SPECIAL_ROUTES)
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_special_flats(hp, dtype, route, flat_type):
    """0, -1, NaN, inf, a float32 denormal, 1e-30f, 1e30f and 2e-30f in the flat image, under pixels at or below the dark
    level and above it: 0 / 0, t / 0, a NaN flat (case "all": M2 is NaN, as numpy.max has it); then without the largest
    quotients, one after the other, so that every special decides a maximum once.  The generic kernel is reached with a
    float32 flat through a dark image (all 100 or 99.5) and with a float64 flat."""
    for dark in (100.0, 99.5):
        for case in fr.SPECIAL_CASES:
            tiles, flat, where = fr.special_scene(dtype, dark, case, flat_dtype=flat_type)
            dark_op = np.full(flat.shape, dark) if (route, flat_type) == ("generic", "float32") else dark
            want = check_max(hp, tiles, flat, dark_op, route, (case, dark))
            if case == "all":
                kinds = {(k, row) for _, _, k, row in where}
                assert {(fr.ZERO, "dark"), (fr.ZERO, "above"), (fr.NAN, "dark")} <= kinds and np.isnan(want[:, 1]).all()
            else:
                assert not np.isnan(want[[0, 2], 1]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_flats_and_pixels_float(hp, dtype):
    """Float pixels (the generic kernel): the special flats, then NaN and inf PIXELS -- group 0 has an inf pixel, group 1
    a NaN pixel (M1 and M2 are NaN), group 2 neither."""
    for case in fr.SPECIAL_CASES:
        tiles, flat, _ = fr.special_scene(dtype, 100.0, case)
        check_max(hp, tiles, flat, 100.0, "generic", case)
    for case in ("small", "two_tiny", "all"):
        tiles, flat, _ = fr.special_scene(dtype, 100.0, case)
        tiles[0, 2, 9, 70] = np.inf
        tiles[1, 4, 20, 33] = np.nan
        tiles[2, 0, 0, 0] = -np.inf
        want = check_max(hp, tiles, flat, 100.0, "generic", case)
        assert np.isinf(want[0, 0]) and np.isnan(want[1]).all() and np.isfinite(want[2, 0])
        want = check_max(hp, tiles, 0.75, 100.0, "generic", case)  # a scalar flat: M2 = M1 / flat
        assert np.isinf(want[0]).all() and np.isnan(want[1]).all() and np.isfinite(want[2]).all()


# ---- pass 2 -----------------------------------------------------------------------------------------------------------
def stitched(per_tile, overlap):
    return rp.stitch(per_tile, overlap)


def expected_image(tiles, flat, dark, max2, ppg, overlap, got):
    """`correct` stitched, with the kernel's own pixels where the reference value is not representable; the mask."""
    want = stitched(fr.correct(tiles, flat, dark, max2, ppg), overlap)
    rep = stitched(fr.representable(tiles, flat, dark, max2, ppg), overlap)
    assert want.shape == got.shape and want.dtype == got.dtype
    return np.where(rep, want, got), rep


def check_image(got, minmax, want, what):
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    planes = want.reshape((-1,) + want.shape[-2:])
    mm = minmax.reshape(-1, 2)
    np.testing.assert_array_equal(mm[:, 0], planes.min(axis=(1, 2)).astype(np.float64), err_msg=str(what))
    np.testing.assert_array_equal(mm[:, 1], planes.max(axis=(1, 2)).astype(np.float64), err_msg=str(what))


def operand(v):
    return dev(v) if isinstance(v, np.ndarray) else v


def near_integer(tiles, flat, dark, max2, ppg):
    """Pixels with t > 0 whose reference value lies within 1e-6 of an integer: the ones that take the exact path."""
    v = fr.correct_f64(tiles, flat, dark, max2, ppg)
    with np.errstate(all="ignore"):
        return (np.abs(v - np.rint(v)) < 1e-6) & (fr.dark_subtracted(tiles, dark) > 0) & fr.representable(tiles, flat, dark, max2, ppg)


def switch_scene(dtype):
    tiles = fr.all_values_tiles(dtype, 4)  # 4 planes of 2 x 2 tiles, two groups of two planes
    return tiles, fr.ratio_flat(tiles.shape[-2:])


def dark_image(shape, seed=77):
    return np.random.default_rng(seed).integers(60, 140, size=shape).astype(np.uint16)


def group_rows(i):
    """Two groups with different maxima in one launch: supplied pair i and the one after it."""
    return np.array([fr.SWITCH_MAX2[i], fr.SWITCH_MAX2[(i + 1) % len(fr.SWITCH_MAX2)]], dtype=np.float64)


@pytest.mark.parametrize("dark", [0.0, 100.0, 99.5, "image"])
@pytest.mark.parametrize("i_max2", range(len(fr.SWITCH_MAX2)))
def test_truncation_switch_u16(hp, i_max2, dark):
    """Every uint16 value under every flat of the ratio image, with supplied maxima: thousands of pixels whose fast
    product sits within an ulp of an integer, where only the switch to the exact path truncates like the reference."""
    tiles, flat = switch_scene(np.uint16)
    dark = dark_image(flat.shape) if isinstance(dark, str) else dark
    max2 = group_rows(i_max2)
    assert near_integer(tiles, flat, dark, max2, 2).sum() >= 1000
    if isinstance(dark, float) and dark == 0.0 and i_max2 in (1, 4, 5, 6):  # M2 = M1 / fl: wrong without the switch even with the exact reciprocal
        assert fr.at_risk(tiles, flat, dark, max2, 2, "rn")[:2].sum() >= 100
    d_tiles, d_flat, d_dark, d_max2 = dev(tiles), dev(flat), operand(dark), dev(max2)
    for overlap, route in ((0, "aligned"), (16, "aligned"), (7, "generic")):
        img, minmax = hp.flatfield_stitch(d_tiles, overlap, d_flat, d_dark, max2=d_max2, n_groups=2)
        assert apply_route(d_tiles, overlap, d_flat, d_dark, img) == route
        got = img.cpu().numpy()
        want, rep = expected_image(tiles, flat, dark, max2, 2, overlap, got)
        assert rep.mean() > 0.4
        check_image(got, minmax.cpu().numpy(), want, (overlap, route))


@pytest.mark.parametrize("variant", ["uint8", "float64_flat"])
def test_truncation_switch_variants(hp, variant):
    """16 x 16 uint8 tiles holding every value (aligned at overlap 0: 16 pixels a vector; generic at 7), and uint16
    against the float64 ratio flat (the same values: load_field's float64 branch)."""
    dtype = np.uint8 if variant == "uint8" else np.uint16
    tiles, flat = switch_scene(dtype)
    flat = flat.astype(np.float64) if variant == "float64_flat" else flat
    routes = ((0, "aligned"), (7, "generic")) if variant == "uint8" else ((0, "aligned"), (16, "aligned"), (7, "generic"))
    d_tiles, d_flat = dev(tiles), dev(flat)
    for dark in (0.0, 10.0, 9.5):
        for i in range(len(fr.SWITCH_MAX2)):
            max2 = group_rows(i)
            d_max2 = dev(max2)
            for overlap, route in routes:
                img, minmax = hp.flatfield_stitch(d_tiles, overlap, d_flat, dark, max2=d_max2, n_groups=2)
                assert apply_route(d_tiles, overlap, d_flat, dark, img) == route
                got = img.cpu().numpy()
                want, _ = expected_image(tiles, flat, dark, max2, 2, overlap, got)
                check_image(got, minmax.cpu().numpy(), want, (dark, i, overlap))


@pytest.mark.parametrize("overlap", [16, 7])
def test_truncation_switch_selected_planes(hp, overlap):
    """hotpath.flatfield_apply_planes: plane 0 of every group of two, then the complement -- the selection lands in its
    place and leaves the rest alone, both together are the reference image and its min/max rows."""
    tiles, flat = switch_scene(np.uint16)
    max2, dark, sentinel = group_rows(0), 100.0, 54321
    d_tiles, d_flat, d_max2 = dev(tiles), dev(flat), dev(max2)
    hy = 256 - overlap
    out = torch.full((4, 1, 2 * hy, 2 * hy), sentinel, dtype=torch.uint16, device="cuda")
    minmax = torch.empty((4, 2), dtype=torch.float64, device="cuda")
    hp.flatfield_apply_planes(d_tiles, overlap, d_flat, dark, d_max2, 0b01, 2, out, minmax)
    got = out.cpu().numpy()
    want, _ = expected_image(tiles, flat, dark, max2, 2, overlap, got)
    assert got[[0, 2]].tobytes() == want[[0, 2]].tobytes() and (got[[1, 3]] == sentinel).all()
    mm = minmax.cpu().numpy()
    assert (mm[[1, 3], 0] == np.inf).all() and (mm[[1, 3], 1] == -np.inf).all()
    hp.flatfield_apply_planes(d_tiles, overlap, d_flat, dark, d_max2, 0b10, 2, out, minmax, init_minmax=False)
    got = out.cpu().numpy()
    want, _ = expected_image(tiles, flat, dark, max2, 2, overlap, got)
    check_image(got, minmax.cpu().numpy(), want, overlap)


@pytest.mark.parametrize("dark", [100.0, 99.5])
def test_truncation_switch_blend_and_shift(hp, dark):
    """blend="linear" mixes the corrected values of the tiles around a seam (tests/blend_ref.py on `correct`'s tiles);
    a table of zero shifts gives the bytes of the plain pass."""
    tiles, flat = switch_scene(np.uint16)
    max2, overlap = group_rows(2), 16
    d_tiles, d_flat, d_max2 = dev(tiles), dev(flat), dev(max2)
    per_tile, _ = hp.flatfield_stitch(d_tiles.reshape(16, 1, 1, 1, 256, 256), 0, d_flat, dark, max2=dev(np.repeat(max2, 8, axis=0)),
                                      n_groups=16, want_minmax=False)
    per_tile = per_tile.cpu().numpy().reshape(tiles.shape)
    rep = fr.representable(tiles, flat, dark, max2, 2)
    values = np.where(rep, fr.correct(tiles, flat, dark, max2, 2), per_tile)
    assert per_tile.tobytes() == values.tobytes()
    img, minmax = hp.flatfield_stitch(d_tiles, overlap, d_flat, dark, max2=d_max2, n_groups=2, blend="linear")
    check_image(img.cpu().numpy(), minmax.cpu().numpy(), br.blend(values, overlap), "blend")
    plain, plain_mm = hp.flatfield_stitch(d_tiles, overlap, d_flat, dark, max2=d_max2, n_groups=2)
    check_image(plain.cpu().numpy(), plain_mm.cpu().numpy(), stitched(values, overlap), "plain")
    shifted, shifted_mm = hp.flatfield_stitch(d_tiles, overlap, d_flat, dark, max2=d_max2, n_groups=2,
                                              shifts=np.zeros((2, 2, 2), dtype=np.int32))
    assert shifted.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert shifted_mm.cpu().numpy().tobytes() == plain_mm.cpu().numpy().tobytes()


# ---- pass 2: operands outside the fast path's range -------------------------------------------------------------------
# one group per row: an ordinary quotient of 1 / 4 (no value of the ratio flat overflows); M1 == 0; M2 == inf; maxima of
# 1e300 and more (quotient 1 / 4 again, but outside group_quotient's range); M1 / M2 = 2e30
RANGE_MAX2 = np.array([(16383.75, 65535.0), (0.0, 60000.0), (60000.0, np.inf), (1e300, 4e300), (1.2e35, 60000.0)])


@pytest.mark.parametrize("dark", [100.0, 99.5])
def test_out_of_range_operands(hp, dark):
    """The special flats in the ratio image (rr == 0: flat_bad, or 2e-30f: in range with a factor beyond 61035, rk_large)
    and maxima that group_quotient refuses: those chunks take the reference's own operations.  Only planted pixels are
    left out of the comparison -- those whose reference value is inf, NaN, negative or beyond 65535.  The group with
    M1 / M2 = 2e30 is at the dark level except under the flats of 1e30f and inf, where its values are representable."""
    tiles = fr.all_values_tiles(np.uint16, 5, grid=(1, 2))
    flat = fr.ratio_flat((256, 256))
    where = fr.special_positions(flat.shape, *fr.SPECIAL_CASES["all"])
    planted = np.zeros(flat.shape, dtype=bool)
    for y, x, k, row in where:
        flat[y, x] = fr.SPECIAL_FLATS[k]
        planted[y, x] = True
        if row == "dark":
            tiles[..., y, x] = np.minimum(tiles[..., y, x], 99)
        else:
            tiles[..., y, x] = 12345 if k == fr.HUGE else np.maximum(tiles[..., y, x], 101)
    keep = np.zeros(flat.shape, dtype=bool)
    for y, x, k, row in where:
        keep[y, x] = k in (fr.HUGE, fr.INF)
    tiles[4] = np.where(keep, tiles[4], np.minimum(tiles[4], 99))
    ppg = 1
    rep_tiles = fr.representable(tiles, flat, dark, RANGE_MAX2, ppg)
    left_out = ~rep_tiles
    assert not (left_out & ~planted).any()  # only planted positions
    per_tile = left_out.reshape(-1, 256, 256).sum(axis=(1, 2))
    assert (per_tile <= len(where)).all() and (per_tile < 0.001 * 256 * 256).all() and per_tile[:8].min() > 0
    assert (fr.correct(tiles, flat, dark, RANGE_MAX2, ppg)[4] > 0).sum() >= 2  # something to see under 1e30f
    d_tiles, d_flat, d_max2 = dev(tiles), dev(flat), dev(RANGE_MAX2)
    for overlap, route in ((0, "aligned"), (7, "generic")):
        img, minmax = hp.flatfield_stitch(d_tiles, overlap, d_flat, dark, max2=d_max2, n_groups=5)
        assert apply_route(d_tiles, overlap, d_flat, dark, img) == route
        got = img.cpu().numpy()
        want, rep = expected_image(tiles, flat, dark, RANGE_MAX2, ppg, overlap, got)
        assert (~rep).sum() <= left_out.sum()
        check_image(got, minmax.cpu().numpy(), want, (overlap, route))


# ---- the fused gather -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dark", [100.0, 99.5])
def test_fused_gather_on_the_ratio_flat(hp, dark):
    """hotpath.roi_gather_reduce(raw=RawChannels(...)): two assays of three channels, each plane the all-values tile
    (rolled), channels 1 and 2 gathered from the raw stack and corrected by the ROI kernel against the ratio flat with
    supplied maxima; channel 0 comes corrected from the image block.  Windows of 64 on every band of the flat, at the
    borders, at even and odd columns.  The roi pixels are `correct`'s, cropped."""
    A, C, h, w, L = 2, 3, 256, 256, 64
    stack = fr.all_values_tiles(np.uint16, A * C, grid=(1, 1)).reshape(A, C, h, w)
    flat = fr.ratio_flat((h, w))
    max2 = np.array([fr.SWITCH_MAX2[1], fr.SWITCH_MAX2[4]])  # M2 = M1 / 3 and M1 / 0.75: see test_cpu_flatfield_ref.py
    rows = [(lo + hi) // 2 for lo, hi in fr.band_rows(h)]
    cols = [0, 33, 64, 97, 128, 161, 200, 231, 255]
    centres = [np.array([(r, c, 5) for r, c in zip(rows, cols)], dtype=np.int32),
               np.array([(r, c, 6) for r, c in zip(rows, cols[::-1])] + [(0, 0, 4), (255, 255, 4)], dtype=np.int32)]
    d_stack, d_flat, d_max2 = dev(stack), dev(flat), dev(max2)
    tiles6 = stack.reshape(A * C, 1, 1, 1, h, w)
    image = torch.full((A * C, 1, h, w), 43981, dtype=torch.uint16, device="cuda")
    minmax = torch.empty((A * C, 2), dtype=torch.float64, device="cuda")
    hp.flatfield_apply_planes(d_stack.view(A * C, 1, 1, 1, h, w), 0, d_flat, dark, d_max2, 0b001, C, image, minmax)

    def refuse():
        raise AssertionError("the fused kernel refused a call it is meant to take")

    raw = hp.RawChannels(d_stack, 0b110, d_flat, dark, d_max2, C, refuse)
    res = hp.roi_gather_reduce(image.view(A, C, 1, h, w), centres, L, None, disks=True, raw=raw)
    roi = res["roi"].cpu().numpy()
    want = fr.correct(tiles6, flat, dark, max2, C).reshape(A, C, h, w)
    rep = fr.representable(tiles6, flat, dark, max2, C).reshape(A, C, h, w)
    near = near_integer(tiles6, flat, dark, max2, C).reshape(A, C, h, w)
    risk = fr.at_risk(tiles6, flat, dark, max2, C, "rn").reshape(A, C, h, w)
    g, lefts, near_seen, risk_seen = 0, set(), 0, 0
    for a in range(A):
        for row, col, _ in centres[a]:
            top, bottom, left, right = rn.bounding_box(int(col), int(row), L, w, h)
            lefts.add(left % 2)
            win = np.s_[:, top:bottom, left:right]
            got = roi[g][:, 0]
            assert got.shape == want[a][win].shape
            expect = np.where(rep[a][win], want[a][win], got)
            assert got.tobytes() == expect.tobytes(), (a, row, col, int((got != expect).sum()))
            near_seen += int(near[a][win][1:].sum())
            risk_seen += int(risk[a][win][1:].sum())
            g += 1
    # (a window over the band of 3 or 0.75 holds the band's 28 rows x 64 columns in two raw channels; 3026 of 65535
    # values are truncated wrongly by the fast product alone: some 160 pixels a window)
    assert g == len(roi) and lefts == {0, 1} and near_seen >= 1000 and risk_seen >= 100
