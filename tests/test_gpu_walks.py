"""Every capped launch through a second trip of its walk ("Capped launches and who walks them twice").

The launchers cap their grids and the kernels stride over the rest; the edge-case shapes of the other test files give
every workgroup one item and one plane.  Each case here (tests/walk_shapes.py; tests/test_cpu_walks.py holds the list to
its preconditions) is the smallest shape that sends a workgroup round again -- the loop's increment, the index split
on a later trip, what a workgroup carries from one item or plane to the next, the barriers around LDS that is filled
again -- through the product's own Python entry, the whole output against the oracle and by the rule of that entry's
own test file: bit for bit everywhere here."""
import numpy as np
import pytest
import torch

import blend_ref as br
import depth_ref as dr
import drift_ref as df
import plot_ref as pr
import ref_shading as rsh
import register_ref as reg
import roi_ref
import roishow_ref as rs
import rotate_ref as rr
import skew_ref as sr
import unmix_ref as ur
import walk_shapes as ws
from oracle import ref_pipeline as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import magnify_amd
    import magnify_amd.hotpath

    magnify_amd.hotpath.require_gpu()
    magnify_amd.seed(2468)
    return magnify_amd


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.uint16).cuda()
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def cases(*entries, loop=None):
    picked = [c for c in ws.cases_of(*entries) if loop in (None, c.loop)]
    assert picked, entries
    return pytest.mark.parametrize("case", picked, ids=lambda c: c.id)


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=what)


# ---- depth stacks ------------------------------------------------------------------------------------------------------

@cases("mg_depth_project")
def test_depth_project(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    n, z = s["n"], s["z"]
    block = dr.random_stack(np.random.default_rng(41), np.dtype(s["dtype"]).type, (n, z, s["h"], s["w"]))
    if block.dtype.kind == "f":
        block[1, 1, -1, -1] = np.nan  # in the last block of lanes of its plane
    picks = np.array([(3 * i + 1) % z for i in range(n)])  # another slice for every stack
    want = {"max": np.stack(dr.over_stacks(dr.project_max, block)), "mean": np.stack(dr.over_stacks(dr.project_mean, block)),
            "pick": block[np.arange(n), picks]}
    d = dev(block)
    for method in ("max", "mean", "pick"):
        got = host(mg.depth.project(d, method, picks if method == "pick" else None))
        assert dr.same(got, want[method]), (case.id, method)


@cases("mg_depth_focus_totals", loop="items")
def test_depth_focus_totals_carries_its_sum_over_tiles(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    block = dr.random_stack(np.random.default_rng(42), np.uint16, (s["n"], s["z"], s["h"], s["w"]))
    yy, xx = np.mgrid[0:s["h"], 0:s["w"]]
    block[5] = (((yy + xx) & 1) * 65535).astype(np.uint16)  # the largest sum a workgroup can carry
    got = mg.depth.focus_totals(dev(block))
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(host(got), np.stack(dr.over_stacks(dr.focus_totals, block)))


@cases("mg_depth_focus_totals", loop="planes")
def test_depth_focus_totals_folds_a_second_slice_in_one_workgroup(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    n, z, h, w = s["n"], s["z"], s["h"], s["w"]
    block = dr.random_stack(np.random.default_rng(43), np.uint8, (n, z, h, w))
    want = np.stack(dr.over_stacks(dr.focus_totals, block))
    d = dev(block)
    np.testing.assert_array_equal(host(mg.depth.focus_totals(d)), want)
    assert want[-60:].all()
    # the entry zeroes its totals itself, past the cap of the clearing kernel as well: 2 words a slice
    assert 2 * n * z > ws.D["MG_ZERO_WALK"] * 256
    nat = mg.hotpath.nat
    dirty = torch.full((n, z), 7, dtype=torch.int64, device="cuda")
    assert nat.lib().mg_depth_focus_totals(d.data_ptr(), nat.dtype_code(d.dtype), n, z, h, w, dirty.data_ptr(),
                                           mg.hotpath._stream()) == 0
    np.testing.assert_array_equal(host(dirty), want)


@cases("mg_depth_fuse")
def test_depth_fuse(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    block = dr.random_stack(np.random.default_rng(44), np.uint8, (s["n"], s["z"], s["h"], s["w"]))
    image, index = mg.depth.fuse(dev(block), 2 * s["k"] + 1)
    want = dr.over_stacks(dr.fuse, block, s["k"])
    want_index = np.stack([w[1] for w in want])
    assert want_index[-60:].any() and not want_index[-60:].all()
    assert np.array_equal(host(index), want_index)
    assert dr.same(host(image), np.stack([w[0] for w in want]))


# ---- rotate ------------------------------------------------------------------------------------------------------------

def rotate_on_device(mg, image, angle):
    out, minmax = mg.hotpath.rotate_image(dev(image), angle, want_minmax=True)
    return host(out), host(minmax)


def plane_minmax(want):
    """(planes, 2) float64 as np.min / np.max give them: a NaN plane gives NaN."""
    planes = want.reshape(-1, want.shape[-2] * want.shape[-1]).astype(np.float64)
    return np.stack([planes.min(axis=1), planes.max(axis=1)], axis=1)


@cases("mg_affine_bilinear", loop="items")
def test_rotate_carries_a_planes_minmax_over_its_tiles(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    n = s["n"]
    stack = rr.random_image(np.random.default_rng(45), s["dtype"], (n, 1, s["h"], s["w"]))
    shrink = (1 + np.arange(n) % 7).reshape(n, 1, 1, 1)  # every plane its own range: a min / max in the wrong plane shows
    stack = (stack // shrink + (np.arange(n) % 5).reshape(n, 1, 1, 1)).astype(s["dtype"])
    got, minmax = rotate_on_device(mg, stack, -3.25)
    want = rr.rotate(stack, -3.25)
    same_bits(got, want, case.id)
    np.testing.assert_array_equal(minmax, plane_minmax(want), err_msg=case.id)
    assert len(np.unique(minmax[:, 1])) > 5


@cases("mg_affine_bilinear", loop="planes")
def test_rotate_starts_a_second_plane_afresh(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    n = s["n"]
    stack = rr.random_image(np.random.default_rng(46), "float32", (n, 1, s["h"], s["w"]))
    stack *= (1 + np.arange(n) % 13).reshape(n, 1, 1, 1).astype(np.float32)
    first, second = 3, 3 + ws.MAX_Y  # the two planes of one workgroup
    stack[first] = np.nan
    stack[7 + ws.MAX_Y] = np.nan
    got, minmax = rotate_on_device(mg, stack, 180.0)
    want = rr.rotate(stack, 180.0)
    same_bits(got, want, case.id)
    want_minmax = plane_minmax(want)
    assert np.isnan(want_minmax[first]).all() and np.isfinite(want_minmax[second]).all() and np.isfinite(want_minmax[7]).all()
    np.testing.assert_array_equal(minmax, want_minmax, err_msg=case.id)


# ---- bin ---------------------------------------------------------------------------------------------------------------

@cases("mg_bin_planes")
def test_bin_planes(mg, case):
    from magnify_amd import track

    ws.require_second_trip(case)
    s = case.shape
    top = 255 if s["dtype"] == "uint8" else 65535
    planes = np.random.default_rng(47).integers(0, top + 1, size=(s["n_t"], s["h"], s["w"])).astype(s["dtype"])
    got = host(track.bin_planes(dev(planes), s["b"]))
    assert got.tobytes() == df.bin_planes(planes, s["b"]).tobytes(), case.id


# ---- percentiles -------------------------------------------------------------------------------------------------------

@cases("mg_percentile_histogram")
def test_percentiles_of_more_windows_than_workgroups(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    rng = np.random.default_rng(48)
    shape = (s["units"], s["channels"], 1, 3, 3)  # (mark, channel, time, L, L): the roi layout
    assert s["unit_len"] == 9
    # the windows of the second trip -- the last ones: a window is a chunk -- hold both ends of the range and nobody
    # else does: without them, or with another window read in their place, the outer percentiles move
    first = ws.D["MG_PERCENTILE_WALK"]
    tail = (s["units"] - first,) + shape[1:]
    if np.dtype(s["dtype"]).kind == "u":
        top = np.iinfo(s["dtype"]).max
        roi = rng.integers(top // 8, top - top // 8, size=shape).astype(s["dtype"])
        ends = np.where(rng.random(tail) < 0.5, rng.integers(0, top // 8, size=tail), rng.integers(top - top // 8, top + 1, size=tail))
        roi[first:] = ends.astype(s["dtype"])
    else:
        bits = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
        roi = np.where(np.isfinite(bits) & (np.abs(bits) < 1e30), bits, np.float32(1.5)).astype(s["dtype"])
        roi[first:] = (np.where(rng.random(tail) < 0.5, -1.0, 1.0) * rng.uniform(2.7e38, 3.3e38, size=tail)).astype(s["dtype"])
    d_roi = dev(roi)
    qs = (0, 1, 50, 99.8, 100)
    for c in range(s["channels"]):
        view = d_roi[:, c]
        assert not view.is_contiguous()
        got = mg.hotpath.percentiles(view, qs)  # uint16 and the floats: refinement passes with prefixes
        want = np.array([rs.percentile(roi[:, c], q) for q in qs])
        without = np.array([rs.percentile(roi[:first, c], q) for q in qs])
        assert (want[[0, 1, 3, 4]] != without[[0, 1, 3, 4]]).all(), case.id
        np.testing.assert_array_equal(got, want, err_msg=case.id)


# ---- unmix -------------------------------------------------------------------------------------------------------------

def same_f32(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok], err_msg=what)


@cases("mg_unmix_planes")
def test_unmix_planes(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    rng = np.random.default_rng(49)
    img = rng.integers(0, np.iinfo(s["dtype"]).max, (s["n_c"], s["n_t"], s["h"], s["w"]), endpoint=True).astype(s["dtype"])
    if case.loop == "items":
        matrix, ratios = np.array([[0.75, -1.25]]), False
    else:
        matrix, ratios = rng.normal(0, 1, (2, 2)), True
    with np.errstate(all="ignore"):
        want = ur.planes(img, [1, 0], matrix, [10.0, -3.5], ratios).astype(np.float32)
    got = host(mg.hotpath.unmix_planes(dev(img), matrix, [1, 0], [10.0, -3.5], ratios))
    same_f32(got, want, case.id)


# ---- skew --------------------------------------------------------------------------------------------------------------

@cases("mg_skew_profiles")
def test_skew_profiles(mg, case):
    from magnify_amd import skew

    ws.require_second_trip(case)
    s = case.shape
    plane = rr.random_image(np.random.default_rng(50), s["dtype"], (s["h"], s["w"]))
    sums, counts = skew.profiles(dev(plane), list(s["angles"]))
    want_sums, want_counts = sr.profiles(plane, list(s["angles"]))
    np.testing.assert_array_equal(counts, want_counts, err_msg=case.id)
    np.testing.assert_array_equal(sums, want_sums, err_msg=case.id)


# ---- overview and label map ----------------------------------------------------------------------------------------------

@cases("mg_render_overview")
def test_overview(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    image = rr.random_image(np.random.default_rng(51), s["dtype"], (1, s["n_t"], s["h"], s["w"]))
    top = float(np.iinfo(s["dtype"]).max)
    limits, colors = [(0.1 * top, 0.8 * top)], [(1.0, 0.5, 0.25)]
    got = host(mg.hotpath.render_overview(dev(image), s["level"], limits, colors))
    np.testing.assert_array_equal(got, pr.overview(image, s["level"], limits, colors), err_msg=case.id)


@cases("mg_roi_image_labels")
def test_image_labels(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    m, n_t, L, h, w = s["m"], s["n_t"], s["roi_len"], s["h"], s["w"]
    rng = np.random.default_rng(52)
    fg = rng.random((m, n_t, L, L)) < 0.3
    origin = np.stack([rng.integers(-L // 2, h - L // 2, (m, n_t)), rng.integers(-L // 2, w - L // 2, (m, n_t))], axis=-1)
    origin = origin.astype(np.int32)
    got = host(mg.hotpath.image_labels(dev(fg), origin, s["level"], h, w))
    want = pr.image_labels(fg, origin, s["level"], h, w)
    assert (want > m - 200).any()  # the markers of the second trip are in the picture
    np.testing.assert_array_equal(got, want, err_msg=case.id)


# ---- the row groups of a stitch pass -------------------------------------------------------------------------------------

@cases("mg_flatfield_apply_stitch", "mg_flatfield_apply_stitch_blend", "mg_flatfield_apply_stitch_shift")
def test_stitch_walks_the_row_groups_of_one_tall_plane(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    v = s["overlap"]
    n_rows = 1 if v == 0 else 2
    ty, tx = s["h_out"] // n_rows + v, s["w_out"] + v
    tiles = np.random.default_rng(53).integers(5, 60000, size=(1, 1, n_rows, 1, ty, tx)).astype(s["dtype"])
    tiles[0, 0, -1, 0, -10, tx // 2], tiles[0, 0, -1, 0, -12, tx // 2] = 65535, 0  # the extremes: in the rows of the second trip
    table = np.array([[[2, -3]], [[-4, 1]]], dtype=np.int32) if case.name == "shift" else None  # within overlap // 2
    image, minmax = mg.hotpath.flatfield_stitch(dev(tiles), v, apply_flatfield=False, blend="linear" if s["blend"] else None,
                                                shifts=table)
    moved = tiles if table is None else reg.shift_tiles(tiles, table)
    want = br.blend(moved, v) if s["blend"] else br.plain(moved, v)
    assert want.shape[-2:] == (s["h_out"], s["w_out"])
    same_bits(host(image), want, case.id)
    np.testing.assert_array_equal(host(minmax), [[want.min(), want.max()]], err_msg=case.id)
    assert want.max() == 65535 and want.min() == 0 and 5 <= want[..., :2048, :].min() and want[..., :2048, :].max() < 60000


@cases("mg_plane_minmax")
def test_plane_minmax(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    top = int(np.iinfo(s["dtype"]).max)
    planes = np.random.default_rng(54).integers(3, 250, size=(s["n"], s["h"], s["w"])).astype(s["dtype"])
    planes[0, -1, -5], planes[1, -2, 7] = top, 0  # in the vectors of the second trip (the last four rows, at the most)
    got = host(mg.hotpath.plane_minmax(dev(planes)))
    np.testing.assert_array_equal(got, [[3, top], [0, 249]], err_msg=case.id)


# ---- the montage ---------------------------------------------------------------------------------------------------------

@cases("mg_render_roi_montage")
def test_roi_montage(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    m, L = s["m"], s["roi_len"]
    rng = np.random.default_rng(55)
    roi = rng.integers(0, 256, size=(m, 1, s["n_t"], L, L)).astype(s["dtype"])
    layout = np.full(s["rows"] * s["cols"], -1, dtype=np.int32)
    layout[:m] = rng.permutation(m)  # the last cells are empty
    layout = layout.reshape(s["rows"], s["cols"])[::-1].copy()  # ... and lie in the first rows of the picture
    limits, colors = [(20.0, 200.0)], [(1.0, 0.5, 0.25)]
    got = host(mg.hotpath.render_roi_montage(dev(roi), layout, s["level"], limits, colors))
    want = rs.roishow(roi, layout, s["level"], limits, colors, overlay=None)
    assert want[:, -L:].any()  # the cells of the second trip are not empty
    np.testing.assert_array_equal(got, want, err_msg=case.id)


# ---- pass 1 of the flat-field correction -----------------------------------------------------------------------------------

@cases("mg_flatfield_max", "mg_flatfield_bound")
def test_flatfield_maxima(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    g, ty, tx = s["n_groups"], s["ty"], s["tx"]
    rng = np.random.default_rng(56)
    dark = 100.0
    if s["path"] == "int":  # scalar operands: the integer maximum of the group decides both
        tiles = rng.integers(0, 50000, size=(g, 1, 1, 1, ty, tx)).astype(s["dtype"])
        flat = 1.7
        flat_host = np.float64(flat)
        assert (tiles.size // g * tiles.itemsize) % 16 == 0
    else:  # a flat image: the generic kernel for float pixels; for integer pixels the kernels with and without its bound
        tiles = (rng.random((g, 1, 1, 1, ty, tx)) * 50000).astype(s["dtype"])
        flat = (0.6 + 0.8 * rng.random((ty, tx))).astype(np.float32)
        flat[-1, -2:] = 0.5
        flat_host = flat.astype(np.float64)
    for i in range(g):  # every group's maxima lie in the vectors (and the tail) of its last trip
        tiles[i, 0, 0, 0, -1, -1 - (i % 2)] = 60000 + i
    d_tiles = dev(tiles)
    if s["path"] == "fast":  # a C caller without the bound of the flat image
        nat, d_flat = mg.hotpath.nat, dev(flat)
        max2 = torch.full((g, 2), -np.inf, dtype=torch.float64, device="cuda")
        nat.check(nat.lib().mg_flatfield_max(d_tiles.data_ptr(), nat.dtype_code(d_tiles.dtype), g, g, ty, tx, dark, 0, 0, 0.0,
                                             d_flat.data_ptr(), nat.MG_F32, max2.data_ptr(), 0, 0, mg.hotpath._stream()),
                  "mg_flatfield_max")
        got = host(max2)
    else:
        got = host(mg.hotpath.flatfield_max(d_tiles, dev(flat) if s["path"] != "int" else flat, dark, g))
    t = np.maximum(tiles.astype(np.float64) - dark, 0.0).reshape(g, ty, tx)
    want = np.stack([t.max(axis=(1, 2)), (t / flat_host).max(axis=(1, 2))], axis=1)
    assert (want[:, 0] == 59900.0 + np.arange(g)).all()
    np.testing.assert_array_equal(got, want, err_msg=case.id)


# ---- the shading correction fused with the stitch --------------------------------------------------------------------------

@cases("mg_shading_apply_stitch")
def test_shading_apply_walks_row_groups(mg, case):
    ws.require_second_trip(case)
    s = case.shape
    c, t, ty, tx = 2, s["n_planes"] // 2, s["h_out"], s["w_out"]
    rng = np.random.default_rng(57)
    tiles = rng.integers(0, 65536, size=(c, t, 1, 1, ty, tx)).astype(s["dtype"])
    flats = (0.4 + 1.2 * rng.random((c, ty, tx))).astype(np.float32)
    darks = (0.3 * 65535 * rng.random((c, ty, tx))).astype(np.float32)
    flats[:, : ty - 8], darks[:, : ty - 8] = np.maximum(flats[:, : ty - 8], 1.0), np.maximum(darks[:, : ty - 8], 100.0)
    flats[:, -3, 5], darks[:, -3, 5], darks[:, -2, 7] = 0.01, 0.0, 65535.0  # the extremes: in the rows of the second trip
    tiles[:, :, 0, 0, -3, 5], tiles[:, :, 0, 0, -2, 7] = 60000, 5
    want = rp.stitch(np.stack([rsh.apply_mirrored(tiles[i], flats[i], darks[i]) for i in range(c)]), 0)
    got, minmax = mg.shading.apply_stitch(dev(tiles), 0, dev(flats), dev(darks))
    got, minmax = host(got), host(minmax)
    same_bits(got, want, case.id)
    planes = want.reshape(c * t, -1)
    np.testing.assert_array_equal(minmax, np.stack([planes.min(1), planes.max(1)], 1).astype(np.float64), err_msg=case.id)
    assert (planes.max(1) == 65535).all() and (planes[:, : (ty - 8) * tx].max(1) < 65535).all()


# ---- the marker table and the unpacked edge map ------------------------------------------------------------------------------

@cases("mg_marker_table")
def test_marker_table(mg, case):
    ws.require_second_trip(case)
    m, n_assays = case.shape["m"], case.shape["n_assays"]
    rng = np.random.default_rng(58)
    cuts = [0, m // 5, m // 2, m]
    assert len(cuts) == n_assays + 1
    beads = rng.integers(0, 4096, size=(m, 3)).astype(np.int32)
    assays = [beads[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    counts = rng.integers(0, 900, size=(m, 2)).astype(np.int32)
    sums = rng.integers(0, 2 ** 40, size=(m, 1, 1, 2)).astype(np.float64)
    out = {"beads": assays, "counts": dev(counts), "sums": dev(sums)}
    got = host(mg.hotpath.marker_table(out, 7, 1))
    np.testing.assert_array_equal(got, roi_ref.marker_table_ref(assays, 7, counts, sums, 0), err_msg=case.id)


@cases("mg_unpack_bits")
def test_unpack_bits(mg, case):
    ws.require_second_trip(case)
    n_planes, n_bits = case.shape["n_planes"], case.shape["n_bits"]
    words = -(-n_bits // 32) + 3  # a plane stride with room to spare
    bits = np.random.default_rng(59).integers(0, 2 ** 32, size=(n_planes, words), dtype=np.uint64).astype(np.uint32)
    d_bits = torch.from_numpy(bits.view(np.int32)).cuda()
    out = torch.full((n_planes, n_bits), 9, dtype=torch.uint8, device="cuda")
    nat = mg.hotpath.nat
    nat.check(nat.lib().mg_unpack_bits(d_bits.data_ptr(), words, n_planes, n_bits, out.data_ptr(), mg.hotpath._stream()),
              "mg_unpack_bits")
    want = np.unpackbits(bits.view(np.uint8).reshape(n_planes, -1), axis=1, bitorder="little")[:, :n_bits]
    np.testing.assert_array_equal(host(out), want, err_msg=case.id)
