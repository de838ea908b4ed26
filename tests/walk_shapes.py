"""The capped launches ("Capped launches and who walks them twice"): per entry the grid its launcher asks for,
restated from the launch code over the constants of include/magnify_hip.h (read through ``magnify_amd._native``, never
restated), and the cases tests/test_gpu_walks.py runs.  No GPU, no library: tests/test_cpu_walks.py holds every case
to its precondition -- at least two trips of the loop it is meant for -- and to the size limits.

A grid function returns ``{"items": (count, workgroups), "planes": (count, workgroups)}``: what one loop of the kernel
walks and how many workgroups (or, for the flat loops, threads' worth of workgroups) share it; ``trips`` is the most
rounds one workgroup makes.  "items" is the walk inside a plane (tiles, blocks of lanes, chunks, flat indices),
"planes" the walk over blockIdx.y.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from magnify_amd import _native as nat

D = nat.DEFINES
GIB = 1 << 30
MAX_Y = D["MG_WALK_MAX_Y"]


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def size_of(dtype) -> int:
    return np.dtype(dtype).itemsize


def plane_grid(items: int, n: int, budget: int = 0, per_plane: int = 0):
    """mg_plane_grid (mg_planes.h): (x, y)."""
    gy = min(n, MAX_Y)
    gx = items
    if per_plane:
        gx = min(gx, per_plane)
    if budget:
        gx = min(gx, budget // gy)
    return max(gx, 1), gy


def _walks(items, gx, n, gy):
    return {"items": (items, gx), "planes": (n, gy)}


def _dword_lanes(pixels: int, dtype) -> int:
    """Lanes that own one aligned dword of u8 / u16 output each (one more: a run may start inside a dword)."""
    px = 4 // size_of(dtype) if size_of(dtype) < 4 else 1
    return cdiv(pixels, px) + (1 if px > 1 else 0)


# ---- the grids, as DESIGN.md states them -----------------------------------------------------------------------------

def depth_project(dtype, n, z, h, w, **_):
    items = cdiv(_dword_lanes(h * w, dtype), 256)
    return _walks(items, *_xy(plane_grid(items, n, D["MG_DEPTH_PROJECT_WALK"]), n))


def depth_focus_totals(n, z, h, w, **_):
    tiles, slices = cdiv(w, 256) * cdiv(h, 16), n * z
    return _walks(tiles, *_xy(plane_grid(tiles, slices, D["MG_DEPTH_FOCUS_WALK"], D["MG_DEPTH_FOCUS_WALK_PER_SLICE"]), slices))


def depth_fuse(n, h, w, **_):
    tiles = cdiv(w, D["MG_DEPTH_TILE"]) * cdiv(h, D["MG_DEPTH_TILE"])
    return _walks(tiles, *_xy(plane_grid(tiles, n), n))


def affine_bilinear(dtype, n, h, w, **_):
    tiles = cdiv(_dword_lanes(w, dtype), 32) * cdiv(h, 32)
    gy = min(n, MAX_Y)
    return _walks(tiles, max(1, min(tiles, D["MG_ROTATE_WALK"] // gy)), n, gy)


def bin_run(dtype, b):
    """(input columns, output columns) of one item of k_bin: a whole number of 16-byte vectors."""
    n = 16 // size_of(dtype)
    vpr = (b // n if b > n else 1) * (2 if b == 2 else 1)
    return vpr * n, vpr * n // b


def bin_planes(dtype, b, n_t, h, w, **_):
    total = n_t * (h // b) * cdiv(w // b, bin_run(dtype, b)[1])
    return _flat(total, D["MG_BIN_WALK"])


def percentile_histogram(dtype, units, unit_len, **_):
    vec = 16 // size_of(dtype)
    rounds = min(8, cdiv(cdiv(unit_len, vec), 256))
    total = units * cdiv(unit_len, 256 * rounds * vec)
    return {"items": (total, min(total, D["MG_PERCENTILE_WALK"])), "planes": (1, 1)}


def unmix_planes(n_t, h, w, **_):
    items = cdiv(cdiv(h * w, 4), 256)
    return _walks(items, *_xy(plane_grid(items, n_t, 0, D["MG_UNMIX_PLANES_WALK_PER_PLANE"]), n_t))


def skew_profiles(h, w, **_):
    tiles = cdiv(w, D["MG_SKEW_TILE"]) * cdiv(h, D["MG_SKEW_TILE"])
    return _walks(tiles, *_xy(plane_grid(tiles, 1, D["MG_SKEW_WALK"]), 1))


def overview_run(dtype, level):
    """Output columns of one item of k_overview."""
    s = 1 << level
    n = (8 if size_of(dtype) == 1 and s == 1 else 16) // size_of(dtype)
    return (s // n if s > n else 1) * n // s


def render_overview(dtype, level, n_t, h, w, **_):
    s = 1 << level
    total = n_t * cdiv(h, s) * cdiv(cdiv(w, s), overview_run(dtype, level))
    return _flat(total, D["MG_OVERVIEW_WALK"])


def roi_image_labels(m, n_t, roi_len, **_):
    return _flat(m * n_t * roi_len * cdiv(roi_len, 4), D["MG_IMAGE_LABELS_WALK"])


def render_roi_montage(n_t, rows, cols, roi_len, level, **_):
    lk = cdiv(roi_len, 1 << level)
    return _flat(n_t * rows * lk * cols * lk, D["MG_MONTAGE_WALK"])


def stitch_grid(dtype, n_planes, h_out, w_out, **_):
    """stitch_grid (mg_stitch.h): the row groups of a plane group against gridDim.y."""
    cols_planes = cdiv(w_out, 256 * (16 // size_of(dtype))) * cdiv(n_planes, 8)
    rows = 32
    while rows > 2 and cols_planes * cdiv(h_out, rows) < D["MG_STITCH_WALK_FILL"]:
        rows //= 2
    groups = cdiv(h_out, rows)
    gy = groups if rows == 32 else min(groups, max(1, D["MG_STITCH_WALK_PER_GROUP"] // max(1, cols_planes)))
    return {"items": (groups, gy), "planes": (1, 1)}


def shading_apply(n_planes, h_out, w_out, **_):
    """launch_shading_apply (mg_shading.hip): row groups of 8 rows against gridDim.y."""
    gx, groups = cdiv(w_out, 256 * 4), cdiv(h_out, 8)
    want = max(1, D["MG_SHADING_APPLY_WALK"] // max(1, gx * n_planes))
    return {"items": (groups, min(groups, want, MAX_Y)), "planes": (1, 1)}


def marker_table(m, **_):
    return _flat(m, D["MG_MARKER_TABLE_WALK"])


def unpack_bits(n_planes, n_bits, **_):
    blocks = cdiv(n_bits, 256)
    return _walks(blocks, min(blocks, D["MG_UNPACK_BITS_WALK"]), n_planes, n_planes)


def plane_minmax(dtype, n, h, w, **_):
    """k_plane_minmax (mg_flatfield.hip) has two loops.  Integer pixels in rows of whole 16-byte vectors (and aligned
    planes: the cases' are) take four vectors a lane and trip, the walk counted in vectors against four times the lanes;
    every other plane takes one vector a lane and trip."""
    vec = 16 // size_of(dtype)
    vectors = h * cdiv(w, vec)
    blocks = min(cdiv(vectors, 256), D["MG_PLANE_MINMAX_WALK"])
    if np.dtype(dtype).kind == "u" and w % vec == 0:
        return _walks(vectors, 4 * blocks * 256, n, n)
    return _walks(cdiv(vectors, 256), blocks, n, n)


def flatfield_max(dtype, path, n_groups, tiles_per_group, tile_elems, **_):
    """launch_max (mg_flatfield.hip).  "int": integer pixels, scalar dark and flat -- a lane takes four vectors of its
    group a trip, so the walk counts the vectors behind a lane's first three; "lean": integer pixels, a float32 flat
    image and its bound -- two vectors of the tile a lane and trip (UV = 2), counted in vectors against twice the lanes;
    "generic" and "fast" (a C caller without the bound): one vector of the tile a lane and trip."""
    n = 16 // size_of(dtype)
    per_group = D["MG_FLATFIELD_MAX_WALK_PER_GROUP"]
    if path == "int":
        gvec = tiles_per_group * tile_elems // n
        gb = max(1, min(gvec // 256, min(per_group, max(D["MG_FLATFIELD_MAX_INT_WALK_MIN"], D["MG_FLATFIELD_MAX_INT_WALK"] // n_groups))))
        return _walks(gvec - 3 * gb * 256, 4 * gb * 256, n_groups, n_groups)
    if path == "lean":
        cvec = tile_elems // n
        per = max(1, min(cdiv(cvec, 256), max(1, D["MG_FLATFIELD_MAX_LEAN_WALK"] // n_groups)))
        return _walks(cvec, 2 * per * 256, n_groups, n_groups)
    blocks = cdiv(tile_elems // n + 1, 256)
    return _walks(blocks, min(blocks, min(per_group, max(1, D["MG_FLATFIELD_MAX_WALK"] // n_groups))), n_groups, n_groups)


def flatfield_bound(dtype, tile_elems, **_):
    """k_flat_rcmax: one chunk of the flat image (the pixels of one vector of `dtype` tiles) a lane and trip."""
    blocks = cdiv(tile_elems // (16 // size_of(dtype)), 256)
    return {"items": (blocks, min(blocks, D["MG_FLATFIELD_BOUND_WALK"])), "planes": (1, 1)}


def _xy(grid, n):
    return grid[0], n, grid[1]


def _flat(total, cap):
    """A flat grid-stride loop of 256-thread workgroups over `total` indices."""
    blocks = cdiv(total, 256)
    return {"items": (blocks, min(blocks, cap)), "planes": (1, 1)}


def trips(walk) -> int:
    count, groups = walk
    return cdiv(count, groups)


# ---- the cases --------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    entry: str          # the C entry, as DESIGN.md's table names it
    loop: str           # "items" or "planes": the loop that must go round again
    name: str           # what tells the entry's cases apart
    shape: dict = field(hash=False)  # the grid function's arguments (and what else the test draws from)
    device_bytes: int = 0            # what the case keeps on the device at once: inputs, outputs, scratch

    @property
    def id(self):
        return f"{self.entry}-{self.loop}-{self.name}"


GRIDS = {"mg_depth_project": depth_project, "mg_depth_focus_totals": depth_focus_totals, "mg_depth_fuse": depth_fuse,
         "mg_affine_bilinear": affine_bilinear, "mg_bin_planes": bin_planes,
         "mg_percentile_histogram": percentile_histogram, "mg_unmix_planes": unmix_planes,
         "mg_skew_profiles": skew_profiles, "mg_render_overview": render_overview,
         "mg_roi_image_labels": roi_image_labels, "mg_flatfield_apply_stitch": stitch_grid,
         "mg_flatfield_apply_stitch_blend": stitch_grid, "mg_flatfield_apply_stitch_shift": stitch_grid,
         "mg_plane_minmax": plane_minmax, "mg_flatfield_max": flatfield_max, "mg_flatfield_bound": flatfield_bound,
         "mg_render_roi_montage": render_roi_montage, "mg_shading_apply_stitch": shading_apply,
         "mg_marker_table": marker_table, "mg_unpack_bits": unpack_bits}

MANY = MAX_Y + 65  # planes: one more than a grid's y would do; a few more, so that the second trip is not one plane


def _bytes(dtype, *dims):
    return int(np.prod(dims, dtype=np.int64)) * size_of(dtype)


def _bin_case(dtype, b):
    """Three planes 1037 wide (no side a multiple of the bin, rows at every alignment, a partial last run), as tall as
    puts the item count just past 2048 workgroups of 256 -- a fixed shape: the header's cap has no part in it."""
    n_t, w = 3, 1037
    hb = cdiv(2048 * 256 + 1, n_t * cdiv(w // b, bin_run(dtype, b)[1])) + 1
    h = hb * b + 1
    return Case("mg_bin_planes", "items", f"{dtype}-bin{b}", dict(dtype=dtype, b=b, n_t=n_t, h=h, w=w),
                _bytes(dtype, n_t, h, w) + _bytes("float32", n_t, h // b, w // b))


def _cases():
    out = []
    add = out.append
    # depth: 64 stacks leave 64 workgroups a plane of 66 (uint8) / 263 (float64) blocks of lanes
    for dtype in ("uint8", "float64"):
        add(Case("mg_depth_project", "items", dtype, dict(dtype=dtype, n=64, z=2, h=130, w=517),
                 _bytes(dtype, 64, 3, 130, 517)))
    add(Case("mg_depth_project", "planes", "uint8", dict(dtype="uint8", n=MANY, z=2, h=3, w=5), _bytes("uint8", MANY, 3, 3, 5)))
    add(Case("mg_depth_focus_totals", "items", "uint16", dict(dtype="uint16", n=64, z=4, h=130, w=517),
             _bytes("uint16", 64, 4, 130, 517)))
    add(Case("mg_depth_focus_totals", "planes", "uint8", dict(dtype="uint8", n=MANY, z=2, h=3, w=5),
             _bytes("uint8", MANY, 2, 3, 5) + 16 * MANY))
    add(Case("mg_depth_fuse", "planes", "uint8", dict(dtype="uint8", n=MANY, z=2, h=3, w=5, k=1), _bytes("uint8", MANY, 4, 3, 5)))
    # rotate: 512 planes leave 4 workgroups a plane of 5 (uint8) / 15 (float32) tiles
    for dtype in ("uint8", "float32"):
        add(Case("mg_affine_bilinear", "items", dtype, dict(dtype=dtype, n=512, h=130, w=71), 2 * _bytes(dtype, 512, 130, 71)))
    add(Case("mg_affine_bilinear", "planes", "float32", dict(dtype="float32", n=MANY, h=2, w=3),
             2 * _bytes("float32", MANY, 2, 3) + 16 * MANY))
    for dtype in ("uint8", "uint16", "float32", "float64"):
        for b in (2, 4, 8):
            add(_bin_case(dtype, b))
    # the ROI layout: 2100 windows of 3 x 3 pixels, one chunk each
    for dtype in ("uint8", "uint16", "float32", "float64"):
        add(Case("mg_percentile_histogram", "items", dtype, dict(dtype=dtype, units=2100, unit_len=9, channels=2),
                 _bytes(dtype, 2100, 2, 9)))
    side = 2897  # 2897^2 / 4 quads: the first odd square past MG_UNMIX_PLANES_WALK_PER_PLANE blocks of 256
    add(Case("mg_unmix_planes", "items", "uint8", dict(dtype="uint8", n_c=2, n_t=1, h=side, w=side),
             _bytes("uint8", 2, side, side) + _bytes("float32", side, side)))
    add(Case("mg_unmix_planes", "planes", "uint16", dict(dtype="uint16", n_c=2, n_t=MANY, h=1, w=4),
             _bytes("uint16", 2, MANY, 4) + _bytes("float32", 3, MANY, 4)))
    side = 2881  # 46 x 46 tiles of 64
    add(Case("mg_skew_profiles", "items", "uint8", dict(dtype="uint8", h=side, w=side, angles=(0.37, -10.0, 44.9)),
             _bytes("uint8", side, side)))
    # the rows the audit added
    side = 2049  # 2049 rows of 257 (uint8, level 0) runs; 513 rows of 257 runs (uint16, level 2: 4 x 4 blocks, two per run)
    for dtype, level in (("uint8", 0), ("uint16", 2)):
        add(Case("mg_render_overview", "items", f"{dtype}-level{level}", dict(dtype=dtype, level=level, n_t=1 << level, h=side, w=side),
                 _bytes(dtype, 1 << level, side, side) + 3 * (1 << level) * cdiv(side, 1 << level) ** 2))
    add(Case("mg_roi_image_labels", "items", "level0", dict(m=5300, n_t=1, roi_len=40, level=0, h=1000, w=1200),
             5300 * 1600 + 4 * 1000 * 1200))
    # 64 x 66 cells of 64 x 64 pixels: 17.3 M output pixels on 65536 workgroups of 256
    add(Case("mg_render_roi_montage", "items", "uint8", dict(dtype="uint8", m=4200, n_t=1, rows=64, cols=66, roi_len=64, level=0),
             _bytes("uint8", 4200, 64, 64) + 3 * 64 * 66 * 64 * 64))
    # one tall plane of few columns, the single-chip case: 1050 row groups of 2 rows on 1024 workgroups.  aligned: the
    # integer kernel of mg_flatfield.hip (overlap 0); plain and blend: k_stitch on two tiles with a seam (overlap 8)
    for name, overlap in (("aligned", 0), ("plain", 8), ("blend", 8), ("shift", 8)):
        add(Case("mg_flatfield_apply_stitch" + {"blend": "_blend", "shift": "_shift"}.get(name, ""), "items", name,
                 dict(dtype="uint16", n_planes=1, h_out=2100, w_out=64, overlap=overlap, blend=name == "blend"),
                 2 * _bytes("uint16", 2116, 72)))
    # pass 1 of the flat-field correction on the two paths the full-size tests do not take
    add(Case("mg_flatfield_max", "items", "int", dict(dtype="uint16", path="int", n_groups=2, tiles_per_group=1, tile_elems=2712 * 2712,
                                                      ty=2712, tx=2712), _bytes("uint16", 2, 2712, 2712)))
    add(Case("mg_flatfield_max", "items", "generic", dict(dtype="float32", path="generic", n_groups=64, tiles_per_group=1,
                                                          tile_elems=363 * 367, ty=363, tx=367), _bytes("float32", 65, 363, 367)))
    add(Case("mg_flatfield_max", "items", "fast", dict(dtype="uint16", path="fast", n_groups=64, tiles_per_group=1,
                                                       tile_elems=364 * 368, ty=364, tx=368), _bytes("uint16", 64, 364, 368) + 4 * 364 * 368))
    # one tile of 790020 vectors: more than 2 x 1536 x 256 for the lean kernel, more than 2048 x 256 for the bound's
    lean = dict(dtype="uint16", path="lean", n_groups=1, tiles_per_group=1, tile_elems=2052 * 3080, ty=2052, tx=3080)
    add(Case("mg_flatfield_max", "items", "lean", lean, _bytes("uint16", 4, 2052, 3080)))
    add(Case("mg_flatfield_bound", "items", "uint16", lean, _bytes("uint16", 4, 2052, 3080)))
    # 64 planes leave a plane's 34 groups of 8 rows 32 workgroups
    add(Case("mg_shading_apply_stitch", "items", "uint16", dict(dtype="uint16", n_planes=64, h_out=265, w_out=37),
             2 * _bytes("uint16", 64, 265, 37)))
    m = 2048 * 256 + 37  # (fixed shapes: a raised cap must fail the precondition, not move the case)
    add(Case("mg_marker_table", "items", "one_channel", dict(m=m, n_assays=3), m * (12 + 8 + 16 + 64)))
    bits = 4096 * 256 + 577
    add(Case("mg_unpack_bits", "items", "two_planes", dict(n_planes=2, n_bits=bits), 2 * (bits // 8 + 8) + 2 * bits))
    # 2049 x 2049 uint8: ragged rows, the general loop; 2052 x 4096 uint16: 1050624 whole vectors, four a lane and trip
    add(Case("mg_plane_minmax", "items", "uint8", dict(dtype="uint8", n=2, h=side, w=side), _bytes("uint8", 2, side, side)))
    add(Case("mg_plane_minmax", "items", "uint16-vectors", dict(dtype="uint16", n=2, h=2052, w=4096), _bytes("uint16", 2, 2052, 4096)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def cases_of(*entries):
    return [c for c in CASES if c.entry in entries]


def walk_of(case: Case):
    """(count, workgroups) of the loop the case is meant for."""
    return GRIDS[case.entry](**case.shape)[case.loop]


def require_second_trip(case: Case):
    """The precondition every GPU case asserts before its launch."""
    walk = walk_of(case)
    assert trips(walk) >= 2, f"{case.id}: {walk[0]} on {walk[1]} workgroups is one trip -- has a cap in the header been raised?"
    return walk
