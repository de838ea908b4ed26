"""What the plane filters share (csrc/mg_planes.h, ``magnify_amd._dataset``): one table of bad and empty blocks applied to
the six entries and to mg_background_scratch_bytes, the page view through the three components, and the rounds of the
tile fill in mg_depth_fuse."""

import numpy as np
import pytest
import torch

import depth_ref as dr

pytestmark = pytest.mark.gpu

N, Z, H, W = 2, 3, 8, 9  # the block of the table: 2 planes (or stacks of 3 slices) of 8 x 9 pixels
CANARY = 9


@pytest.fixture(scope="module")
def mg():
    import magnify_amd

    magnify_amd.hotpath = __import__("magnify_amd.hotpath", fromlist=["x"])
    magnify_amd.hotpath.require_gpu()
    return magnify_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the shared check -------------------------------------------------------------------------------------------------

REFUSED = [dict(dtype=99), dict(n=-1), dict(h=-1), dict(w=-1), dict(h=(1 << 30) + 1), dict(w=(1 << 20) + 1)]
MISALIGNED = [dict(dtype=dt, **{which: 1}) for dt in ("u16", "f32") for which in ("src_off", "dst_off")]
EMPTY = [dict(n=0), dict(h=0), dict(w=0)]


def test_one_table_of_blocks_for_every_entry(mg):
    nat = mg.hotpath.nat
    lib, s = nat.lib(), mg.hotpath._stream()
    codes = {"u8": nat.MG_U8, "u16": nat.MG_U16, "f32": nat.MG_F32, "f64": nat.MG_F64}
    room = N * Z * H * W * 8 + 16  # bytes: the block in any dtype, and one byte off
    src = torch.zeros(room, dtype=torch.uint8, device="cuda")
    outs = {name: torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
            for name in ("dst", "index", "totals", "counts", "votes", "scratch")}
    p = {name: t.data_ptr() for name, t in outs.items()}
    bright = nat.DEFINES["MG_OUTLIER_BRIGHT"]

    # every entry as f(dtype, n, h, w, source, destination); the other arguments are good ones.  The host function comes
    # first: were the shared check ever to let a size through, the test ends there, before a kernel is given that size
    entries = {
        "mg_background_scratch_bytes": lambda dt, n, h, w, a, b: lib.mg_background_scratch_bytes(dt, n, h, w, 4),
        "mg_depth_project": lambda dt, n, h, w, a, b: lib.mg_depth_project(a, b, dt, n, Z, h, w, nat.DEFINES["MG_DEPTH_MAX"],
                                                                           0, s),
        "mg_depth_focus_totals": lambda dt, n, h, w, a, b: lib.mg_depth_focus_totals(a, dt, n, Z, h, w, p["totals"], s),
        "mg_depth_fuse": lambda dt, n, h, w, a, b: lib.mg_depth_fuse(a, dt, n, Z, h, w, 1, b, p["index"], s),
        "mg_despeckle_planes": lambda dt, n, h, w, a, b: lib.mg_despeckle_planes(a, b, dt, n, h, w, 1, bright, 1.0, 0,
                                                                                 p["counts"], s),
        "mg_outlier_votes": lambda dt, n, h, w, a, b: lib.mg_outlier_votes(a, dt, n, h, w, 1, bright, 1.0, p["votes"], s),
        "mg_background_planes": lambda dt, n, h, w, a, b: lib.mg_background_planes(
            a, 0, b, dt, n, h, w, 4, nat.DEFINES["MG_BACKGROUND_SUBTRACT"], p["scratch"], room, s),
    }
    no_dst = ("mg_depth_focus_totals", "mg_outlier_votes", "mg_background_scratch_bytes")
    assert sorted(entries) == sorted(e for e in nat.PROTOTYPES if e.startswith(("mg_depth_", "mg_despeckle_", "mg_outlier_",
                                                                                 "mg_background_")))

    def call(name, dtype="u8", n=N, h=H, w=W, src_off=0, dst_off=0):
        return entries[name](codes.get(dtype, dtype), n, h, w, src.data_ptr() + src_off, p["dst"] + dst_off)

    for name in entries:
        for bad in REFUSED:
            assert call(name, **bad) == -1, (name, bad)
        for bad in MISALIGNED:
            if name == "mg_background_scratch_bytes" or ("dst_off" in bad and name in no_dst):
                continue  # (the entry has no such pointer)
            assert call(name, **bad) == -1, (name, bad)
        for empty in EMPTY:
            assert call(name, **empty) == 0, (name, empty)
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert (t.cpu().numpy() == CANARY).all(), name
    # validity comes before emptiness: an empty block with a bad dtype, size or pointer is refused all the same
    for name in entries:
        assert call(name, dtype=99, n=0) == -1 and call(name, n=0, w=(1 << 20) + 1) == -1, name
        if name != "mg_background_scratch_bytes":
            assert call(name, dtype="u16", h=0, src_off=1) == -1, name
    # ... and the table's block itself is a good one
    for name in entries:
        assert call(name) == (2 * N * H * W if name == "mg_background_scratch_bytes" else 0), name
    torch.cuda.synchronize()


# ---- the page view through the components ------------------------------------------------------------------------------

def test_components_equal_the_functions_on_the_transposed_planes(mg):
    rng = np.random.default_rng(77)
    despeckle, background, depth = mg.despeckle, mg.background, mg.depth
    image = rng.integers(0, 4096, size=(2, 2, 8, 9)).astype(np.uint16)  # (channel, time, y, x)
    image[0, 1, 3, 4] = image[1, 0, 6, 1] = 60000
    stack = rng.integers(0, 4096, size=(2, 2, 3, 8, 9)).astype(np.uint16)  # (channel, time, depth, y, x)
    coords = {"channel": ["bf", "cy5"], "time": [10, 20]}

    def sources(data, base, dims, var, pages):
        """``data`` (dimensions ``base``) with its dimensions in the order ``dims``: as a DataArray with pages (y, x) and
        as a Dataset whose variable ``var`` has the pages ``pages``."""
        arr = mg.DataArray(np.ascontiguousarray(data.transpose([base.index(d) for d in dims])), dims, coords=coords,
                           name="pixels", attrs={"name": "assay"})
        named = tuple({"y": pages[0], "x": pages[1]}.get(d, d) for d in dims)
        ds = mg.Dataset({var: mg.DataArray(arr.data, named, attrs={"unit": "adu"})}, coords=coords, attrs={"name": "assay"})
        return arr, ds

    def values(res, var):
        return res.values if isinstance(res, mg.DataArray) else res[var].values

    # remove_outliers: lead in the variable's own order (time, channel)
    base, dims = ("channel", "time", "y", "x"), ("time", "y", "channel", "x")
    planes = dev(image.transpose(1, 0, 2, 3))
    want, counts = despeckle.remove_outliers(planes, 5000.0)
    assert int(counts.sum().item()) == 2
    want = want.cpu().numpy().transpose(1, 0, 2, 3)  # back to (channel, time, y, x)
    for src in sources(image, base, dims, "tile", ("tile_y", "tile_x")):
        got = despeckle.remove_outliers_component(src, 5000.0)
        assert type(got) is type(src) and got.attrs == {"name": "assay", "despeckle_replaced": 2}
        np.testing.assert_array_equal(values(got, "tile"), want.transpose(1, 2, 0, 3))
    # subtract_background: channel first, whatever the variable's order
    planes = dev(image)
    want = background.subtract(planes, 2).cpu().numpy()
    for src in sources(image, base, dims, "image", ("im_y", "im_x")):
        got = background.subtract_background(src, 2)
        assert type(got) is type(src) and got.attrs == {"name": "assay", "background_radius": 2}
        np.testing.assert_array_equal(values(got, "image"), want.transpose(1, 2, 0, 3))
    # project_depth: the depth dimension between lead and pages
    dims = ("depth", "time", "y", "channel", "x")
    want = depth.project(dev(stack.transpose(1, 0, 2, 3, 4)), "mean").cpu().numpy()  # (time, channel, y, x)
    for src in sources(stack, ("channel", "time", "depth", "y", "x"), dims, "tile", ("tile_y", "tile_x")):
        got = depth.project_depth(src, "mean")
        assert type(got) is type(src) and got.attrs == {"name": "assay", "depth_method": "mean"}
        tile = got if isinstance(got, mg.DataArray) else got["tile"]
        assert tile.dims[:2] == ("time", "channel") and "depth" not in tile.dims
        np.testing.assert_array_equal(tile.values, want)


# ---- the rounds of the tile fill ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 15])
@pytest.mark.parametrize("dtype", [np.uint16, np.float64])
def test_fuse_fill_in_whole_and_in_broken_rounds(mg, dtype, k):
    """A thread of mg_depth_fuse fills the padded tile in rounds of eight loads, 2048 pixels a workgroup: (32 + 2k + 2)^2
    pixels are 1296 at k = 1 (a part of one round) and 4096 at k = 15 (two whole rounds)."""
    tile = mg.depth.TILE
    assert (tile + 2 * k + 2) ** 2 % 2048 == (0 if k == 15 else 1296)
    rng = np.random.default_rng(5 + k)
    block = dr.random_stack(rng, dtype, (2, 3, tile + 5, 2 * tile + 7))
    image, index = mg.depth.fuse(dev(block), 2 * k + 1)
    want = dr.over_stacks(dr.fuse, block, k)
    assert np.array_equal(index.cpu().numpy(), np.stack([w[1] for w in want]))
    assert dr.same(image.cpu().numpy(), np.stack([w[0] for w in want]))
