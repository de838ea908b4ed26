"""Shading model on the MI355X (DESIGN.md §4 "shading"): the HIP downsample, DCT, ALM iterations and the whole fit
against the float64 oracle tests/ref_shading.py, determinism, and shading_correct -> stitch through the Pipeline."""
import numpy as np
import pytest
import torch
from scipy.fft import dctn, idctn

import ref_shading as rs
from oracle import ref_pipeline as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import magnify_amd

    magnify_amd.hotpath.require_gpu()
    return magnify_amd


def _cast(tiles_u16, dtype):
    if dtype == np.uint8:
        return (tiles_u16 >> 4).clip(0, 255).astype(np.uint8)
    return tiles_u16.astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("shape", [(256, 256), (300, 211)])
@pytest.mark.parametrize("w", [128, 100])
def test_downsample_matches_oracle(mg, dtype, shape, w):
    rng = np.random.default_rng(3)
    tiles = _cast(rng.integers(0, 65536, size=(3,) + shape).astype(np.uint16), dtype)
    got = mg.shading.working_stack(torch.from_numpy(tiles).cuda(), w).cpu().numpy()
    want = rs.downsample(tiles, w)
    np.testing.assert_allclose(got, want, rtol=1e-6)


@pytest.mark.parametrize("w", [128, 64, 100])
def test_dct_matches_scipy(mg, w):
    rng = np.random.default_rng(w)
    d = torch.from_numpy(rng.random((2, w, w)).astype(np.float32)).cuda()
    f = mg.shading._Fitter(d)
    x = rng.standard_normal((w, w))
    xin = torch.from_numpy(x).cuda()
    out = torch.empty_like(xin)
    # the forward-error bound of test_gpu_shading_stages.py (two chained FMA dot products of w terms, and the table's
    # own error on each side), plus 1e-13 for scipy's transform, in place of the first guess of 1e-5
    c, cb = np.abs(f.cos_table()), rs.cos_table_bound(w)
    for inverse, ref in ((0, dctn), (1, idctn)):
        f._call("mg_shading_dct2", xin.data_ptr(), out.data_ptr(), inverse)
        left, lb = (c.T, cb.T) if inverse else (c, cb)
        bound = (2.1 * w * 2.0**-53 * (left @ np.abs(x) @ left.T) + lb @ np.abs(x) @ left.T + left @ np.abs(x) @ lb.T
                 + 1e-13)
        assert bound.max() < 1e-10  # (the table term grows with the argument, up to about pi w)
        assert np.all(np.abs(out.cpu().numpy() - ref(x, norm="ortho")) <= bound)


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize("k", [1, 10])
def test_alm_iterations_match_oracle(mg, k):
    tiles, _, _ = rs.synthetic_stack(n=8, size=256, seed=2)
    d = mg.shading.working_stack(torch.from_numpy(tiles).cuda(), 128)
    f = mg.shading._Fitter(d)
    dh = d.cpu().numpy().astype(np.float64)
    c = rs.Consts(dh)
    assert abs(f.norm2 - c.norm2) <= 1e-9 * c.norm2 and abs(f.lam_f - c.lam_f) <= 1e-9 * c.lam_f
    st = rs.State(c)
    for _ in range(k):
        rs.alm_step(st, dh, np.ones_like(dh), c)
    f.begin()
    f.iterate(k)
    done, it = f.flags()
    assert it == k and not done
    w = 128
    for region, dtype, shape, want in ((mg.shading._E, torch.float32, (8, w, w), st.E),
                                       (mg.shading._Y, torch.float32, (8, w, w), st.Y),
                                       (mg.shading._FW, torch.float64, (w, w), st.F_w),
                                       (mg.shading._AOFF, torch.float64, (w, w), st.A_off),
                                       (mg.shading._COEFF, torch.float64, (8,), st.coeff)):
        got = f.view(region, dtype, shape).cpu().numpy().astype(np.float64)
        assert _rel(got, want) <= 1e-4, (region, _rel(got, want))
    b1 = float(f.view(mg.shading._SC, torch.float64, (32,))[mg.shading._SC_B1])
    assert abs(b1 - st.B1_off) <= 1e-4 * max(abs(st.B1_off), 1e-3)


def test_fit_matches_oracle_and_is_deterministic(mg):
    tiles, _, _ = rs.synthetic_stack(n=16, size=256, seed=4)
    model = mg.shading.fit(tiles)
    flat, dark, its = rs.fit(tiles)
    assert len(model.iterations) == len(its)
    assert all(abs(a - b) <= 2 for a, b in zip(model.iterations, its)), (model.iterations, its)
    assert np.abs(model.flatfield.cpu().numpy() - flat).max() <= 2e-3
    assert np.abs(model.darkfield.cpu().numpy() - dark).max() <= 1e-3 * tiles.mean()
    again = mg.shading.fit(torch.from_numpy(tiles).cuda())
    assert torch.equal(again.flatfield, model.flatfield) and torch.equal(again.darkfield, model.darkfield)
    assert again.iterations == model.iterations


def test_fit_recovers_known_fields(mg):
    tiles, flat, dark = rs.synthetic_stack(seed=0)
    model = mg.shading.fit(tiles)
    ef, ed, eoff = rs.recovery(model.flatfield.cpu().numpy(), model.darkfield.cpu().numpy(), flat, dark)
    assert ef <= 0.03 and ed <= 0.35 and eoff <= 1.2  # the oracle's bounds (test_cpu_shading.py)
    nodark = mg.shading.fit(tiles, get_darkfield=False)
    assert not nodark.darkfield.any()


def _assay(tiles, mg):
    return mg.DataArray(tiles, ("channel", "time", "tile_row", "tile_col", "tile_y", "tile_x"))


def _two_channel_tiles(grid, t, size=128):
    """(2, t, rows, cols, size, size) u16 with a different vignette per channel; the last timepoint's corners are
    65535, which saturates after the division by a flat below 1 there (kept out of the training tiles: a spike of
    that size dominates the smoothness constant and the fit's flat collapses -- the oracle's too)."""
    rows, cols = grid
    out = []
    for ch, strength in enumerate((0.3, 0.6)):
        st, _, _ = rs.synthetic_stack(n=rows * cols * t, size=size, seed=10 + ch, strength=strength)
        out.append(st.reshape(t, rows, cols, size, size))
    tiles = np.stack(out)
    tiles[:, -1, :, :, :4, :4] = 65535
    return tiles


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("grid, overlap, timepoints", [((2, 2), 0, (0,)), ((2, 2), 102, (0,)), ((1, 1), 0, (0, 1))])
def test_shading_correct_then_stitch_is_exact(mg, dtype, grid, overlap, timepoints):
    tiles = _cast(_two_channel_tiles(grid, 3), dtype)
    pipe = mg.Pipeline("read")
    pipe.add_pipe("standardize_format")
    pipe.add_pipe("shading_correct", timepoints=timepoints)
    pipe.add_pipe("stitch", overlap=overlap)
    xp = pipe(_assay(tiles, mg))
    lazy = xp.data_vars["tile"].raw
    flats, darks = lazy.flatfield.cpu().numpy(), lazy.darkfield.cpu().numpy()
    assert flats.shape == (2, 128, 128) and not np.array_equal(flats[0], flats[1])
    corrected = np.stack([rs.apply(tiles[c], flats[c], darks[c]) for c in range(2)])
    want = rp.stitch(corrected, overlap)
    got = xp.image.values
    assert got.dtype == tiles.dtype
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(xp.tile.values, corrected)
    if dtype == np.uint16:
        assert (corrected == 65535).any()  # the last timepoint's corners (cropped away by overlap 102)
    assert set(xp.data_vars) == {"tile", "image"}


def test_fields_ignore_other_timepoints(mg):
    tiles = _two_channel_tiles((2, 2), 2, size=96)
    fields = []
    for t1 in (tiles, np.concatenate([tiles[:, :1], tiles[:, 1:] // 3 + 7], axis=1)):
        xp = mg.components.get("standardize_format")()(_assay(t1, mg))
        xp = mg.components.get("shading_correct")()(xp)
        fields.append((xp.data_vars["tile"].raw.flatfield.cpu(), xp.data_vars["tile"].raw.darkfield.cpu()))
    assert torch.equal(fields[0][0], fields[1][0]) and torch.equal(fields[0][1], fields[1][1])


def test_model_apply(mg):
    tiles, _, _ = rs.synthetic_stack(n=6, size=128, seed=5)
    model = mg.shading.fit(tiles)
    got = model.apply(tiles).cpu().numpy()
    np.testing.assert_array_equal(got, rs.apply(tiles, model.flatfield.cpu().numpy(), model.darkfield.cpu().numpy()))
