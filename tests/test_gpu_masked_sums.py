"""mg_masked_sums on the GPU: sums and counts of gathered windows under fg / bg masks in every form the window kernels
read -- one mask for all timepoints, one per timepoint, a view expanded along time, a slice of a larger tensor --
against NumPy, exactly.  Float pixels are integers below 2^20, so every float64 partial sum is exact and the comparison
does not depend on the order of the additions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, C, T = 3, 2, 3
LENGTHS = (1, 7, 17)  # 17^2 = 289 > 256: the second trip of the thread loop; 7, 17: windows that are not 16-byte aligned
DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
FORMS = ("one", "per_time", "expanded", "slice")


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def pixels(dtype, L, rng):
    hi = 256 if dtype == np.uint8 else 65536 if dtype == np.uint16 else 1 << 20
    return rng.integers(0, hi, size=(M, C, T, L, L)).astype(dtype)


def masks(form, L, rng):
    """(what goes to the device, the (M, T, L, L) boolean masks it stands for)"""
    n_t = T if form == "per_time" else 1
    m = rng.random((M, n_t, L, L)) < 0.5
    m[1] = False  # one marker with an empty mask
    return (m[:, 0] if form == "one" else m), np.broadcast_to(m, (M, T, L, L))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LENGTHS)
def test_sums_and_counts_equal_numpy(hp, L, dtype, form):
    import torch

    rng = np.random.default_rng(1000 * L + 10 * DTYPES.index(dtype) + FORMS.index(form))
    roi = pixels(dtype, L, rng)
    (fg_in, fg), (bg_in, bg) = masks(form, L, rng), masks(form, L, rng)

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if form == "expanded":
            return t.expand(M, T, L, L)
        if form == "slice":  # the masks are the middle of a larger tensor: marker stride 3 L^2
            big = torch.zeros((M, 3, L, L), dtype=torch.bool, device="cuda")
            big[:, 1] = t[:, 0]
            return big[:, 1:2]
        return t

    d_fg, d_bg = dev(fg_in), dev(bg_in)
    if form in ("expanded", "slice"):  # read where they lie: the pointer is handed on, nothing is copied
        for d in (d_fg, d_bg):
            view, sm, st = hp._mask_view("test", d, M, T, L)
            assert view.data_ptr() == d.data_ptr() and st == 0
            assert sm == (3 * L * L if form == "slice" else L * L)
    sums, counts = hp.masked_sums(torch.from_numpy(roi).cuda(), d_fg, d_bg)

    wide = roi.astype(np.int64 if np.issubdtype(dtype, np.integer) else np.float64)
    want = np.stack([(wide * fg[:, None]).sum((-1, -2)), (wide * bg[:, None]).sum((-1, -2))], axis=-1)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int32
    np.testing.assert_array_equal(sums.cpu().numpy(), want.astype(np.float64))
    want_counts = np.stack([fg.sum((-1, -2)), bg.sum((-1, -2))], axis=-1)  # (M, T, 2)
    if form == "one":
        assert tuple(counts.shape) == (M, 2)
        np.testing.assert_array_equal(counts.cpu().numpy(), want_counts[:, 0])
    else:
        n_tm = d_fg.shape[1]
        assert tuple(counts.shape) == (M, n_tm, 2)
        np.testing.assert_array_equal(counts.cpu().numpy(), want_counts[:, :n_tm])
    assert not want_counts[1].any() and not want[1].any()  # the empty masks were among them
