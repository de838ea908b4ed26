"""The window kernels of mg_roi.hip -- k_roi_u16_even, k_roi<T, ACC> -- and the small kernels around them
(k_window_order, k_counts_to_offsets, k_marker_table) against tests/roi_ref.py, the pass restated in NumPy, at the
shapes where they take another path or reach a limit: every output of every call, every call twice for the same bits.

Masks, counts, roi pixels and integer sums are compared for equality.  A float sum is compared with math.fsum of the
float64 values: |got - fsum| <= n 2^-52 sum|v| over the n masked pixels, the float64 recursive-summation bound
(n - 1) 2^-53 sum|v| with a factor of two in hand -- it holds for any order the kernel adds in.

Every test asserts that its inputs still produce the condition it was built for (an odd `left`, lane 63 loading, 97
disks in a window, a second scan batch, a second rank trip, the generic kernel reached)."""
import numpy as np
import pytest

import roi_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OUTPUTS = ("roi", "fg", "bg", "sums", "counts")
NBR_CAP = 96                  # disks of one window that build_disk_masks draws row-parallel
SCAN_BATCH = 256 * 8          # beads per trip of its scan
ORDER_TRIP = 8 * 256          # markers k_window_order ranks per trip
MG_EINVAL = -1


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- inputs -----------------------------------------------------------------------------------------------------------
def int_images(rng, dtype, shape):
    """Full-range integer pixels; the first plane holds the type's maximum everywhere."""
    images = rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    images[0, 0, 0] = np.iinfo(dtype).max
    return images


def float_images(rng, dtype, shape):
    """Mixed signs, magnitudes 1e-3 .. 1e6."""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 6, shape)).astype(dtype)


def make_images(rng, dtype, shape):
    return float_images(rng, dtype, shape) if np.dtype(dtype).kind == "f" else int_images(rng, dtype, shape)


def edge_beads(rng, h, w, L, extra=15, r_hi=14):
    """Beads whose windows are clamped at every corner and border, touch the bottom and right borders unclamped, start
    at even and at odd columns, with centres outside the image, plus `extra` random ones."""
    cy, cx = h // 2, w // 2
    centres = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (cy, 0), (cy, w - 1), (0, cx), (h - 1, cx), (cy, cx),
               (cy, cx + 1), (cy + 1, cx), (-3, cx + 30), (cy + 30, w + 4), (h - L + L // 2, w - L + L // 2)]
    centres += list(zip(rng.integers(0, h, extra), rng.integers(0, w, extra)))
    beads = np.array([(y, x, r) for (y, x), r in zip(centres, rng.integers(2, r_hi, len(centres)))], dtype=np.int64)
    beads[11:13, 2] = 2  # the two outside: their disks stay outside, their windows (of any length) see background
    return beads


def assert_placements(win, L, h, w):
    """The placements test a asks for, read from bounding_box's windows (n, 2) [top, left]."""
    top, left = win[:, 0], win[:, 1]
    if w > L:
        assert (left % 2 == 0).any() and (left % 2 == 1).any(), "no even or no odd left"
    for at_top in (top == 0, top + L == h):
        for at_left in (left == 0, left + L == w):
            assert (at_top & at_left).any(), "a corner is missing"
    if h > L + 1:
        assert ((top > 0) & (top + L < h)).any()
    if w > L + 1:
        assert ((left > 0) & (left + L < w)).any()


def fast_kernel_takes(images, L):
    """roi_u16_even_ok of mg_roi.hip for the plain pass, restated: uint16, an even window of at most 126, even width
    and assay stride, dword indices below 2^31, the image on a dword (torch's own output blocks are aligned)."""
    _, c, t, h, w = images.shape
    return (images.dtype == torch.uint16 and L % 2 == 0 and L <= 126 and w % 2 == 0 and (c * t * h * w) % 2 == 0
            and h * w < 2 ** 31 and images.data_ptr() % 4 == 0)


# ---- calls and comparison ---------------------------------------------------------------------------------------------
def padded(assays):
    cap = max(len(b) for b in assays) + 3
    tab = np.zeros((len(assays), cap, 3), dtype=np.int32)
    for a, b in enumerate(assays):
        tab[a, : len(b)] = b
    return tab


def table_max_r(assays):
    return max(2, max((int(np.asarray(b)[:, 2].max()) for b in assays if len(b)), default=2))


def call_pass(hp, images, assays, L, mode, max_r, time_major=False):
    """One call of the pass through hotpath.roi_gather_reduce: mode "disk" (padded device tables, explicit max_r),
    "compact" (host tables; max_r is the table's largest radius) or a label map (A, h, w)."""
    if isinstance(mode, str) and mode == "disk":
        kw = dict(disks=True, device_tables=(dev(padded(assays)), [len(b) for b in assays], max_r), time_major=time_major)
        res = hp.roi_gather_reduce(images, None, L, None, **kw)
    elif isinstance(mode, str) and mode == "compact":
        assert max_r == table_max_r(assays)
        res = hp.roi_gather_reduce(images, assays, L, None, disks=True, time_major=time_major)
    else:
        res = hp.roi_gather_reduce(images, assays, L, dev(mode))
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in OUTPUTS}


def same_bits(a, b):
    for name in OUTPUTS:
        assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), f"{name} differs between two calls"


def compare(got, ref):
    for name in ("fg", "bg", "counts", "roi"):
        assert got[name].dtype == ref[name].dtype
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    assert got["sums"].dtype == np.float64
    if ref["sums"].dtype.kind == "i":
        np.testing.assert_array_equal(got["sums"], ref["sums"].astype(np.float64), err_msg="sums")
    else:
        n = ref["counts"].astype(np.float64)[:, None, None, :]
        bound = n * 2.0 ** -52 * ref["abs_sums"]
        err = np.abs(got["sums"] - ref["sums"])
        assert (err <= bound).all(), f"float sums: error / bound up to {np.nanmax(err / np.where(bound > 0, bound, np.nan))}"


def check(hp, images, assays, L, mode="disk", max_r=None, time_major=False, to_device=None, fast=None):
    """Reference, two calls, all five outputs.  `fast`: which window kernel the shape has to reach."""
    max_r = table_max_r(assays) if max_r is None else max_r
    ref = roi_ref.roi_ref(images, assays, L, max_r, time_major=time_major)
    d_images = (to_device or dev)(images)
    layout = d_images if not time_major else d_images.transpose(1, 2)
    assert fast_kernel_takes(layout, L) == fast
    mode = ref["labels"] if mode == "label" else mode
    got = call_pass(hp, d_images, assays, L, mode, max_r, time_major)
    same_bits(got, call_pass(hp, d_images, assays, L, mode, max_r, time_major))
    compare(got, ref)
    return ref


# ---- a. the fast kernel's geometry ------------------------------------------------------------------------------------
PLANES = [(1, 1, False), (3, 1, False), (2, 2, False), (2, 2, True), (5, 1, False), (3, 3, False), (3, 3, True)]


@pytest.mark.parametrize("n_c,n_t,time_major", PLANES)
@pytest.mark.parametrize("L", [2, 32, 34, 64, 96, 126])
def test_fast_kernel_geometry(hp, L, n_c, n_t, time_major):
    rng = np.random.default_rng(100 + L)
    h, w = 130, 132
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=4)]
    images = int_images(rng, np.uint16, (2, n_t, n_c, h, w) if time_major else (2, n_c, n_t, h, w))
    ref = check(hp, images, assays, L, time_major=time_major, fast=True)
    assert_placements(ref["windows"], L, h, w)
    if L == 126:  # 63 active lanes and an odd start: lane 63 loads the row's extra dword
        assert (ref["windows"][:, 1] % 2 == 1).any()
    assert ref["fg"].any() and ref["bg"].any() and (ref["labels"] == -2).any()


@pytest.mark.parametrize("mode", ["disk", "label"])
def test_fast_kernel_window_is_the_image(hp, mode):
    rng = np.random.default_rng(126)
    h = w = L = 126
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=2)]
    ref = check(hp, int_images(rng, np.uint16, (2, 3, 1, h, w)), assays, L, mode=mode, fast=True)
    assert not ref["windows"].any()


@pytest.mark.parametrize("n_c", [1, 5])
@pytest.mark.parametrize("L", [2, 126])
def test_fast_kernel_label_mode(hp, L, n_c):
    rng = np.random.default_rng(200 + L)
    h, w = 130, 132
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=4)]
    ref = check(hp, int_images(rng, np.uint16, (2, n_c, 1, h, w)), assays, L, mode="label", fast=True)
    assert_placements(ref["windows"], L, h, w)
    assert ref["fg"].any() and ref["bg"].any()


# ---- b. sums over the whole 16-bit range ------------------------------------------------------------------------------
def test_full_range_sums(hp):
    rng = np.random.default_rng(300)
    h = w = 200
    L = 126
    images = rng.integers(0, 65536, size=(2, 2, 1, h, w)).astype(np.uint16)
    images[:, 0] = 65535
    assays = [np.array([[100, 100, 1]]), np.array([[100, 100, 91]])]  # nothing drawn at all / one disk over the whole window
    ref = check(hp, images, assays, L, max_r=91, fast=True)
    assert ref["bg"][0].all() and not ref["fg"][0].any() and ref["sums"][0, 0, 0, 1] == 126 * 126 * 65535 == 1040433660
    assert ref["fg"][1].all() and not ref["bg"][1].any() and ref["sums"][1, 0, 0, 0] == 1040433660
    assert ref["sums"][:, 1].max() > 1 << 24


# ---- c. the generic kernel and what sends a call to it ------------------------------------------------------------------
def test_generic_kernel_u16_window_lengths(hp):
    rng = np.random.default_rng(400)
    h, w = 140, 150
    for L in (33, 127, 128):
        assays = [edge_beads(rng, h, w, L, extra=3), edge_beads(rng, h, w, L, extra=0)]
        ref = check(hp, int_images(rng, np.uint16, (2, 2, 1, h, w)), assays, L, fast=False)
        assert_placements(ref["windows"], L, h, w)


def test_generic_kernel_u16_odd_width(hp):
    rng = np.random.default_rng(401)
    h, w, L = 100, 131, 40
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=3)]
    ref = check(hp, int_images(rng, np.uint16, (2, 3, 2, h, w)), assays, L, fast=False)
    assert_placements(ref["windows"], L, h, w)


def test_generic_kernel_u16_image_on_a_halfword(hp):
    """The same shape on and off a dword: only the image's base address decides."""
    rng = np.random.default_rng(402)
    h, w, L = 100, 132, 40
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=3)]
    images = int_images(rng, np.uint16, (2, 3, 2, h, w))

    def one_element_in(a):
        view = dev(np.concatenate([[0], a.ravel()]).astype(a.dtype))[1:].view(a.shape)
        assert view.is_contiguous() and view.data_ptr() % 4 == 2
        return view

    check(hp, images, assays, L, to_device=one_element_in, fast=False)
    check(hp, images, assays, L, fast=True)


@pytest.mark.parametrize("L", [40, 41])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_generic_kernel_dtypes(hp, dtype, L):
    rng = np.random.default_rng(410 + L)
    h, w = 100, 132
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=3)]
    ref = check(hp, make_images(rng, dtype, (2, 2, 2, h, w)), assays, L, fast=False)
    assert_placements(ref["windows"], L, h, w)
    assert ref["fg"].any() and ref["bg"].any()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32, np.float64])
def test_generic_kernel_label_mode(hp, dtype):
    rng = np.random.default_rng(420)
    h, w, L = 100, 132, 33
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=3)]
    check(hp, make_images(rng, dtype, (2, 2, 2, h, w)), assays, L, mode="label", fast=False)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_generic_kernel_time_major(hp, dtype):
    rng = np.random.default_rng(430)
    t, c, h, w, L = 3, 2, 100, 132, 40
    assays = [edge_beads(rng, h, w, L), edge_beads(rng, h, w, L, extra=3)]
    check(hp, make_images(rng, dtype, (2, t, c, h, w)), assays, L, time_major=True, fast=False)


# ---- the C entry points themselves ------------------------------------------------------------------------------------
def sentinel(shape, dtype):
    return dev(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xA5, dtype=np.uint8).view(dtype).reshape(shape))


def native_pass(images, assays, L, max_r=None, labels=None, null=(), time_major=False):
    """mg_roi_segment_reduce (compact tables) or, with a label map, mg_roi_gather_reduce_batched, into outputs
    pre-filled with a byte pattern; the outputs named in `null` are passed as NULL.  Returns (status, outputs)."""
    from magnify_amd import _native as nat
    from magnify_amd import hotpath

    A, c, t, h, w = images.shape if not time_major else images.transpose(1, 2).shape
    beads = np.concatenate([np.asarray(b, dtype=np.int32).reshape(-1, 3) for b in assays])
    off = np.concatenate([[0], np.cumsum([len(b) for b in assays])]).astype(np.int32)
    m, side = len(beads), max(L, 1)
    np_dtype = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32, torch.float64: np.float64}[images.dtype]
    outs = {"roi": sentinel((m, c, t, side, side), np_dtype), "fg": sentinel((m, side, side), np.uint8),
            "bg": sentinel((m, side, side), np.uint8), "sums": sentinel((m, c, t, 2), np.float64),
            "counts": sentinel((m, 2), np.int32)}
    ptrs = [0 if name in null else outs[name].data_ptr() for name in OUTPUTS]
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream
    d_beads = dev(beads)
    code = nat.dtype_code(images.dtype)
    if labels is None:
        d_off, tab = dev(off), hotpath._halfwidth_table(max_r, "cuda")
        rc = lib.mg_roi_segment_reduce(images.data_ptr(), code, c * t * h * w, c, t, h, w, int(time_major), d_beads.data_ptr(),
                                       0, d_off.data_ptr(), A, m, 0, L, tab.data_ptr(), max_r, *ptrs, stream)
    else:
        d_assay = dev(np.repeat(np.arange(A, dtype=np.int32), np.diff(off)))
        d_local = dev(np.concatenate([np.arange(n, dtype=np.int32) for n in np.diff(off)]))
        d_labels = dev(np.asarray(labels, dtype=np.int32))
        rc = lib.mg_roi_gather_reduce_batched(images.data_ptr(), code, c * t * h * w, c, t, h, w, d_beads.data_ptr(),
                                              d_assay.data_ptr(), d_local.data_ptr(), m, L, d_labels.data_ptr(), *ptrs, stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def assert_untouched(outs):
    for name, v in outs.items():
        assert (v.view(np.uint8) == 0xA5).all(), f"{name} was written"


# ---- d. the largest windows ---------------------------------------------------------------------------------------------
def test_largest_label_window(hp):
    rng = np.random.default_rng(500)
    h = w = 250
    L = 244  # 244^2 = 59 536 bytes of flags: the last length below the 60 000-byte bound
    assays = [edge_beads(rng, h, w, L, extra=0, r_hi=30)[:9], edge_beads(rng, h, w, L, extra=0, r_hi=30)[9:]]
    ref = check(hp, int_images(rng, np.uint8, (2, 1, 2, h, w)), assays, L, mode="label", fast=False)
    assert ref["fg"].any() and ref["bg"].any() and len(np.unique(ref["windows"], axis=0)) > 4


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_largest_disk_window(hp, dtype):
    rng = np.random.default_rng(501)
    h, w = 210, 214
    L = 206  # 206^2 flags + 3 x 206 x 7 mask words = 59 740 bytes
    assays = [edge_beads(rng, h, w, L, extra=0, r_hi=30)[:9], edge_beads(rng, h, w, L, extra=0, r_hi=30)[9:]]
    ref = check(hp, make_images(rng, dtype, (2, 2, 1, h, w)), assays, L, fast=False)
    assert ref["fg"].any() and ref["bg"].any() and len(np.unique(ref["windows"], axis=0)) > 4


def test_windows_that_are_refused(hp):
    rng = np.random.default_rng(502)
    beads = [np.array([[20, 20, 5], [30, 25, 6]])]

    def refused(h, w, L, label_mode):
        images = dev(int_images(rng, np.uint8, (1, 1, 1, h, w)))
        labels = roi_ref.ownership(beads[0], h, w, 6)[None] if label_mode else None
        rc, outs = native_pass(images, beads, L, max_r=6, labels=labels)
        assert rc == MG_EINVAL
        assert_untouched(outs)

    refused(250, 250, 245, True)   # 245^2 = 60 025 bytes
    refused(210, 214, 207, False)  # 207^2 + 3 x 207 x 7 words = 60 237 bytes
    for label_mode in (False, True):
        refused(40, 50, 45, label_mode)  # L > h
        refused(50, 40, 45, label_mode)  # L > w
        refused(40, 50, 0, label_mode)
        refused(40, 50, -2, label_mode)


# ---- e. the disk table's edges ------------------------------------------------------------------------------------------
def reaching(beads, top, left, L, max_r):
    """Disks the scan of build_disk_masks collects for a window: drawn radii whose bounding box meets it."""
    y, x, r = np.asarray(beads).T
    return int(((r >= 2) & (r <= max_r) & (y + r >= top) & (y - r < top + L) & (x + r >= left) & (x - r < left + L)).sum())


def test_disks_per_window_at_the_row_parallel_limit(hp):
    rng = np.random.default_rng(600)
    h, w, L = 160, 200, 40
    grid = [(y, x, 2 + (k % 2)) for k, (y, x) in enumerate((y, x) for y in range(22, 60, 4) for x in range(22, 60, 4))]
    far = [(130, 150, 5), (140, 170, 4), (120, 190, 6), (150, 120, 3), (100, 160, 7)]
    assays = [np.array([(40, 40, 6)] + grid[:n] + far) for n in (NBR_CAP - 1, NBR_CAP)]
    ref = check(hp, int_images(rng, np.uint16, (2, 2, 1, h, w)), assays, L, fast=True)
    m0 = len(assays[0])
    for a, first in enumerate((0, m0)):
        top, left = ref["windows"][first]
        assert (top, left) == (20, 20) and reaching(assays[a], top, left, L, 7) == NBR_CAP + a
        per_window = [reaching(assays[a], t, l, L, 7) for t, l in ref["windows"][first:first + len(assays[a])]]
        assert max(per_window) == NBR_CAP + a
        assert 0 < ref["counts"][first, 1] < L * L and ref["fg"][first:first + len(assays[a])].any()
    assert (ref["labels"] == -2).any()


def test_disk_table_edges(hp):
    rng = np.random.default_rng(601)
    h, w, L, max_r = 160, 200, 40, 12
    top, left = 60, 80  # the window of marker 0
    tangent = [(top - 1 - 6, 85, 6), (top - 6, 95, 6), (top + L - 1 + 6, 105, 6), (top + L + 6, 115, 6),
               (65, left - 1 - 6, 6), (75, left - 6, 6), (85, left + L - 1 + 6, 6), (95, left + L + 6, 6)]
    twins = [(30, 30, 7), (30, 30, 7)]
    radii = [(130, 40, -1), (130, 60, 0), (130, 80, 1), (130, 100, max_r), (133, 104, max_r + 1), (128, 98, 1), (20, 150, 9),
             (22, 152, 0), (18, 149, max_r + 1)]
    assay = np.array([(80, 100, 5)] + tangent + twins + radii)
    assays = [assay, edge_beads(rng, h, w, L)]
    for dtype in (np.uint16, np.float32):
        ref = check(hp, make_images(rng, dtype, (2, 2, 1, h, w)), assays, L, max_r=max_r, fast=dtype == np.uint16)
        assert tuple(ref["windows"][0]) == (top, left)
        y, x, r = assay[1:9].T
        assert [int(v) for v in (y + r)[:2] - top] == [-1, 0] and [int(v) for v in (y - r)[2:4] - top - L] == [-1, 0]
        assert [int(v) for v in (x + r)[4:6] - left] == [-1, 0] and [int(v) for v in (x - r)[6:8] - left - L] == [-1, 0]
        # the disks that touch the window leave one contour pixel each out of its background; the others none
        inside = ref["labels"][0][top:top + L, left:left + L]
        assert sorted(np.unique(inside[inside > 0])) == [2, 3, 6, 7]
        assert ref["counts"][9, 0] == 0 and ref["counts"][10, 0] == 0 and (ref["labels"][0][30, 23:38] == -2).all()
        excluded = np.nonzero((assay[:, 2] < 2) | (assay[:, 2] > max_r))[0]
        assert sorted(set(assay[excluded, 2])) == [-1, 0, 1, max_r + 1] and not ref["counts"][excluded, 0].any()
        assert ref["counts"][14, 0] > 0 and ref["counts"][17, 0] > 0 and not np.isin(ref["labels"][0], excluded).any()
        assert not (ref["labels"][0] == -2)[116:, :].any()  # the excluded disks over (130, 100, max_r) contest nothing


def test_bead_table_longer_than_a_scan_batch(hp, monkeypatch):
    rng = np.random.default_rng(602)
    h, w, L, n = 160, 200, 8, 2100
    beads = np.column_stack([rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(2, 5, n)])
    assays = [beads, np.empty((0, 3), dtype=np.int64)]
    images = int_images(rng, np.uint16, (2, 1, 1, h, w))
    assert n > SCAN_BATCH
    orders = []
    inner = hp._window_order
    monkeypatch.setattr(hp, "_window_order", lambda *a, **k: orders.append(inner(*a, **k)) or orders[-1])
    ref = check(hp, images, assays, L, fast=True)
    assert orders == [None, None]  # below _ROI_ORDER_MIN: the windows are visited in table order
    monkeypatch.setattr(hp, "_ROI_ORDER_MIN", 1)
    check(hp, images, assays, L, fast=True)
    assert len(orders) == 4 and all(o is not None and o.numel() == n for o in orders[2:])
    want = roi_ref.window_order_ref(assays, n, np.zeros(n))
    np.testing.assert_array_equal(orders[3].cpu().numpy(), want)
    assert (want != np.arange(n)).any()
    # the beads of the second batch decide masks of markers of the first
    cut = beads.copy()
    cut[SCAN_BATCH:, 2] = 0
    short = roi_ref.roi_ref(images, [cut, assays[1]], L, 4)
    assert (short["fg"][:SCAN_BATCH] != ref["fg"][:SCAN_BATCH]).any() and (short["bg"][:SCAN_BATCH] != ref["bg"][:SCAN_BATCH]).any()


# ---- f. any output may be NULL ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,L,label_mode,fast", [(np.uint16, 34, False, True), (np.uint16, 34, True, True),
                                                     (np.float32, 33, False, False), (np.uint8, 34, True, False)])
def test_each_output_may_be_null(hp, dtype, L, label_mode, fast):
    rng = np.random.default_rng(700)
    h, w = 60, 64
    assays = [edge_beads(rng, h, w, L, extra=3), edge_beads(rng, h, w, L, extra=0)]
    images = make_images(rng, dtype, (2, 3, 2, h, w))
    ref = roi_ref.roi_ref(images, assays, L, 13)
    d_images = dev(images)
    assert fast_kernel_takes(d_images, L) == fast
    kw = dict(max_r=13, labels=ref["labels"] if label_mode else None)
    rc, full = native_pass(d_images, assays, L, **kw)
    assert rc == 0
    compare(full, ref)
    for name in OUTPUTS:
        rc, part = native_pass(d_images, assays, L, null=(name,), **kw)
        assert rc == 0
        assert_untouched({name: part[name]})
        for other in OUTPUTS:
            if other != name:
                assert part[other].tobytes() == full[other].tobytes(), f"{other} with {name} NULL"


# ---- g. the small kernels -----------------------------------------------------------------------------------------------
def native_tables(assays, compact):
    """(d_beads, bead_stride, d_offsets, offsets) of compact or padded bead tables."""
    off = np.concatenate([[0], np.cumsum([len(b) for b in assays])]).astype(np.int32)
    if compact:
        return dev(np.concatenate([np.asarray(b, dtype=np.int32).reshape(-1, 3) for b in assays])), 0, dev(off), off
    tab = padded(assays)
    return dev(tab), tab.shape[1], dev(off), off


@pytest.mark.parametrize("compact", [False, True])
def test_window_order(hp, compact):
    from magnify_amd import _native as nat

    rng = np.random.default_rng(800)
    sizes = [1, 2047, 2048, 2049, 5000, 8192, 8193]
    rows = np.concatenate([np.arange(-70, 330), [-(1 << 31), (1 << 20) - 1, 1 << 20, (1 << 20) + 64, (1 << 31) - 1]])
    cols = np.concatenate([np.arange(-3, 40), [-(1 << 31), (1 << 17) - 1, 1 << 17, (1 << 17) + 5, (1 << 31) - 1]])
    assays = [np.column_stack([rng.choice(rows, n), rng.choice(cols, n), np.full(n, 3)]) for n in sizes]
    d_beads, stride, d_off, off = native_tables(assays, compact)
    total = int(off[-1])
    assert max(sizes[:-1]) == roi_ref.ORDER_CAP and sizes[-1] == roi_ref.ORDER_CAP + 1 and sizes[3] > ORDER_TRIP
    for b in assays[1:]:
        assert (b[:, 0] < 0).any() and (b[:, 0] >= 1 << 20).any() and (b[:, 1] < 0).any() and (b[:, 1] >= 1 << 17).any()
    # a bound at and beyond the table's end, in the middle of an assay's second trip, and in the assay too long to be
    # ordered: cut below the limit and exactly to it
    bounds = [total, total + 100, int(off[4]) + 2500, int(off[6]) + 4000, int(off[6]) + roi_ref.ORDER_CAP]
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream
    for m in bounds:
        before = np.full(total + 108, -1, dtype=np.int32)
        want = roi_ref.window_order_ref(assays, m, before)
        got = []
        for _ in range(2):
            order = dev(before)
            assert lib.mg_roi_window_order(d_beads.data_ptr(), stride, d_off.data_ptr(), len(assays), m, order.data_ptr(), stream) == 0
            got.append(order.cpu().numpy())
        np.testing.assert_array_equal(got[0], got[1])
        np.testing.assert_array_equal(got[0], want)
        assert (want[min(m, total):] == -1).all()
        for a, n in enumerate(sizes):  # many equal keys, and an order that is not the table's
            part = want[off[a]:min(off[a + 1], m)]
            if len(part) > 50:
                sorts = len(part) <= roi_ref.ORDER_CAP
                assert (part != np.arange(off[a], off[a] + len(part))).any() == sorts
    key = (np.clip(assays[4][:, 0], 0, (1 << 20) - 1) >> 6 << 17) | np.clip(assays[4][:, 1], 0, (1 << 17) - 1)
    assert len(np.unique(key)) < len(key) // 4


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2500])
def test_counts_to_offsets(hp, n):
    from magnify_amd import _native as nat

    rng = np.random.default_rng(810 + n)
    cap = 25
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream
    for counts in ([[-3], [0], [99], [7]] if n == 1 else [rng.integers(-5, 40, n)]):
        counts = np.asarray(counts, dtype=np.int32)
        if n > 1:
            assert (counts < 0).any() and (counts == 0).any() and (counts > cap).any() and (counts == cap).any()
        want = roi_ref.counts_to_offsets_ref(counts, cap)
        if n > 1024:  # the second trip starts from what the first one summed
            assert want[1024] > 0 and want[-1] > want[1024]
        d_off = dev(np.full(n + 5, -1, dtype=np.int32))
        assert lib.mg_counts_to_offsets(dev(counts).data_ptr(), n, cap, d_off.data_ptr(), stream) == 0
        got = d_off.cpu().numpy()
        np.testing.assert_array_equal(got[: n + 1], want)
        assert (got[n + 1:] == -1).all()


@pytest.mark.parametrize("compact", [False, True])
def test_marker_table_at_every_time_index(hp, compact):
    from magnify_amd import _native as nat

    rng = np.random.default_rng(820)
    n_c, n_t, assay_offset = 2, 3, 4
    assays = [np.column_stack([rng.integers(-5, 300, (n, 2)), rng.integers(2, 20, n)]) for n in (5, 0, 7, 300)]
    d_beads, stride, d_off, off = native_tables(assays, compact)
    total = int(off[-1])
    counts = rng.integers(0, 10000, (total, 2)).astype(np.int32)
    sums = rng.integers(0, 1 << 40, (total, n_c, n_t, 2)).astype(np.float64)
    lib, stream = nat.lib(), torch.cuda.current_stream().cuda_stream
    d_counts, d_sums, tables = dev(counts), dev(sums), []
    for t_index in range(n_t):
        table = dev(np.full((total + 3, 6 + 2 * n_c), -7.0))
        assert lib.mg_marker_table(d_beads.data_ptr(), stride, d_off.data_ptr(), len(assays), total + 3, assay_offset,
                                   d_counts.data_ptr(), d_sums.data_ptr(), n_c, n_t, t_index, table.data_ptr(), stream) == 0
        got = table.cpu().numpy()
        np.testing.assert_array_equal(got[:total], roi_ref.marker_table_ref(assays, assay_offset, counts, sums, t_index))
        assert (got[total:] == -7.0).all()
        tables.append(got)
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])
    for bad in (-1, n_t):
        assert lib.mg_marker_table(d_beads.data_ptr(), stride, d_off.data_ptr(), len(assays), total, assay_offset,
                                   d_counts.data_ptr(), d_sums.data_ptr(), n_c, n_t, bad, 0, stream) == MG_EINVAL
