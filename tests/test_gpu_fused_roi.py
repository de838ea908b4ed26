"""The ROI pass that corrects the non-searched channels itself (mg_roi_segment_reduce_raw) against the path that
corrects every channel as a full frame first (MG_FUSED_ROI=0) -- bit for bit -- and against the oracle's flat-field
function cropped at the windows.  The correction of the selected planes alone (mg_flatfield_apply_stitch_planes) and
the lazy completion of ``StackProcessor.image`` / ``.minmax`` are checked on the way."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ref_numeric as rn  # noqa: E402
from oracle import ref_pipeline as rp  # noqa: E402
from synth import draw_beads, vignette  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("roi", "fg", "bg", "sums", "counts")


def bead_stack(seed, T, C, h, w, extra=(), r=8, margin=13):
    """uint16 (T, C, h, w): noisy background, disks of radius ``r`` along all four borders (``margin`` from them: an
    L = 48 window around each is clipped), in the corners, a few inside and at ``extra``; per-channel values."""
    rng = np.random.default_rng(seed)
    ys, xs = [margin, h // 2, h - 1 - margin], [margin, w // 3, 2 * w // 3, w - 1 - margin]
    pos = [(y, x) for y in ys for x in xs] + [(h // 4 + 6, w // 2 + 3)] + list(extra)
    stack = np.empty((T, C, h, w), dtype=np.uint16)
    for t in range(T):
        for c in range(C):
            img = 100 + rng.poisson(20.0, size=(h, w)).astype(np.float64) + rng.normal(0, 3.0, size=(h, w))
            beads = draw_beads((h, w), pos, 2 * r, rng.integers(800, 4000, size=len(pos))).astype(np.float64)
            stack[t, c] = np.clip(np.rint(img + beads), 0, 65535).astype(np.uint16)
    return stack


def oracle_image(stack, flat, dark):
    """Mode P: every timepoint is its own assay with its own maxima (pipeline.py:18-24)."""
    with np.errstate(all="ignore"):
        return np.stack([rp.flatfield_correct(stack[t], flat, dark) for t in range(stack.shape[0])])


def to_host(out):
    return {k: out[k].cpu().numpy().copy() for k in KEYS} | {"beads": [np.asarray(b).copy() for b in out["beads"]]}


def run_processor(monkeypatch, fused, stack, flat, dark, search, **kw):
    from magnify_amd import hotpath as hp
    from magnify_amd.stack import StackProcessor

    monkeypatch.setenv("MG_FUSED_ROI", "1" if fused else "0")
    T, C, h, w = stack.shape
    hp.release_pool()
    proc = StackProcessor(T, C, h, w, num_iter=40000, min_bead_diameter=10, max_bead_diameter=24,
                          search_channels=search, mode="P", **kw)
    proc._image.view(torch.int16).fill_(-21555)  # what a channel nobody wrote would show
    d_flat = torch.from_numpy(flat).cuda() if isinstance(flat, np.ndarray) else flat
    out = to_host(proc(torch.from_numpy(stack).cuda(), d_flat, dark, seed=5))
    assert (proc._raw is not None) == fused and proc._deferred == fused
    if fused:  # the full frames of the other channels have not been written
        other = [c for c in range(C) if c not in search]
        assert (proc._image.view(torch.int16)[:, other] == -21555).all()
    out["image"] = proc.image.cpu().numpy().copy()
    out["minmax"] = proc.minmax.cpu().numpy().copy()
    assert not proc._deferred
    return out, proc.L


def check_pair(monkeypatch, stack, flat, dark, search, need_clip=True, **kw):
    got, L = run_processor(monkeypatch, True, stack, flat, dark, search, **kw)
    old, _ = run_processor(monkeypatch, False, stack, flat, dark, search, **kw)
    T, C, h, w = stack.shape
    for a, b in zip(got["beads"], old["beads"]):
        np.testing.assert_array_equal(a, b)
    for k in KEYS + ("image", "minmax"):
        np.testing.assert_array_equal(got[k], old[k], err_msg=k)
    # the oracle is the authority: full frames, and the ROI pixels of every channel cropped at the windows
    want = oracle_image(stack, flat, dark)
    np.testing.assert_array_equal(got["image"], want)
    sides, g = set(), 0
    for t, beads in enumerate(got["beads"]):
        for row, col, _ in beads:
            top, bottom, left, right = rn.bounding_box(int(col), int(row), L, w, h)
            np.testing.assert_array_equal(got["roi"][g][:, 0], want[t][:, top:bottom, left:right])
            sides |= {s for s, hit in (("top", top == 0), ("bottom", bottom == h), ("left", left == 0), ("right", right == w)) if hit}
            g += 1
    assert g == len(got["roi"])
    if need_clip:
        assert g >= 6 * T and sides == {"top", "bottom", "left", "right"}, (g, sides)
    return got, want, L


CASES = [  # T, C, (h, w), search channels, flat, dark
    (2, 2, (256, 320), (0,), "image", 100.0),
    (3, 4, (256, 320), (0,), "scalar", 100.0),
    (2, 4, (200, 262), (2,), "image", 90.5),   # width not a multiple of 8 (the general correction kernel), float dark
    (3, 2, (200, 262), (1,), "scalar", 90.0),
    (3, 4, (232, 232), (0,), "image", 0.0),
]


@pytest.mark.parametrize("T,C,shape,search,flat_kind,dark", CASES)
def test_fused_call_equals_full_correction(monkeypatch, T, C, shape, search, flat_kind, dark):
    h, w = shape
    stack = bead_stack(7 + T + C, T, C, h, w)
    flat = vignette((h, w)) if flat_kind == "image" else 0.9
    check_pair(monkeypatch, stack, flat, dark, search)


def test_fused_call_multi_search_and_plane_batch(monkeypatch):
    """Two searched channels (host-side de-duplication, segment_reduce) and detection in plane batches."""
    stack = bead_stack(31, 3, 4, 256, 320)
    check_pair(monkeypatch, stack, vignette((256, 320)), 100.0, (0, 2))
    check_pair(monkeypatch, stack, vignette((256, 320)), 100.0, (1,), plane_batch=2)


def test_exact_fallback_pixels_inside_windows(monkeypatch):
    """A flat image whose smallest value f0 sits under the brightest pixel AND under a patch with beads: there
    M1 / M2 = f0 and t / f0 * M1 / M2 lands within rounding of the integer t, so those pixels cannot take the fast
    product and go through the two exact divisions -- in the ROI kernel as in the correction pass."""
    T, C, h, w = 2, 4, 256, 320
    dark = 100.0
    stack = bead_stack(11, T, C, h, w, extra=[(96, 100), (96, 150), (140, 120)])
    flat = vignette((h, w))
    f0 = np.float32(flat.min() * 0.9)
    flat[60:180, 60:200] = f0
    stack[:, 0, 70, 70] = 60000  # M1 of every assay, under f0: M2 = M1 / f0
    got, want, L = check_pair(monkeypatch, stack, flat, dark, (0,))
    near = 0
    for t in range(T):
        tt = np.clip(stack[t].astype(np.float64) - dark, 0, None)
        m1 = tt.max()
        q = tt / flat
        v = q * m1 / q.max()  # the oracle's operations (ref_pipeline.flatfield_correct) before its cast
        close = (np.abs(v - np.rint(v)) < 1e-6) & (tt > 0)
        for row, col, _ in got["beads"][t]:
            top, bottom, left, right = rn.bounding_box(int(col), int(row), L, w, h)
            near += int(close[1:, top:bottom, left:right].sum())  # channels the ROI kernel corrects
    assert near > 0


def roi_fused_and_plain(stack, flat, dark, centres, L, searched=(0,)):
    """The two kernels side by side on chosen centres, without detection: (fused, plain, oracle image)."""
    from magnify_amd import hotpath as hp

    T, C, h, w = stack.shape
    d_stack = torch.from_numpy(stack).cuda()
    d_flat = torch.from_numpy(flat).cuda() if isinstance(flat, np.ndarray) else flat
    tiles = d_stack.view(T * C, 1, 1, 1, h, w)
    img, mm = hp.flatfield_stitch(tiles, 0, d_flat, dark, n_groups=T)
    plain = hp.roi_gather_reduce(img.view(T, C, 1, h, w), centres, L, None, disks=True)
    mask = sum(1 << c for c in searched)
    max2 = hp.flatfield_max(tiles, d_flat, dark, n_groups=T)
    img2 = torch.empty_like(img)
    img2.view(torch.int16).fill_(-21555)
    mm2 = torch.empty_like(mm)
    hp.flatfield_apply_planes(tiles, 0, d_flat, dark, max2, mask, C, out=img2, minmax_out=mm2)
    sel, rest = [c for c in range(C) if c in searched], [c for c in range(C) if c not in searched]
    v_img, v_img2 = img.view(torch.int16).view(T, C, h, w), img2.view(torch.int16).view(T, C, h, w)
    assert torch.equal(v_img2[:, sel], v_img[:, sel])
    assert (v_img2[:, rest] == -21555).all()

    def refuse():
        raise AssertionError("the fused kernel refused a call it is meant to take")

    raw = hp.RawChannels(d_stack, ((1 << C) - 1) & ~mask, d_flat, dark, max2, C, refuse)
    fused = hp.roi_gather_reduce(img2.view(T, C, 1, h, w), centres, L, None, disks=True, raw=raw)
    for k in KEYS:
        np.testing.assert_array_equal(fused[k].cpu().numpy(), plain[k].cpu().numpy(), err_msg=k)
    # the complementary selection completes the block and the min/max rows to what the full pass wrote
    hp.flatfield_apply_planes(tiles, 0, d_flat, dark, max2, raw.mask, C, out=img2, minmax_out=mm2, init_minmax=False)
    assert torch.equal(img2.view(torch.int16), img.view(torch.int16))
    np.testing.assert_array_equal(mm2.cpu().numpy(), mm.cpu().numpy())
    return fused, img.view(T, C, h, w).cpu().numpy()


def border_centres(h, w, T):
    pts = [(0, 0, 8), (0, w - 1, 8), (h - 1, 0, 9), (h - 1, w - 1, 8), (5, w // 2, 8), (h - 4, w // 2 + 1, 10),
           (h // 2, 3, 8), (h // 2 + 1, w - 6, 8), (h // 2, w // 2, 12), (h // 2 + 7, w // 2 + 9, 12), (h // 3, w // 3 + 1, 8)]
    return [np.asarray(pts[t:] + pts[:t], dtype=np.int32) for t in range(T)]


@pytest.mark.parametrize("flat_kind,dark", [("image", 100.0), ("scalar", 100.0), ("image", 33.25)])
def test_windows_clipped_at_every_border(flat_kind, dark):
    T, C, h, w, L = 2, 4, 180, 214, 40
    stack = bead_stack(3, T, C, h, w)
    flat = vignette((h, w)) if flat_kind == "image" else 0.8
    centres = border_centres(h, w, T)
    fused, _ = roi_fused_and_plain(stack, flat, dark, centres, L, searched=(1,))
    want = oracle_image(stack, flat, dark)
    g = 0
    for t in range(T):
        for row, col, _ in centres[t]:
            top, bottom, left, right = rn.bounding_box(int(col), int(row), L, w, h)
            np.testing.assert_array_equal(fused["roi"][g].cpu().numpy()[:, 0], want[t][:, top:bottom, left:right])
            g += 1


@pytest.mark.parametrize("bad", ["inf", "zero"])
def test_out_of_range_flat_values(bad):
    """Flat values outside the reciprocal's range (0, inf) inside windows: those lanes take the reference's own
    operations.  A zero makes the assay's M2 infinite or NaN (every pixel of it is then 0, as in the reference)."""
    T, C, h, w, L = 2, 2, 180, 214, 40
    stack = bead_stack(5, T, C, h, w)
    flat = vignette((h, w))
    flat[h // 2 - 3 : h // 2 + 3, w // 2 - 5 : w // 2 + 4] = np.inf
    flat[2, 3] = np.inf
    if bad == "zero":
        flat[h // 2 + 8, w // 2 + 8] = 0.0
    centres = border_centres(h, w, T)
    fused, img = roi_fused_and_plain(stack, flat, 100.0, centres, L)
    if bad == "inf":  # (a NaN's cast is the platform's in NumPy: the zero case is compared with the full pass only)
        want = oracle_image(stack, flat, 100.0)
        np.testing.assert_array_equal(img, want)
        assert (want[:, :, h // 2, w // 2] == 0).all() and want.max() > 0


def test_refused_call_completes_and_gathers(monkeypatch):
    """A case the fused kernel does not take (odd window length): the channels are corrected by the correction pass
    (``complete``) and the plain kernel runs -- same results."""
    from magnify_amd import hotpath as hp

    T, C, h, w, L = 2, 2, 180, 214, 41
    stack = bead_stack(9, T, C, h, w)
    flat = vignette((h, w))
    d_stack, d_flat = torch.from_numpy(stack).cuda(), torch.from_numpy(flat).cuda()
    tiles = d_stack.view(T * C, 1, 1, 1, h, w)
    img, mm = hp.flatfield_stitch(tiles, 0, d_flat, 100.0, n_groups=T)
    centres = border_centres(h, w, T)
    plain = hp.roi_gather_reduce(img.view(T, C, 1, h, w), centres, L, None, disks=True)
    max2 = hp.flatfield_max(tiles, d_flat, 100.0, n_groups=T)
    img2, mm2 = torch.empty_like(img), torch.empty_like(mm)
    img2.view(torch.int16).zero_()
    hp.flatfield_apply_planes(tiles, 0, d_flat, 100.0, max2, 1, C, out=img2, minmax_out=mm2)
    called = []

    def complete():
        called.append(1)
        hp.flatfield_apply_planes(tiles, 0, d_flat, 100.0, max2, 2, C, out=img2, minmax_out=mm2, init_minmax=False)

    raw = hp.RawChannels(d_stack, 2, d_flat, 100.0, max2, C, complete)
    got = hp.roi_gather_reduce(img2.view(T, C, 1, h, w), centres, L, None, disks=True, raw=raw)
    assert called == [1]
    for k in KEYS:
        np.testing.assert_array_equal(got[k].cpu().numpy(), plain[k].cpu().numpy(), err_msg=k)
