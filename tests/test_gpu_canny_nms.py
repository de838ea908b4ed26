"""mg_canny_nms alone, through the C ABI, on torch buffers: the kernel takes the blurred uint8 image and explicit
integer thresholds, so no other stage is involved.  Every plane is compared with the oracle:

  weak   == (oracle.ref_opencv.canny_nms(dx, dy, low, high) != 1)
  strong == (... == 2)
  the three orientation planes == the kernel's integer rule, restated in NumPy below, at EVERY pixel (the edge-stage
  tests check them off the sector boundaries only)
  the bits of every plane's words at and beyond h * w stay zero
  every in-image word is written: the buffers are handed over full of ones.

Shapes come from the strip geometry (mg_canny_nms_strips): widths around one strip, over several strips, with and
without whole bitmap words per row, one width the strip walk does not take; heights below the stencil's three rows
and around one wave's and one workgroup's rows.  Images: noise, a constant, and 8 x 8-block plateaus / ramps /
checkerboards, whose equal neighbouring magnitudes and on-axis / on-diagonal gradients sit exactly on the > / >=
asymmetry and on the sector boundaries.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_opencv as rcv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def nat():
    from magnify_amd import _native, hotpath

    hotpath.require_gpu()
    return _native


def _geometry(nat, w):
    s, rw, r = C.c_int(0), C.c_int(0), C.c_int(0)
    nat.check(nat.lib().mg_canny_nms_strips(w, C.byref(s), C.byref(rw), C.byref(r)), "mg_canny_nms_strips")
    return s.value, rw.value, r.value


# ---- images ------------------------------------------------------------------------------------------------------
IMAGE_KINDS = ("noise", "constant", "ramp_h", "ramp_v", "diag_down", "diag_up", "checker")


def _image(kind, h, w, seed):
    by, bx = np.mgrid[0:h, 0:w] // 8  # 8 x 8 blocks of equal value
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "constant":
        return np.full((h, w), 77, np.uint8)
    if kind == "ramp_h":
        return ((bx * 17) % 256).astype(np.uint8)
    if kind == "ramp_v":
        return ((by * 17) % 256).astype(np.uint8)
    if kind == "diag_down":
        return (((bx + by) * 13) % 256).astype(np.uint8)
    if kind == "diag_up":
        return (((bx - by) * 13) % 256).astype(np.uint8)
    assert kind == "checker"
    return np.where((bx + by) & 1, 200, 40).astype(np.uint8)


# ---- thresholds ----------------------------------------------------------------------------------------------------
THRESHOLD_KINDS = ("zero", "equal", "above_all", "quantiles")


def _thresholds(kind, mag):
    """(low, high) as the kernel takes them (squared-magnitude integers)."""
    if kind == "zero":
        return 0, 0
    nonzero = mag[mag > 0]  # (the block images are flat nearly everywhere)
    if kind == "equal":
        v = int(np.median(nonzero)) if nonzero.size else 0
        return v, v
    if kind == "above_all":  # no strong bit
        return (int(np.quantile(nonzero, 0.25)) if nonzero.size else 0), int(mag.max()) + 1
    assert kind == "quantiles"
    g = np.sqrt(mag.astype(np.float32))
    lo, hi = np.quantile(g, [0.1, 0.9])
    return rcv.canny_thresholds(float(lo), float(hi))


# ---- oracle ----------------------------------------------------------------------------------------------------
def _orientation_planes(dx, dy):
    """The kernel's integer rule for the planes c0, c1, c2 of bin = 4 c1 + 2 c0 + c2, at every pixel."""
    a, b = np.abs(dx), np.abs(dy)
    neg = (dx ^ dy) < 0
    le, ge = b <= a, b >= a
    c1 = neg
    c0 = np.where(neg, le, ge)
    lowq = np.where(neg, le, ~ge)
    s = np.where(lowq, a + b, b - a)
    c2 = neg ^ (s * s > 2 * a * a)
    return c0, c1, c2


def _unpack(words, n_bits):
    """(bits [0, n_bits), the bits behind them) of one plane's uint32 words."""
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    return bits[:n_bits], bits[n_bits:]


def _run_and_check(nat, imgs, thresholds):
    """One mg_canny_nms call over the planes `imgs` with per-plane (low, high); every plane against the oracle."""
    p, h, w = imgs.shape
    n = h * w
    in_words = (n + 31) // 32
    words = in_words + 3  # (one spare word is required; the others watch the tail)
    blur = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    thr = torch.from_numpy(np.asarray(thresholds, np.int32).reshape(p, 2)).cuda()

    def buffer(*shape):  # in-image words full of ones: every one of them has to be written (or cleared and ORed)
        t = torch.zeros(shape + (words,), dtype=torch.int32, device="cuda")
        t[..., :in_words] = -1
        return t

    weak, strong, cls = buffer(p), buffer(p), buffer(p, 3)
    nat.check(nat.lib().mg_canny_nms(blur.data_ptr(), p, h, w, thr.data_ptr(), weak.data_ptr(), strong.data_ptr(),
                                     cls.data_ptr(), words, None), "mg_canny_nms")
    torch.cuda.synchronize()
    weak, strong, cls = (t.cpu().numpy().view(np.uint32) for t in (weak, strong, cls))
    for k in range(p):
        dx, dy = (g.astype(np.int64) for g in rcv.scharr(imgs[k]))
        low, high = (int(v) for v in thresholds[k])
        nms = rcv.canny_nms(dx, dy, low, high)
        what = f"plane {k} of {h} x {w}, thresholds {low}, {high}"
        for name, got, want in (("weak", weak[k], nms != 1), ("strong", strong[k], nms == 2)) + tuple(
                (f"c{j}", cls[k, j], c) for j, c in enumerate(_orientation_planes(dx, dy))):
            bits, tail = _unpack(got, n)
            np.testing.assert_array_equal(bits.reshape(h, w), want.astype(np.uint8), err_msg=f"{name}, {what}")
            assert not tail.any(), f"{name}: bits beyond h * w, {what}"
    return weak, strong


def _planes(h, w, first):
    """Three planes of different image kinds, with different threshold kinds; `first` rotates through both lists."""
    kinds = [IMAGE_KINDS[(first + k) % len(IMAGE_KINDS)] for k in range(3)]
    imgs = np.stack([_image(kind, h, w, 100 * first + k) for k, kind in enumerate(kinds)])
    thresholds = []
    for k in range(3):
        dx, dy = (g.astype(np.int64) for g in rcv.scharr(imgs[k]))
        thresholds.append(_thresholds(THRESHOLD_KINDS[(first + 2 * k) % len(THRESHOLD_KINDS)], dx * dx + dy * dy))
    return imgs, thresholds


def _widths(nat):
    s = _geometry(nat, 4)[0]
    return {"four": 4, "below_strip": s - 4, "strip": s, "above_strip": s + 4, "three_strips_whole_words": 2 * s + 32,
            "partial_words": s + s // 2 + 12, "not_dwords": s + 3}


def test_strip_geometry(nat):
    s, rw, r = _geometry(nat, 4)
    assert s % 32 == 0 and s >= 32, "strips are whole bitmap words"
    assert rw >= 1 and r % rw == 0
    w = _widths(nat)
    assert w["three_strips_whole_words"] % 32 == 0 and w["three_strips_whole_words"] > 2 * s
    assert w["partial_words"] % 4 == 0 and w["partial_words"] % 32 != 0
    assert w["above_strip"] % 4 == 0 and w["below_strip"] % 4 == 0 and w["not_dwords"] % 4 != 0


@pytest.mark.parametrize("width", ["four", "below_strip", "strip", "above_strip", "three_strips_whole_words",
                                   "partial_words", "not_dwords"])
def test_nms_shapes(nat, width):
    w = _widths(nat)[width]
    _, rw, r = _geometry(nat, 4)
    for i, h in enumerate((1, 2, 3, rw - 1, rw + 1, r - 1, r + 1, 2 * r + 3)):
        imgs, thresholds = _planes(h, w, first=i + w // 4)
        _run_and_check(nat, imgs, thresholds)


@pytest.mark.parametrize("image", IMAGE_KINDS)
def test_nms_images_and_thresholds(nat, image):
    """Every image kind under every threshold kind, across a strip border and a wave border."""
    s, rw, _ = _geometry(nat, 4)
    h, w = rw + 9, s + 32
    img = _image(image, h, w, 5)
    dx, dy = (g.astype(np.int64) for g in rcv.scharr(img))
    mag = dx * dx + dy * dy
    thresholds = [_thresholds(kind, mag) for kind in THRESHOLD_KINDS]
    weak, strong = _run_and_check(nat, np.stack([img] * len(thresholds)), thresholds)
    if image == "constant":
        assert not weak.any() and not strong.any(), "a constant plane sets no bit"
    assert not strong[THRESHOLD_KINDS.index("above_all")].any(), "high above every magnitude: no strong bit"
