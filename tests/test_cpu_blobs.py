"""The blob oracle alone (tests/blobs_ref.py) held to scipy.ndimage directly, the planes of
tests/blobs_cases.py held to what the GPU tests assume of them, and the host side of ``magnify_amd.blobs``: registration,
constants and every refusal that has to come before a device call.  The kernels are held to the oracle by
tests/test_gpu_blobs.py."""
import inspect

import numpy as np
import pytest

pytest.importorskip("scipy")

import scipy.ndimage as ndi  # noqa: E402

import blobs_cases as bc  # noqa: E402
import blobs_ref as br  # noqa: E402


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("p", [0.05, 0.41, 0.59, 0.95])
def test_oracle_numbers_in_raster_order_and_counts_what_numpy_counts(p, connectivity):
    rng = np.random.default_rng(int(p * 100) + connectivity)
    for h, w in [(1, 1), (1, 37), (37, 1), (33, 65), (70, 131)]:
        on = rng.random((h, w)) < p
        labels, k, stats = br.label_mask(on, connectivity)
        lab, n = ndi.label(on, br.S8 if connectivity == 8 else br.S4)
        assert k == n and np.array_equal(labels, lab.astype(np.int64) - 1) and (labels[~on] == -1).all()
        # raster-first: walking the plane in raster order meets the numbers 0, 1, 2, ... in order
        seen = labels.reshape(-1)[labels.reshape(-1) >= 0]
        _, first_at = np.unique(seen, return_index=True)
        assert np.all(np.diff(first_at) > 0)
        assert np.array_equal(stats[:, 0], np.bincount(seen, minlength=k)) and stats[:, 0].sum() == on.sum()
        for i, sl in enumerate(ndi.find_objects(lab)):
            ys, xs = np.nonzero(lab == i + 1)
            assert stats[i].tolist() == [len(ys), ys.sum(), xs.sum(), ys.min(), xs.min(), ys.max(), xs.max(),
                                         (ys * w + xs).min()]
            assert (sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1) == (ys.min(), ys.max(), xs.min(), xs.max())


def test_oracle_threshold_polarity_and_nan():
    plane = np.array([[0.5, 1.5, np.nan], [np.inf, -np.inf, 1.0]])
    assert br.on_mask(plane, 1.0).tolist() == [[False, True, False], [True, False, False]]
    assert br.on_mask(plane, 1.0, below=True).tolist() == [[True, False, False], [False, True, False]]


@pytest.mark.parametrize("seed", range(4))
def test_oracle_fill_holes_is_scipy(seed):
    on = np.random.default_rng(seed).random((40, 70)) < 0.59
    want = ndi.binary_fill_holes(on)
    assert np.array_equal(br.fill_holes(on.astype(np.uint8)), want)
    # the rule the kernel is given: the 4-connected components of the complement that touch no side of the frame
    labels, k, stats = br.label_mask(~on, 4)
    inside = (stats[:, 3] > 0) & (stats[:, 4] > 0) & (stats[:, 5] < 39) & (stats[:, 6] < 69)
    assert np.array_equal(on | ((labels >= 0) & inside[np.maximum(labels, 0)]), want)


def test_oracle_select_and_table():
    on = np.zeros((20, 30), dtype=bool)
    on[0:3, 0:3] = True      # touches top and left, area 9
    on[5:9, 5:12] = True     # inside, area 28
    on[12, 20] = True        # inside, area 1
    on[17:20, 27:30] = True  # touches bottom and right
    labels, k, stats = br.label_mask(on, 8)
    out, kept, table = br.select(labels, stats, min_area=2, clear_border=True)
    assert k == 4 and kept[:, 0].tolist() == [28] and table.tolist() == [[7, 8, 3]]
    assert out[6, 6] == 0 and out[0, 0] == -2 and out[12, 20] == -2 and out[19, 29] == -2 and out[10, 0] == -1
    out, kept, table = br.select(labels, stats, max_area=9)
    assert kept[:, 0].tolist() == [9, 1, 9] and sorted(set(out.reshape(-1).tolist())) == [-2, -1, 0, 1, 2]
    # the nearest integer to sqrt(area / pi), in integers
    for a in list(range(1, 4000)) + [10 ** 6, 2 ** 31 - 1]:
        r = br.radius(a)
        assert 355 * (2 * r - 1) ** 2 <= 452 * a < 355 * (2 * r + 1) ** 2
        assert abs(r - np.sqrt(a * 113 / 355)) <= 0.5 + 1e-9


def test_structured_planes_are_what_the_gpu_tests_assume():
    h, w = bc.structured_shape(32, 64)
    m, path = bc.spiral(h, w)
    assert path[0] == (0, 0) and m.sum() == len(path)
    for c in (4, 8):
        assert br.label_mask(m, c)[1] == 1
        cut = m.copy()
        cut[path[len(path) // 2]] = False
        assert br.label_mask(cut, c)[1] == 2
    # through all nine tiles
    assert {(y // 32, x // 64) for y, x in path} >= {(a, b) for a in range(3) for b in range(3)}
    assert br.label_mask(bc.comb(h, w), 4)[1] == 1
    us, n = bc.nested_us(h, w)
    assert n > 10 and br.label_mask(us, 8)[1] == n and br.label_mask(us, 4)[1] == n
    cb = bc.checkerboard(h, w)
    assert br.label_mask(cb, 8)[1] == 1 and br.label_mask(cb, 4)[1] == (h * w + 1) // 2
    d = bc.pair(h, w, (31, 63), (32, 64))
    a = bc.pair(h, w, (31, 64), (32, 63))
    assert [br.label_mask(x, c)[1] for x in (d, a) for c in (8, 4)] == [1, 2, 1, 2]
    assert br.label_mask(bc.corners_and_tile_corner(h, w, 32, 64), 4)[1] == 5


@pytest.mark.parametrize("seed", range(8))
def test_scene_has_twelve_blobs(seed):
    plane, masks, ring = bc.scene(seed)
    assert plane.shape == bc.SCENE_SHAPE and plane.dtype == np.uint16 and len(masks) == bc.SCENE_BLOBS
    for fill in (False, True):
        want = br.component(plane[None, None], fill=fill, min_area=20)
        assert len(want["table"]) == 12 and want["area"].min() >= 20 and not want["clipped"].any()
        assert want["blob_components"] == 12  # no component below 20 pixels: the selection rejects nothing here
    hollow, filled = br.component(plane[None, None]), br.component(plane[None, None], fill=True)
    at = bc.mark_of(hollow["labels"], ring)  # (marks are in raster order of their first pixels, not in drawing order)
    assert at == bc.mark_of(filled["labels"], ring) and (ring <= masks[bc.SCENE_RING]).all()
    assert filled["area"][at] > hollow["area"][at] + 50
    others = np.arange(12) != at
    assert np.array_equal(filled["area"][others] >= hollow["area"][others], np.ones(11, dtype=bool))


def test_registered_exported_and_mirrored():
    import magnify_amd as mg
    from magnify_amd import _native as nat
    from magnify_amd import blobs

    assert mg.blobs is blobs and "blobs" in mg.__all__ and "blobs_pipe" in mg.__all__ and callable(mg.blobs)
    assert "find_blobs" in mg.components.get_all()
    assert (blobs.TILE_H, blobs.TILE_W) == (nat.DEFINES["MG_BLOB_TILE_H"], nat.DEFINES["MG_BLOB_TILE_W"])
    assert blobs.STATS == br.STATS
    for name in ("mg_blob_labels", "mg_blob_threshold", "mg_blob_select", "mg_blob_fill_holes", "mg_blob_scratch_bytes"):
        assert name in nat.PROTOTYPES
    sig = inspect.signature(mg.components.get("find_blobs"))
    assert list(sig.parameters) == ["threshold", "search_channel", "polarity", "smooth", "connectivity", "fill_holes",
                                    "min_area", "max_area", "clear_border", "roi_length", "max_components"]
    assert [p.default for p in sig.parameters.values()] == ["otsu", None, "bright", False, 8, False, 20, None, False, None,
                                                            1 << 20]
    steps = [name for name, _ in mg.blobs_pipe(despeckle=100, background=16, profile=2, roi_length=40).components]
    assert steps == ["standardize_format", "remove_outliers", "flatfield_correct", "stitch", "subtract_background",
                     "find_blobs", "profile_rois", "drop", "restore_format"]


def test_refusals_come_before_any_device_call():
    """None of these reaches the library or the GPU (there is none here): the argument is named in the message."""
    import torch

    from magnify_amd import blobs

    plane = np.zeros((4, 5), dtype=np.uint16)
    for kw, word in [(dict(threshold=float("nan")), "threshold"), (dict(threshold="otsu"), "threshold"),
                     (dict(threshold=1, connectivity=6), "connectivity"), (dict(threshold=1, max_components=0), "max_components"),
                     (dict(threshold=1, below=1), "below")]:
        with pytest.raises(ValueError, match=word):
            blobs.label(plane, **kw)
    for bad in (np.zeros((4, 5), dtype=np.int32), np.zeros((2, 4, 5), dtype=np.uint8), np.zeros((0, 5), dtype=np.uint8), [[1]]):
        with pytest.raises(ValueError, match="plane"):
            blobs.label(bad, 1)
    with pytest.raises(ValueError, match="threshold"):
        blobs.threshold_mask(plane, float("nan"))
    with pytest.raises(ValueError, match="plane"):
        blobs.threshold_mask(np.zeros((4, 5), dtype=np.int32), 1)
    with pytest.raises(ValueError, match="u8_plane"):
        blobs.otsu_level(plane)
    with pytest.raises(ValueError, match="on"):
        blobs.fill_holes(np.zeros((4, 5), dtype=np.float32))
    labels, stats = torch.zeros((4, 5), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int64)
    for kw, word in [(dict(min_area=-1), "min_area"), (dict(min_area=1.5), "min_area"), (dict(max_area=0), "max_area"),
                     (dict(min_area=5, max_area=4), "max_area"), (dict(clear_border=2), "clear_border")]:
        with pytest.raises(ValueError, match=word):
            blobs.select(labels, stats, **kw)
    with pytest.raises(ValueError, match="stats"):
        blobs.select(labels, stats[:, :7])
    with pytest.raises(ValueError, match="labels"):
        blobs.select(labels.to(torch.int64), stats)
    import magnify_amd as mg

    for kw, word in [(dict(search_channel=["a", "b"]), "search_channel"), (dict(threshold=10, smooth=True), "smooth"),
                     (dict(threshold="mean"), "threshold"), (dict(polarity="both"), "polarity"),
                     (dict(connectivity=6), "connectivity"), (dict(fill_holes=1), "fill_holes"), (dict(min_area=-3), "min_area"),
                     (dict(max_area=3), "max_area"), (dict(roi_length=246), "roi_length"), (dict(roi_length=0), "roi_length"),
                     (dict(max_components=0), "max_components")]:
        with pytest.raises(ValueError, match=word):
            mg.components.get("find_blobs")(**kw)
        with pytest.raises(ValueError, match=word):
            mg.blobs_pipe(**kw)


def test_otsu_rule_on_a_histogram_is_the_projects():
    from segment_ref import otsu_k

    from magnify_amd import blobs

    rng = np.random.default_rng(3)
    for _ in range(20):
        b = np.concatenate([rng.integers(0, 90, 500), rng.integers(120, 256, rng.integers(1, 400))])
        assert blobs.otsu_histogram_level(np.bincount(b, minlength=256)) == otsu_k(b)
    assert blobs.otsu_histogram_level(np.bincount([7], minlength=256)) == otsu_k(np.array([7])) == 0


def test_auto_roi_length_is_the_oracles():
    from magnify_amd import blobs

    for side in range(1, 40):
        stats = np.array([[1, 0, 0, 3, 5, 3 + side - 1, 5 + side // 2, 0]], dtype=np.int64)
        L = blobs.auto_roi_length(stats)
        assert L == br.auto_roi_length(stats) and L % 2 == 0 and side + 8 <= L <= side + 9
    assert blobs.auto_roi_length(np.zeros((0, 8), dtype=np.int64)) == br.auto_roi_length(np.zeros((0, 8))) == 8
