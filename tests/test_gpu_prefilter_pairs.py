"""The keyed scoring prefilter (k_prefilter of mg_score.hip) decides by its tables, not by how it walks the perimeter:
a circle is dropped if and only if the sum of its perimeter points' table bounds (mg_score_pair_table; a point that is
no edge pixel or lies off the image counts 0) is below ceil(64 (min_roundness P - 1e-3)).  The test recomputes that sum
in NumPy for EVERY unique circle of two small noisy planes, at every radius 2..26, from the finder's own edge and
orientation bitmaps, and compares the decision set; then it runs the same call through the other scoring path
(mg_score_circles, tile scoring with the angle map), which has to return the same circles and scores bit for bit.

The planes are 150 x 300: the padded centre grid is 2 x 2 super-tiles, the image's right and bottom edges fall inside
a window, beads of every size sit in the image and across its right and bottom borders."""
import numpy as np
import pytest

from oracle import ref_numeric as rn
from synth import draw_beads, noisy_bead_image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H, W = 150, 300
MIN_R, MAX_R = 2, 26
NUM_ITER = 200000
SEEDS = [31, 32]
LOW_Q, HIGH_Q, MIN_ROUNDNESS, MIN_DIST = 0.1, 0.9, 0.3, 5
SKIPPED = np.float32(-2.0)

# (row, col, radius) of the beads; the last three of a plane are cut by the right border, the bottom border, the corner
BEADS = [
    [(40, 40, 26), (36, 108, 22), (32, 166, 18), (26, 214, 14), (22, 252, 10), (20, 280, 6), (112, 28, 16), (100, 70, 8),
     (104, 96, 5), (100, 116, 4), (106, 134, 3), (100, 148, 2), (104, 176, 12), (80, 296, 20), (146, 236, 24), (147, 297, 7)],
    [(38, 38, 25), (34, 104, 21), (30, 160, 17), (26, 206, 13), (22, 244, 9), (18, 276, 7), (112, 30, 19), (104, 80, 11),
     (104, 112, 5), (100, 132, 3), (110, 150, 2), (96, 176, 15), (120, 210, 4), (60, 298, 9), (150, 252, 26), (148, 299, 23)],
]


def make_planes():
    planes = []
    for k, beads in enumerate(BEADS):
        noise, _ = noisy_bead_image(100 + k, (H, W), 0)
        b = np.asarray(beads)
        values = np.random.default_rng(200 + k).integers(500, 4001, size=len(b))
        disks = draw_beads((H, W), b[:, :2], 2 * b[:, 2], values).astype(np.int64)
        planes.append(np.where(disks > 0, disks + noise, noise).clip(0, 65535).astype(np.uint16))
    return np.stack(planes)


def bound_sums(edges, bins, circles, table, pairs_of):
    """Sum of the table bounds over the perimeter of every circle (row, col, r): table[r][k][bin] at the edge pixels
    among the points +-pairs_of(r)[k], 0 elsewhere.  Returns (sums, need, touches_last_column)."""
    h, w = edges.shape
    sums = np.zeros(len(circles), dtype=np.int64)
    need = np.zeros(len(circles), dtype=np.int64)
    last_col = np.zeros(len(circles), dtype=bool)
    for r in np.unique(circles[:, 2]):
        sel = np.nonzero(circles[:, 2] == r)[0]
        first = pairs_of(int(r)).astype(np.int64)
        n = len(first)
        pts = np.concatenate([first, -first])  # point j belongs to pair j mod n
        bound = table[r, :n].view(np.int8).reshape(n, 8).astype(np.int64)
        rows = circles[sel, 0, None].astype(np.int64) + pts[None, :, 0]
        cols = circles[sel, 1, None].astype(np.int64) + pts[None, :, 1]
        inside = (rows >= 0) & (rows < h) & (cols >= 0) & (cols < w)
        rr, cc = np.clip(rows, 0, h - 1), np.clip(cols, 0, w - 1)
        hit = inside & edges[rr, cc]
        k = np.broadcast_to(np.tile(np.arange(n), 2)[None, :], rows.shape)
        sums[sel] = np.where(hit, bound[k, bins[rr, cc]], 0).sum(axis=1)
        need[sel] = int(np.ceil(64.0 * (float(np.float32(MIN_ROUNDNESS)) * (2 * n) - 1e-3)))
        last_col[sel] = (inside & (cols == w - 1)).any(axis=1)
    return sums, need, last_col


def check_inputs(circles, sums, need):
    """The conditions the planes and seeds were chosen for (both planes together)."""
    per_radius = np.bincount(circles[:, 2], minlength=MAX_R + 1)[MIN_R:]
    assert per_radius.min() >= 100, per_radius
    assert len(np.unique(circles[sums >= need, 2])) >= 10
    outside = (circles[:, 0] < 0) | (circles[:, 0] >= H) | (circles[:, 1] < 0) | (circles[:, 1] >= W)
    assert outside.any()


def _unpack(words, h, w):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[: h * w].reshape(h, w)


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def _find(hp, planes, keyed_score):
    cf = hp.CircleFinder(len(planes), H, W, MIN_R, MAX_R, NUM_ITER)
    assert cf.keyed and cf.keyed_score  # one call covers the radii 2..26
    cf.keyed_score = keyed_score
    cf.keep_debug_maps = True
    res, _ = cf.find(torch.from_numpy(planes).cuda(), None, LOW_Q, HIGH_Q, MIN_ROUNDNESS, MIN_DIST, SEEDS)
    return cf, res


def test_prefilter_drops_exactly_the_circles_below_the_bound(hp):
    """(a) the decision set, every unique circle, no tolerance; (b) the tile-scoring path gives the same results.

    `scores == MG_SCORE_SKIPPED` marks the prefilter's drops AND the survivors the exact pass found below the threshold,
    so the prefilter's own decision is read where it writes it: the survivor list.  Every circle with sum < need must
    carry MG_SCORE_SKIPPED and must not be a survivor, every other circle must be one; a survivor that carries
    MG_SCORE_SKIPPED must be below min_roundness by the oracle's exact score."""
    from magnify_amd import _native as nat

    planes = make_planes()
    cf, res = _find(hp, planes, True)
    table = nat.score_pair_table()
    ntc = (W + 2 * MAX_R + 63) // 64
    n_circles, n_surv = cf.num_circles.cpu().numpy(), cf.num_surv.cpu().numpy()
    ukeys = cf.unique_keys.cpu().numpy().view(np.uint32)
    scores = cf.scores.cpu().numpy()
    surv = cf.surv_list.cpu().numpy()
    edge_bits, class_bits = cf.edge_bits.cpu().numpy(), cf.class_bits.cpu().numpy()
    angle = cf.angle.cpu().numpy()
    everything, any_last_col = [], False
    for p in range(len(planes)):
        n = int(n_circles[p])
        kk = ukeys[p, :n]
        assert len(np.unique(kk)) == n
        tile = (kk >> 17).astype(np.int64)
        circles = np.stack([(tile // ntc) * 64 + ((kk >> 6) & 63) - MAX_R, (tile % ntc) * 64 + (kk & 63) - MAX_R,
                            MIN_R + ((kk >> 12) & 31)], axis=1).astype(np.int64)
        edges = _unpack(edge_bits[p], H, W).astype(bool)
        c0, c1, c2 = (_unpack(class_bits[p, i], H, W).astype(np.int64) for i in range(3))
        sums, need, last_col = bound_sums(edges, 4 * c1 + 2 * c0 + c2, circles, table, nat.score_pairs)
        any_last_col |= bool(last_col.any())
        everything.append((circles, sums, need))
        drop = sums < need
        survivors = np.zeros(n, dtype=bool)
        idx = surv[p, : n_surv[p], 0]
        assert len(np.unique(idx)) == len(idx)
        survivors[idx] = True
        np.testing.assert_array_equal(surv[p, : n_surv[p], 1].view(np.uint32), kk[idx])
        skipped = scores[p, :n] == SKIPPED
        print(f"plane {p}: {n} circles, {int(drop.sum())} below the bound, {int(survivors.sum())} survivors, "
              f"{int((skipped & ~drop).sum())} survivors skipped by the exact pass")
        np.testing.assert_array_equal(survivors, ~drop)
        assert skipped[drop].all()
        late = np.nonzero(skipped & ~drop)[0]
        if len(late):
            pad = 2 * MAX_R
            pa = np.pad(np.where(edges, angle[p], 0).astype(np.float32), pad)
            pe = np.pad(edges.astype(np.uint8), pad)
            for r in np.unique(circles[late, 2]):
                sel = late[circles[late, 2] == r]
                per = rn.circle_points(int(r))
                exact = rn.mean_grad(pa, pe, circles[sel, :2].astype(np.int32) + pad, per) / len(per)
                assert (exact.astype(np.float32) < np.float32(MIN_ROUNDNESS)).all()
    check_inputs(*(np.concatenate(x) for x in zip(*everything)))
    assert any_last_col
    # (b) the second product path
    cf2, res2 = _find(hp, planes, False)
    assert not cf2.keyed_score
    for p in range(len(planes)):
        assert len(res[p][0]) >= 5
        np.testing.assert_array_equal(res2[p][0], res[p][0])
        np.testing.assert_array_equal(res2[p][1].view(np.uint32), res[p][1].view(np.uint32))
