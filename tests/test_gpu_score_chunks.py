"""How the keyed scoring kernels (mg_score.hip) deal their work must not show in what they compute.

k_prefilter hands a wave a ticket: 128 positions of one (super-tile, radius) -- two circles per lane, a double chunk --
while at least 128 are left, then single chunks of up to 64; a position is mapped to its key through the per-radius
prefix table of the eight sub-tiles.  k_exact takes the survivors in rounds of 64 per workgroup and evaluates their hits
a few at a time.  Both are checked the way test_gpu_prefilter_pairs.py checks the walk: the NumPy bound sum of EVERY
unique circle from the finder's own bitmaps against the survivor list, no tolerance, and the tile-scoring path
(keyed_score = False) bit for bit; the inputs are asserted to contain every way a radius can be cut into tickets, read
from layer_starts (which these kernels only consume), and every kind of round the exact pass can meet."""
import numpy as np
import pytest

from oracle import ref_numeric as rn
from synth import noisy_bead_image
from test_gpu_prefilter_pairs import (H, HIGH_Q, LOW_Q, MAX_R, MIN_DIST, MIN_R, MIN_ROUNDNESS, SEEDS, SKIPPED, W, _unpack,
                                      bound_sums, make_planes)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NUM_ITER = 1000000  # the first value tried: the planes below hold every case of test_double_chunks_... at it
TS, SUBY, SUBX = 64, 2, 4
NTR, NTC = (H + 2 * MAX_R + TS - 1) // TS, (W + 2 * MAX_R + TS - 1) // TS
NR = MAX_R - MIN_R + 1


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


def chunk_planes():
    """The two planes of test_gpu_prefilter_pairs; the second with its lower right part flat from 34 pixels before
    the last super-tile on: no edge pixel within MAX_R of that super-tile, so all its radii are empty."""
    planes = make_planes()
    planes[1, 68:, 196:] = np.median(planes[1])
    return planes


def _find(hp, planes, num_iter, seeds, keyed_score, min_roundness=MIN_ROUNDNESS):
    cf = hp.CircleFinder(len(planes), H, W, MIN_R, MAX_R, num_iter)
    assert cf.keyed and cf.keyed_score
    cf.keyed_score = keyed_score
    cf.keep_debug_maps = True
    res, _ = cf.find(torch.from_numpy(planes).cuda(), None, LOW_Q, HIGH_Q, min_roundness, MIN_DIST, seeds)
    return cf, res


def _decode(kk):
    tile = (kk >> 17).astype(np.int64)
    return np.stack([(tile // NTC) * TS + ((kk >> 6) & 63) - MAX_R, (tile % NTC) * TS + (kk & 63) - MAX_R,
                     MIN_R + ((kk >> 12) & 31)], axis=1).astype(np.int64)


def _segments(layer_starts, sr, sc):
    """(first key, count) [8, NR] of the sub-tiles' radius segments of a super-tile; a sub-tile beyond the grid is empty."""
    first, count = np.zeros((SUBY * SUBX, NR), dtype=np.int64), np.zeros((SUBY * SUBX, NR), dtype=np.int64)
    for s in range(SUBY * SUBX):
        tr, tc = SUBY * sr + s // SUBX, SUBX * sc + s % SUBX
        if tr < NTR and tc < NTC:
            row = layer_starts[tr * NTC + tc].astype(np.int64)
            first[s], count[s] = row[:-1], row[1:] - row[:-1]
    return first, count


def _exact_scores(edges, angle, circles):
    """The oracle's score (mean_grad / perimeter length, float32) of every circle, from the finder's own angle map."""
    pad = 2 * MAX_R
    pa = np.pad(np.where(edges, angle, 0).astype(np.float32), pad)
    pe = np.pad(edges.astype(np.uint8), pad)
    out = np.empty(len(circles), dtype=np.float32)
    for r in np.unique(circles[:, 2]):
        sel = circles[:, 2] == r
        per = rn.circle_points(int(r))
        out[sel] = rn.mean_grad(pa, pe, circles[sel, :2].astype(np.int32) + pad, per) / len(per)
    return out


def _ulp_diff(a, b):
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(2 ** 31) - i, i) for i in (ia, ib))
    return np.abs(ia - ib)


def _check_plane(cf, p, table, pairs_of, min_roundness=MIN_ROUNDNESS):
    """Survivor list == the circles whose bound sum reaches the threshold; survivors' scores == the oracle's within the
    float32 ulp test_gpu_kernels allows for its angle table.  Returns (circles, survivors' list indices, keys)."""
    n, n_surv = int(cf.num_circles[p].item()), int(cf.num_surv[p].item())
    kk = cf.unique_keys[p, :n].cpu().numpy().view(np.uint32)
    assert len(np.unique(kk)) == n
    circles = _decode(kk)
    edges = _unpack(cf.edge_bits[p].cpu().numpy(), H, W).astype(bool)
    cb = cf.class_bits[p].cpu().numpy()
    c0, c1, c2 = (_unpack(cb[i], H, W).astype(np.int64) for i in range(3))
    surv = cf.surv_list[p, :n_surv].cpu().numpy()
    idx = surv[:, 0]
    assert len(np.unique(idx)) == len(idx)
    np.testing.assert_array_equal(surv[:, 1].view(np.uint32), kk[idx])
    survivors = np.zeros(n, dtype=bool)
    survivors[idx] = True
    if n:
        sums, _, _ = bound_sums(edges, 4 * c1 + 2 * c0 + c2, circles, table, pairs_of)
        points = np.array([2 * len(pairs_of(int(r))) for r in circles[:, 2]])
        need = np.ceil(64.0 * (float(np.float32(min_roundness)) * points - 1e-3)).astype(np.int64)
        np.testing.assert_array_equal(survivors, sums >= need)
    scores = cf.scores[p, :n].cpu().numpy()
    assert (scores[~survivors] == SKIPPED).all()
    if n_surv:
        want = _exact_scores(edges, cf.angle[p].cpu().numpy(), circles[idx])
        got = scores[idx]
        late = got == SKIPPED  # survivors the exact pass left early: below the threshold by the oracle's score
        assert (want[late] < np.float32(min_roundness)).all()
        assert _ulp_diff(got[~late], want[~late]).max(initial=0) <= 1
    return circles, idx, kk


def test_double_chunks_tails_and_empty_radii_drop_the_same_circles(hp):
    from magnify_amd import _native as nat

    planes = chunk_planes()
    cf, res = _find(hp, planes, NUM_ITER, SEEDS, True)
    table = nat.score_pair_table()
    layer_starts = cf.layer_starts.cpu().numpy()
    seen = dict(double_and_tail=0, one_to_two=0, below_one=0, empty=0, three_sub_tiles=0, both_halves=0)
    for p in range(len(planes)):
        circles, idx, kk = _check_plane(cf, p, table, nat.score_pairs)
        print(f"plane {p}: {len(circles)} circles, {len(idx)} survivors")
        # where the survivors sit in their radius's positions
        tile, layer = (kk[idx] >> 17).astype(np.int64), ((kk[idx] >> 12) & 31).astype(np.int64)
        tr, tc = tile // NTC, tile % NTC
        for sr in range((NTR + SUBY - 1) // SUBY):
            for sc in range((NTC + SUBX - 1) // SUBX):
                first, count = _segments(layer_starts[p], sr, sc)
                pre = np.cumsum(count, axis=0) - count
                total = count.sum(axis=0)
                seen["double_and_tail"] += int((total >= 192).sum())
                seen["one_to_two"] += int(((total >= 64) & (total < 128)).sum())
                seen["below_one"] += int(((total >= 1) & (total < 64)).sum())
                seen["empty"] += int((total == 0).sum())
                mine = (tr // SUBY == sr) & (tc // SUBX == sc)
                sub = (tr[mine] % SUBY) * SUBX + tc[mine] % SUBX
                pos = pre[sub, layer[mine]] + idx[mine] - first[sub, layer[mine]]
                assert (pos >= 0).all() and (pos < total[layer[mine]]).all()
                for rho in range(NR):
                    for k in range(total[rho] // 128):  # the double chunks of this radius
                        lo, hi = 128 * k, 128 * k + 128
                        inside = (count[:, rho] > 0) & (pre[:, rho] < hi) & (pre[:, rho] + count[:, rho] > lo)
                        seen["three_sub_tiles"] += int(inside.sum() >= 3)
                        here = pos[(layer[mine] == rho) & (pos >= lo) & (pos < hi)]
                        seen["both_halves"] += int((here < lo + 64).any() and (here >= lo + 64).any())
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    # the second product path: same circles, same scores, bit for bit
    cf2, res2 = _find(hp, planes, NUM_ITER, SEEDS, False)
    assert not cf2.keyed_score
    for p in range(len(planes)):
        assert len(res[p][0]) >= 3
        np.testing.assert_array_equal(res2[p][0], res[p][0])
        np.testing.assert_array_equal(res2[p][1].view(np.uint32), res[p][1].view(np.uint32))


# k_exact: 256 planes make a round of the large-batch launch as small as it gets (16 workgroups of 64 survivors), and
# min_roundness 0.15 lets ~1 600 circles of the small bead plane reach the exact pass (a few hundred at 0.3), most of
# them undecided for many terms
EXACT_PLANES, EXACT_ITER, EXACT_ROUNDNESS, ROUND = 256, 200000, 0.15, 16 * 64


def test_exact_pass_rounds_long_hit_lists_noise_and_nothing(hp):
    """Plane 0: the beads up to radius 26 (more than 64 hits: several evaluation steps), more survivors than a round
    and no multiple of 64; plane 1: pure noise; every other plane: constant, no edge and no survivor at all."""
    from magnify_amd import _native as nat

    planes = np.full((EXACT_PLANES, H, W), 1000, dtype=np.uint16)
    planes[0] = make_planes()[0]
    planes[1] = noisy_bead_image(300, (H, W), 0)[0]
    seeds = list(range(40, 40 + EXACT_PLANES))
    cf, res = _find(hp, planes, EXACT_ITER, seeds, True, EXACT_ROUNDNESS)
    table = nat.score_pair_table()
    n_surv = cf.num_surv.cpu().numpy()
    print(f"survivors: beads {n_surv[0]}, noise {n_surv[1]}, constant planes {n_surv[2:].max()}")
    assert n_surv[0] > ROUND and n_surv[0] % 64 != 0
    assert n_surv[1] > 0 and (n_surv[2:] == 0).all()
    for p in (0, 1, 2, EXACT_PLANES - 1):
        _check_plane(cf, p, table, nat.score_pairs, EXACT_ROUNDNESS)
    # a survivor with more than 64 edge pixels on its perimeter was scored (not left early)
    kk = cf.unique_keys[0, : int(cf.num_circles[0].item())].cpu().numpy().view(np.uint32)
    idx = cf.surv_list[0, : n_surv[0], 0].cpu().numpy()
    scored = cf.scores[0].cpu().numpy()[idx] != SKIPPED
    big = _decode(kk[idx])[scored]
    big = big[big[:, 2] >= 24]
    assert len(big) > 0
    edges = np.pad(_unpack(cf.edge_bits[0].cpu().numpy(), H, W), 2 * MAX_R)
    hits = []
    for row, col, r in big:
        per = rn.circle_points(int(r))
        hits.append(int(edges[row + 2 * MAX_R + per[:, 0], col + 2 * MAX_R + per[:, 1]].sum()))
    print(f"most hits on a scored perimeter: {max(hits)}")
    assert max(hits) > 64
    cf2, res2 = _find(hp, planes, EXACT_ITER, seeds, False, EXACT_ROUNDNESS)
    for p in (0, 1, 2, EXACT_PLANES - 1):
        np.testing.assert_array_equal(res2[p][0], res[p][0])
        np.testing.assert_array_equal(res2[p][1].view(np.uint32), res[p][1].view(np.uint32))
    assert len(res[0][0]) >= 5 and len(res[2][0]) == 0
