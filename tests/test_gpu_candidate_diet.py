"""mg_candidate_keys after its diet: k_candidates_tab walks its iterations in runs per lane, addresses its
lists by 32-bit offsets, and -- where no raw triples are asked for, the product path's form -- decides radius range and
layer from the squared radius and a table (mg_radius.h) instead of a square root.  Every key must be the one derived
from the oracle's float32 triples, in both forms of the call; with raw triples asked for those must equal the
oracle's bit for bit as well.

Planes as in test_gpu_kernels.py::test_candidates_degenerate_triplets (degenerate triplets, 20 % dense noise, true
circles plus the frame), and two more: one without edges, one with a single edge."""
import functools
import os

import numpy as np
import pytest

from oracle import ref_numeric as rn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H, W, GRID = 200, 260, 20
SEEDS = np.array([101, 102, 103, 104, 105], dtype=np.uint64)
UNTOUCHED = 0xA5A5A5A5  # what the key buffer holds before the call: a plane without edges is left alone
NUM_ITERS = [1, 2, 3, 2999, 3000, 40001]  # odd tails of a run of 2 or 4; 3000 < edges of the dense plane < 40001


@functools.lru_cache(maxsize=None)
def edge_planes():
    e = np.zeros((5, H, W), dtype=np.uint8)
    e[0, 10::40, 10::40] = 1                      # lone pixels
    e[0, 5, 60:80] = 1                            # a horizontal run inside one cell row
    e[0, 40:60, 7] = 1                            # a vertical run
    e[0, np.arange(100, 120), np.arange(100, 120)] = 1    # a diagonal: collinear triplets
    e[0, np.arange(140, 160), np.arange(59, 39, -1)] = 1  # the other diagonal
    e[0, 181, 181] = e[0, 183, 190] = 1           # two pixels in a cell
    e[1] = np.random.default_rng(5).random((H, W)) < 0.2  # dense: general triplets
    yy, xx = np.mgrid[0:H, 0:W]
    for cy, cx, r in ((60, 70, 9), (120, 180, 12), (150, 60, 6)):
        e[2] |= (np.abs(np.hypot(yy - cy, xx - cx) - r) < 0.6).astype(np.uint8)  # true circles
    e[2, 0, :] = e[2, :, 0] = e[2, H - 1, :] = e[2, :, W - 1] = 1  # the frame: centres off the image
    # e[3]: no edge at all
    e[4, 77, 133] = 1                             # a single edge: p0 = p1 = p2, whatever the draws
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def oracle_triples(plane, num_iter):
    """float32 [num_iter][3] of the oracle for a plane of edge_planes() and its seed; computed once, never changed."""
    e = edge_planes()[plane]
    want = rn.candidate_circles_from_picks(e, GRID, *rn.draw_picks(int(SEEDS[plane]), num_iter, e, GRID))
    want.setflags(write=False)
    return want


def keys_of(want, min_r, max_r):
    """The reference's radius / on-image filter (utils.py:157-166) on the rounded triples, as keys."""
    ntc = (W + 2 * max_r + 63) // 64
    with np.errstate(invalid="ignore"):
        ok = (want[:, 2] >= min_r) & (want[:, 2] <= max_r) & (np.abs(np.round(want[:, 0])) < 1e9) & (np.abs(np.round(want[:, 1])) < 1e9)
        c = np.where(ok[:, None], np.round(want), 0).astype(np.int64)
    ok &= (c[:, 0] + c[:, 2] >= 0) & (c[:, 1] + c[:, 2] >= 0) & (c[:, 0] - c[:, 2] < H) & (c[:, 1] - c[:, 2] < W)
    pr, pc = c[:, 0] + max_r, c[:, 1] + max_r
    key = (((pr >> 6) * ntc + (pc >> 6)) << 17) | ((c[:, 2] - min_r) << 12) | ((pr & 63) << 6) | (pc & 63)
    return np.where(ok, key, 0xFFFFFFFF).astype(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def lists():
    """The cell-major edge lists of edge_planes() on the device."""
    from magnify_amd import hotpath

    hotpath.require_gpu()
    e = edge_planes()
    P = e.shape[0]
    gr, gc = -(-H // GRID), -(-W // GRID)
    per_plane = [rn.grid_array(e[k], GRID) if e[k].any() else (np.zeros((0, 2), np.int32), np.zeros((gr, gc), np.int32), np.zeros((gr, gc), np.int32))
                 for k in range(P)]
    cap = max(len(c) for c, _, _ in per_plane)
    coords = np.zeros((P, cap, 2), dtype=np.int32)
    starts = np.zeros((P, gr, gc), dtype=np.int32)
    counts = np.zeros((P, gr, gc), dtype=np.int32)
    for k, (c, s, n) in enumerate(per_plane):
        coords[k, : len(c)], starts[k], counts[k] = c, s, n
    n_edges = np.array([len(c) for c, _, _ in per_plane], dtype=np.int32)
    assert n_edges[3] == 0 and n_edges[4] == 1 and n_edges[0] < 3000 < n_edges[1] < 40001
    return dict(coords=coords, starts=starts, counts=counts, n_edges=n_edges, cap=cap)


def candidate_keys(lists, planes, num_iter, min_r, max_r, raw):
    """One call of mg_candidate_keys on the given planes: (keys uint32 [P][num_iter], raw float32 [P][num_iter][3] or None)."""
    from magnify_amd import _native as nat

    planes = list(planes)
    d = {k: dev(lists[k][planes]) for k in ("coords", "starts", "counts", "n_edges")}
    d_seeds = torch.from_numpy(SEEDS[planes].view(np.int64)).cuda()
    keys = torch.full((len(planes), num_iter), UNTOUCHED - (1 << 32), dtype=torch.int32, device="cuda")
    d_raw = torch.full((len(planes), num_iter, 3), -7.0, dtype=torch.float32, device="cuda") if raw else None
    nat.check(nat.lib().mg_candidate_keys(d["coords"].data_ptr(), lists["cap"], d["starts"].data_ptr(), d["counts"].data_ptr(),
                                          d["n_edges"].data_ptr(), len(planes), H, W, GRID, d_seeds.data_ptr(), num_iter, min_r, max_r,
                                          keys.data_ptr(), d_raw.data_ptr() if raw else 0, torch.cuda.current_stream().cuda_stream),
              "mg_candidate_keys")
    return keys.cpu().numpy().view(np.uint32), (d_raw.cpu().numpy() if raw else None)


def check_against_oracle(got_keys, got_raw, planes, num_iter, min_r, max_r):
    for j, k in enumerate(planes):
        if k == 3:  # no edges: nothing is drawn, nothing is written
            assert (got_keys[j] == UNTOUCHED).all()
            assert got_raw is None or (got_raw[j] == -7.0).all()
            continue
        want = oracle_triples(k, num_iter)
        if got_raw is not None:
            np.testing.assert_array_equal(got_raw[j].view(np.uint32), want.view(np.uint32), err_msg=f"triples of plane {k}")
        np.testing.assert_array_equal(got_keys[j], keys_of(want, min_r, max_r), err_msg=f"keys of plane {k}")


@pytest.mark.parametrize("raw", [False, True], ids=["keys", "keys+raw"])
@pytest.mark.parametrize("num_iter", NUM_ITERS)
def test_keys_are_those_of_the_oracles_triples(lists, num_iter, raw):
    """All five planes in one call, so that strata of many edges (E > K), of one edge and of none (E < K) and the
    planes of no and of one edge meet in one launch; every length of the tail behind the last whole run."""
    min_r, max_r = 5, 14
    planes = range(5)
    keys, got_raw = candidate_keys(lists, planes, num_iter, min_r, max_r, raw)
    check_against_oracle(keys, got_raw, planes, num_iter, min_r, max_r)
    if num_iter >= 2999:
        assert (keys[2] != 0xFFFFFFFF).sum() > num_iter // 50  # the circles are found


@pytest.mark.parametrize("raw", [False, True], ids=["keys", "keys+raw"])
@pytest.mark.parametrize("num_iter", [5000, 8195])
def test_second_trip_of_the_walk(lists, num_iter, raw):
    """One workgroup of 1024 lanes per plane (the environment's MG_CANDIDATES_TAB_WALK, looked up on every call).
    With 5000 iterations every lane goes round its loop at least twice in runs of 2; in runs of 4 (what
    MG_CANDIDATES_TAB_RUN is) the first 226 lanes do, the others once -- so 8195 as well: two trips for every lane and
    a tail of three.  The carried stratum, the RNG counter and the tail must arrive where the uncapped launch puts them."""
    min_r, max_r = 5, 14
    planes = range(5)
    free_keys, free_raw = candidate_keys(lists, planes, num_iter, min_r, max_r, raw)
    old = os.environ.get("MG_CANDIDATES_TAB_WALK")
    os.environ["MG_CANDIDATES_TAB_WALK"] = "1"
    try:
        keys, got_raw = candidate_keys(lists, planes, num_iter, min_r, max_r, raw)
    finally:
        if old is None:
            del os.environ["MG_CANDIDATES_TAB_WALK"]
        else:
            os.environ["MG_CANDIDATES_TAB_WALK"] = old
    np.testing.assert_array_equal(keys, free_keys)
    if raw:
        np.testing.assert_array_equal(got_raw.view(np.uint32), free_raw.view(np.uint32))
    check_against_oracle(keys, got_raw, planes, num_iter, min_r, max_r)


def test_radii_at_the_tables_edges(lists):
    """(min_r, max_r) = (2, 26) on the plane of true circles: every radius layer 0 .. 24 occurs among the ORACLE's
    keys (asserted on its side: the test cannot pass by leaving layers out), and the keys are the oracle's."""
    min_r, max_r, num_iter = 2, 26, 200000
    want = keys_of(oracle_triples(2, num_iter), min_r, max_r)
    layers = (want[want != 0xFFFFFFFF] >> 12) & 31
    assert set(layers.tolist()) == set(range(25)), sorted(set(range(25)) - set(layers.tolist()))
    keys, _ = candidate_keys(lists, [2], num_iter, min_r, max_r, False)
    np.testing.assert_array_equal(keys[0], want)
