"""Every path of the greedy suppression against filter_neighbors, through the C ABI on torch buffers (tests/nms_ref.py holds
the oracle wrapper and the seeded planes; tests/test_cpu_nms_ref.py proves the planes are what they claim to be):

  A  mg_nms_sparse at its stated limits -- 12 288 / 12 289 circles, 9 216 buckets and one column more, the bucket-start
     scan with 2 and 9 buckets per thread and an odd bucket count, centres at and past -(min_dist + 1), an understated
     extent, pairs astride bucket borders, chains of dependent decisions; a refused plane's state bytes stay as they were
  B  the claim-grid path (same-centre pass or not, rounds to convergence, gather, cleanup) with the three lane mappings of
     the ring walk, twice on the same grid
  C  both paths through CircleFinder.nms_stage with tie keys, twice on the same finder
  D  mg_collect_circles alone: one to three staging chunks, every tail length, the clamp at out_cap.

Tie keys are unique 32-bit values, most with bit 31 set, handed over as int32; every launch runs with them and without.
Circles that are not alive hold sentinels (state bytes, keys, coordinates, scores) that must come back untouched.
Everything is integer-exact: every comparison is assert_array_equal.
"""
import types

import numpy as np
import pytest

import nms_ref as nr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


@pytest.fixture(scope="module")
def nat(hp):
    from magnify_amd import _native

    return _native


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _upload(layouts, cap, alive_state, state=None):
    """The planes' lists on the device.  State bytes: ``alive_state`` for alive circles, the sentinel for the others
    (``state``: written into this buffer instead of a new one)."""
    P = len(layouts)
    alive = np.zeros((P, cap), dtype=np.int32)
    host_state = np.full((P, cap), nr.STATE_SENTINEL, dtype=np.uint8)
    for k, lo in enumerate(layouts):
        assert lo.circles.shape == (cap, 3) and len(lo.alive) < cap
        alive[k, : len(lo.alive)] = lo.alive
        host_state[k, lo.alive] = alive_state
    b = types.SimpleNamespace(P=P, cap=cap, layouts=layouts, host_state=host_state)
    b.circles = dev(np.stack([lo.circles for lo in layouts]))
    b.scores = dev(np.stack([lo.scores for lo in layouts]))
    b.keys = dev(np.stack([lo.keys for lo in layouts]).view(np.int32))
    b.alive = dev(alive)
    b.num_alive = dev(np.array([len(lo.alive) for lo in layouts], dtype=np.int32))
    b.max_rc = dev(np.stack([lo.max_rc for lo in layouts]).astype(np.int32))
    if state is None:
        b.state = dev(host_state)
    else:
        assert state.shape == (P, cap)
        state.copy_(dev(host_state))
        b.state = state
    return b


def _want_state(layout, state_of_alive):
    """The plane's state bytes: the oracle's (or a constant) for the alive circles, the sentinel for the others."""
    want = np.full(len(layout.circles), nr.STATE_SENTINEL, dtype=np.uint8)
    want[layout.alive] = state_of_alive[layout.alive] if isinstance(state_of_alive, np.ndarray) else state_of_alive
    return want


def _inputs_untouched(b):
    np.testing.assert_array_equal(b.circles.cpu().numpy(), np.stack([lo.circles for lo in b.layouts]))
    np.testing.assert_array_equal(b.keys.cpu().numpy().view(np.uint32), np.stack([lo.keys for lo in b.layouts]))
    np.testing.assert_array_equal(b.scores.cpu().numpy(), np.stack([lo.scores for lo in b.layouts]))


# ---- A: mg_nms_sparse ------------------------------------------------------------------------------------------------
PRIOR = 0x3C  # what the alive circles' state bytes hold before the launch: the kernel does not look, a refusal leaves it


@pytest.mark.parametrize("use_keys", [True, False], ids=["keys", "index"])
@pytest.mark.parametrize("min_dist", nr.SPARSE_DISTS)
def test_sparse_kernel_at_its_limits(hp, nat, min_dist, use_keys):
    """One launch over the twelve planes of nms_ref.sparse_planes: d_done per plane, the oracle's state byte for every
    alive circle of a decided plane, the prior byte for every circle of a refused one, the sentinels untouched.

    d_done observed on MI355X (every min_dist, with and without keys): full 1, over 0, big 1, big_over 0, per2_even 1,
    per2_odd 1, at_edge 1, past_edge 0, understated 0, empty 1, border 1, chain 1."""
    layouts, want = nr.sparse_case(min_dist, use_keys)
    names = list(layouts)
    b = _upload([layouts[n] for n in names], nr.SPARSE_LIST_CAP, PRIOR)
    done = torch.full((b.P,), -3, dtype=torch.int32, device="cuda")
    dbits = dev(hp._ring_difference_bits(nat.circle_points(min_dist, True), min_dist))
    nat.check(nat.lib().mg_nms_sparse(b.circles.data_ptr(), b.cap, b.scores.data_ptr(), b.alive.data_ptr(), b.num_alive.data_ptr(),
                                      b.max_rc.data_ptr(), b.P, min_dist, dbits.data_ptr(), b.state.data_ptr(),
                                      b.keys.data_ptr() if use_keys else 0, done.data_ptr(), _stream()), "mg_nms_sparse")
    torch.cuda.synchronize()
    got_done = dict(zip(names, done.cpu().numpy().tolist()))
    print(f"min_dist {min_dist} keys {use_keys} d_done {got_done}")
    assert got_done == {n: d for n, (_, d) in nr.sparse_planes(min_dist).items()}
    state = b.state.cpu().numpy()
    for k, name in enumerate(names):
        if name in want:
            np.testing.assert_array_equal(state[k], _want_state(layouts[name], want[name][0]), err_msg=f"plane {name}")
        else:
            np.testing.assert_array_equal(state[k], b.host_state[k], err_msg=f"refused plane {name}")
    assert want["full"][0].max() == 2 and 0 < (want["full"][0] == 1).sum() < nr.SPARSE_CAP
    _inputs_untouched(b)


# ---- B: the claim-grid path --------------------------------------------------------------------------------------------
P_GRID = 4
CHAIN = 3  # the chain plane of nms_ref.grid_planes
# (circle_cap, max_alive: 0 = unknown, the launch is sized for circle_cap; None = the true maximum)
MAPPINGS = [(3200, 0), (8192, 0), (65536, 0), (8192, None)]


def _expected_cpw(cap, max_alive):
    """Circles a wave of the ring walk looks up at once (mg_nms_rounds): by the bound of alive circles over all planes."""
    bound = min(max_alive, cap) if max_alive > 0 else cap
    total = bound * P_GRID
    return 64 if total >= 262144 else 16 if total >= 32768 else 4


def _true_max_alive(d):
    return max(len(p.circles) for seed in (0, 1) for p in nr.grid_planes(d, seed))


def test_mappings_cover_every_lane_mapping():
    assert [_expected_cpw(cap, m if m is not None else nr.GRID_N) for cap, m in MAPPINGS] == [4, 16, 64, 4]
    assert all(_true_max_alive(d) == nr.GRID_N < min(cap for cap, _ in MAPPINGS) for d in nr.GRID_DISTS)


def _grid_cells(d):
    """Cells per plane: the largest extent d_max_rc asks for in either pass (k_nms leaves a plane alone that needs more)."""
    pad = 2 * d + 1
    return max((int(p.max_rc[0]) + 2 * pad) * (int(p.max_rc[1]) + 2 * pad) for seed in (0, 1) for p in nr.grid_planes(d, seed))


def _claim_grid_pass(nat, b, d, ring, grid, same_centre, use_keys, max_alive):
    """mg_nms_same_centre (optional), mg_nms_rounds two at a time until the last round leaves no plane undecided,
    mg_collect_circles, mg_nms_cleanup.  Returns the state bytes before the cleanup, the gathered tables and the number
    of round pairs each plane needed."""
    lib, s = nat.lib(), _stream()
    tie = b.keys.data_ptr() if use_keys else 0
    common = (b.circles.data_ptr(), b.cap, b.scores.data_ptr(), b.alive.data_ptr(), b.num_alive.data_ptr(), b.max_rc.data_ptr(),
              b.P, d)
    if same_centre:
        nat.check(lib.mg_nms_same_centre(*common, grid.data_ptr(), grid.shape[1], b.state.data_ptr(), tie, max_alive, 0, s),
                  "mg_nms_same_centre")
    undecided = torch.full((2, b.P), 7, dtype=torch.int32, device="cuda")
    needed = np.zeros(b.P, dtype=np.int64)
    for pair in range(1, 2001):
        nat.check(lib.mg_nms_rounds(*common, ring.data_ptr(), ring.shape[0], grid.data_ptr(), grid.shape[1], b.state.data_ptr(),
                                    undecided.data_ptr(), undecided.stride(0), 2, 0, tie, max_alive, 0, s), "mg_nms_rounds")
        left = undecided.cpu().numpy()
        assert set(np.unique(left).tolist()) <= {0, 1}
        needed[(needed == 0) & (left[1] == 0)] = pair
        if not left[1].any():
            break
    assert not left[1].any(), "the rounds did not converge"
    state = b.state.cpu().numpy()
    out_cap = nr.GRID_N
    out = torch.full((b.P, out_cap, 3), -77, dtype=torch.int32, device="cuda")
    out_scores = torch.full((b.P, out_cap), -5.0, dtype=torch.float32, device="cuda")
    num_out = torch.full((b.P,), 777, dtype=torch.int32, device="cuda")
    scratch = torch.zeros((b.P, 3 * out_cap), dtype=torch.int32, device="cuda")
    nat.check(lib.mg_collect_circles(b.circles.data_ptr(), b.cap, b.scores.data_ptr(), b.alive.data_ptr(), b.num_alive.data_ptr(),
                                     b.state.data_ptr(), 0, b.P, out.data_ptr(), out_scores.data_ptr(), out_cap,
                                     num_out.data_ptr(), scratch.data_ptr(), tie, 0, s), "mg_collect_circles")
    nat.check(lib.mg_nms_cleanup(*common, ring.data_ptr(), ring.shape[0], grid.data_ptr(), grid.shape[1], b.state.data_ptr(),
                                 max_alive, 0, s), "mg_nms_cleanup")
    torch.cuda.synchronize()
    return state, out.cpu().numpy(), out_scores.cpu().numpy(), num_out.cpu().numpy(), needed


@pytest.mark.parametrize("cap,max_alive", MAPPINGS, ids=[f"cap{c}-{'bound' if m is None else 'cap'}" for c, m in MAPPINGS])
@pytest.mark.parametrize("use_keys", [True, False], ids=["keys", "index"])
@pytest.mark.parametrize("same_centre", [True, False], ids=["same_centre", "rounds_only"])
@pytest.mark.parametrize("min_dist", nr.GRID_DISTS)
def test_claim_grid_path(nat, min_dist, same_centre, use_keys, cap, max_alive):
    """Four 700 x 900 planes (crowded, wrap, empty, chain), then four others on the same grid and state buffers."""
    d = min_dist
    max_alive = _true_max_alive(d) if max_alive is None else max_alive
    ring = dev(nat.circle_points(d, True))
    grid = torch.full((P_GRID, _grid_cells(d)), -1, dtype=torch.int64, device="cuda")
    state = None
    for seed in (0, 1):
        layouts, want = nr.grid_case(d, seed, cap, use_keys)
        b = _upload(list(layouts), cap, 0, state)
        state = b.state
        got_state, out, out_scores, num_out, needed = _claim_grid_pass(nat, b, d, ring, grid, same_centre, use_keys, max_alive)
        for k, (lo, (want_state, rows, kept_scores)) in enumerate(zip(layouts, want)):
            what = f"plane {k}, pass {seed}"
            np.testing.assert_array_equal(got_state[k], _want_state(lo, want_state), err_msg=what)
            assert num_out[k] == len(rows), what
            np.testing.assert_array_equal(out[k, : len(rows)], rows, err_msg=what)
            np.testing.assert_array_equal(out_scores[k, : len(rows)], kept_scores, err_msg=what)
            assert (out[k, len(rows):] == -77).all() and (out_scores[k, len(rows):] == -5.0).all(), what
        # after the cleanup: the grid as it was handed over, the alive circles undecided again, the others as they were
        assert bool((grid == -1).all())
        after = state.cpu().numpy()
        for k, lo in enumerate(layouts):
            np.testing.assert_array_equal(after[k], _want_state(lo, 0), err_msg=f"plane {k}, pass {seed}, after the cleanup")
        _inputs_untouched(b)
        print(f"min_dist {d} pass {seed}: round pairs per plane {needed.tolist()}")
        assert needed[CHAIN] > 50  # the chain's decisions really are handed over many times
        assert needed[2] == 1  # (the empty plane)


# ---- C: CircleFinder.nms_stage -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_dist", nr.STAGE_DISTS)
def test_both_paths_through_nms_stage(hp, monkeypatch, min_dist):
    """mg_nms_sparse + rounds for what it declines, and the rounds alone, with CircleFinder's own buffers, launch plan and
    grid, cf._tie_keys set: the oracle's tables, nms_done, state bytes back to 0, the claim grid back to all-ones; then
    other circles on the same finder."""
    P, d = 4, min_dist
    got = {}
    for sparse in (True, False):
        monkeypatch.setattr(hp, "_NMS_SPARSE", sparse)
        cf = hp.CircleFinder(P, nr.H, nr.W, 5, 25, 3200)
        assert cf._sparse_nms() == sparse
        for seed in (0, 1):
            layouts, want = nr.grid_case(d, seed, cf.cap, True)
            cf.circles.copy_(dev(np.stack([lo.circles for lo in layouts])))
            cf.scores.copy_(dev(np.stack([lo.scores for lo in layouts])))
            cf._tie_keys = dev(np.stack([lo.keys for lo in layouts]).view(np.int32))
            cf.alive.zero_()
            for k, lo in enumerate(layouts):
                cf.alive[k, : len(lo.alive)] = dev(lo.alive)
            cf.num_circles.fill_(cf.cap)
            cf.num_alive.copy_(dev(np.array([len(lo.alive) for lo in layouts], dtype=np.int32)))
            cf.max_rc.copy_(dev(np.stack([lo.max_rc for lo in layouts]).astype(np.int32)))
            out, out_scores, num_out = cf.nms_stage(d)
            torch.cuda.synchronize()
            counts = num_out.cpu().numpy()
            if sparse:
                assert cf.nms_done.cpu().numpy().tolist() == [1, 0, 1, 1]  # (the wrap plane is left to the rounds)
            assert not cf.state.any()
            assert bool((cf.nms_grid == -1).all())
            for k, (_, rows, kept_scores) in enumerate(want):
                what = f"plane {k}, pass {seed}, sparse {sparse}"
                assert counts[k] == len(rows), what
                np.testing.assert_array_equal(out[k, : len(rows)].cpu().numpy(), rows, err_msg=what)
                np.testing.assert_array_equal(out_scores[k, : len(rows)].cpu().numpy(), kept_scores, err_msg=what)
            got[sparse, seed] = [out[k, : counts[k]].cpu().numpy() for k in range(P)]
    for seed in (0, 1):
        for k in range(P):
            np.testing.assert_array_equal(got[True, seed][k], got[False, seed][k])


# ---- D: mg_collect_circles ---------------------------------------------------------------------------------------------
KEPT = (0, 1, 2047, 2048, 2049, 4099, 6001)  # tails of 0 .. 7 keys behind the trips of eight, one to three chunks of 2 048
COLLECT_CAP, GUARD = 6500, 64


def _collect_planes(keep_all):
    """Per plane: a layout of distinct circles, its state bytes (written here, not by a kernel) and the kept slots."""
    planes = []
    for k, m in enumerate(KEPT):
        extra = 0 if keep_all else 300  # dropped (2) and undecided (0) circles among the alive ones
        n = m + extra
        rng = np.random.default_rng([50, k, n])
        idx = rng.permutation(COLLECT_CAP)[:n]
        c = np.column_stack([idx // 100 - 20, (idx % 100) * 7 - 20, 5 + idx % 13])  # distinct (row, col)
        lo = nr.lay_out(nr._plane(c, nr._scores(rng, n), nr._keys(rng, n)), COLLECT_CAP, 60 + k)
        state = np.full(COLLECT_CAP, nr.STATE_SENTINEL, dtype=np.uint8)
        kept = rng.permutation(lo.alive)[:m]
        state[lo.alive] = np.where(np.arange(n) % 2 == 0, 2, 0)
        state[kept] = 1
        planes.append((lo, state, kept))
    return planes


def _collect(nat, planes, keep_all, use_keys, counters_clear, out_cap):
    P = len(planes)
    b = _upload([lo for lo, _, _ in planes], COLLECT_CAP, 0)
    b.state.copy_(dev(np.stack([st for _, st, _ in planes])))
    out = torch.full((P * out_cap + GUARD, 3), -77, dtype=torch.int32, device="cuda")
    out_scores = torch.full((P * out_cap + GUARD,), -5.0, dtype=torch.float32, device="cuda")
    scratch = torch.full((P * 3 * out_cap + GUARD,), -99, dtype=torch.int32, device="cuda")
    num_out = torch.full((P,), 0 if counters_clear else 777, dtype=torch.int32, device="cuda")
    nat.check(nat.lib().mg_collect_circles(b.circles.data_ptr(), b.cap, b.scores.data_ptr(), b.alive.data_ptr(),
                                           b.num_alive.data_ptr(), b.state.data_ptr(), keep_all, P, out.data_ptr(),
                                           out_scores.data_ptr(), out_cap, num_out.data_ptr(), scratch.data_ptr(),
                                           b.keys.data_ptr() if use_keys else 0, counters_clear, _stream()), "mg_collect_circles")
    torch.cuda.synchronize()
    out, out_scores = out.cpu().numpy(), out_scores.cpu().numpy()
    # nothing behind the tables, nothing behind the work space, no state byte changed
    assert (out[P * out_cap:] == -77).all() and (out_scores[P * out_cap:] == -5.0).all()
    assert (scratch[P * 3 * out_cap:] == -99).all()
    np.testing.assert_array_equal(b.state.cpu().numpy(), np.stack([st for _, st, _ in planes]))
    _inputs_untouched(b)
    return out[: P * out_cap].reshape(P, out_cap, 3), out_scores[: P * out_cap].reshape(P, out_cap), num_out.cpu().numpy()


@pytest.mark.parametrize("counters_clear", [0, 1])
@pytest.mark.parametrize("use_keys", [True, False], ids=["keys", "index"])
@pytest.mark.parametrize("keep_all", [0, 1])
def test_collect_orders_every_chunk_and_tail(nat, keep_all, use_keys, counters_clear):
    planes = _collect_planes(keep_all)
    out_cap = 6100
    out, out_scores, num_out = _collect(nat, planes, keep_all, use_keys, counters_clear, out_cap)
    for k, (lo, _, kept) in enumerate(planes):
        _, rows, kept_scores = nr.expected(lo.circles, lo.scores, lo.keys if use_keys else None, lo.alive if keep_all else kept, 0)
        m = KEPT[k]
        assert len(rows) == m == num_out[k], f"plane {k}"
        np.testing.assert_array_equal(out[k, :m], rows, err_msg=f"plane {k}")
        np.testing.assert_array_equal(out_scores[k, :m], kept_scores, err_msg=f"plane {k}")
        assert (out[k, m:] == -77).all() and (out_scores[k, m:] == -5.0).all(), f"plane {k}"


@pytest.mark.parametrize("use_keys", [True, False], ids=["keys", "index"])
@pytest.mark.parametrize("out_cap", [KEPT[-1] - 5, KEPT[4] - 5])
def test_collect_clamps_at_out_cap(nat, out_cap, use_keys):
    """out_cap five below a plane's kept count: the count is clamped, every emitted row is a distinct kept circle of the
    plane with its own score, nothing is written behind the tables.  WHICH circles drop out is not specified.  Planes
    that fit are complete and in order."""
    planes = _collect_planes(0)
    out, out_scores, num_out = _collect(nat, planes, 0, use_keys, 0, out_cap)
    clamped = 0
    for k, (lo, _, kept) in enumerate(planes):
        m = min(KEPT[k], out_cap)
        assert num_out[k] == m, f"plane {k}"
        assert (out[k, m:] == -77).all() and (out_scores[k, m:] == -5.0).all(), f"plane {k}"
        if KEPT[k] <= out_cap:
            _, rows, kept_scores = nr.expected(lo.circles, lo.scores, lo.keys if use_keys else None, kept, 0)
            np.testing.assert_array_equal(out[k, :m], rows, err_msg=f"plane {k}")
            np.testing.assert_array_equal(out_scores[k, :m], kept_scores, err_msg=f"plane {k}")
            continue
        clamped += 1
        slot_of = {(int(r), int(c)): int(s) for s, (r, c, _) in zip(kept, lo.circles[kept])}
        assert len(slot_of) == len(kept)
        slots = np.array([slot_of.get((int(r), int(c)), -1) for r, c, _ in out[k, :m]])
        assert (slots >= 0).all() and len(np.unique(slots)) == m, f"plane {k}"
        np.testing.assert_array_equal(out[k, :m], lo.circles[slots], err_msg=f"plane {k}")
        np.testing.assert_array_equal(out_scores[k, :m], lo.scores[slots], err_msg=f"plane {k}")
    assert clamped == (1 if out_cap > KEPT[-2] else 5)
