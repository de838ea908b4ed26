"""k_tile_dedup (mg_circles.hip, C-ABI call mg_keys_to_circles) at the edges of its counting and emission.

After the key scan a thread of a tile group owns a run of PER consecutive words of the group's LDS layers, reads it
once (bit count, count in front of the one layer start a run can hold, mask of the non-empty words) and then stores
one key per step of a flat loop, fetching the next non-empty word when the current one is used up.  The cases below
are hand-made key lists, called straight through the C ABI on a one-cell grid: with grid >= max(h, w) there is one
cell, cell_starts = [0] and cell_counts = num_edges = [E >= 1] give every tile whose reach rectangle meets the image
the single key range [0, num_iter), so every tile group sees every key in the order listed.

The oracle is NumPy: drop MG_NO_KEY, np.unique, split by key >> 17.  Tile slices are compared exactly through
tile_ranges (the order of the groups' slices is arrival order), layer_starts exactly relative to the slice, every
case twice into buffers filled with two different patterns, with guard words behind every buffer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TS, LAYER_WORDS, NT, TX = 64, 128, 256, 2  # tile edge, words per layer, threads and tiles per workgroup
NO_KEY = np.uint32(0xFFFFFFFF)
PATTERNS = (0x5A5A5A5A, 0x3C3C3C3C)  # tile >> 17 of either is far beyond every tile used here
GUARD = 64
H = W = 160


@pytest.fixture(scope="module")
def hp():
    from magnify_amd import hotpath

    hotpath.require_gpu()
    return hotpath


class Layout:
    """What mg_key_layout derives, and the run of words a thread of a group of `ntx` tiles owns."""

    def __init__(self, min_r, max_r, h=H, w=W):
        self.h, self.w, self.min_r, self.max_r = h, w, min_r, max_r
        self.ntr, self.ntc = (h + 2 * max_r + TS - 1) // TS, (w + 2 * max_r + TS - 1) // TS
        self.nr = max_r - min_r + 1
        self.n_tiles = self.ntr * self.ntc
        self.words = self.nr * LAYER_WORDS  # per tile
        # every tile's reach rectangle meets the image (the docstring's condition for "sees every key")
        reach = max_r + 2
        assert (self.ntr - 1) * TS - max_r - reach <= h - 1 and (self.ntc - 1) * TS - max_r - reach <= w - 1

    def per(self, ntx=TX):
        return -(-(ntx * self.words) // NT)

    def key(self, tile, word, bit):
        """Key of bit `bit` of word `word` (layer * 128 + row * 2 + col // 32) of a tile."""
        assert 0 <= tile < self.n_tiles and 0 <= word < self.words and 0 <= bit < 32
        return np.uint32((tile << 17) | (word << 5) | bit)

    def group_key(self, tile0, gword, bit):
        """Key of a word counted through the group that starts at tile0 (the index a thread's run is made of)."""
        return self.key(tile0 + gword // self.words, gword % self.words, bit)

    def tile_keys(self, tile, words=None):
        """Every key of the given words (default: all) of a tile."""
        words = np.arange(self.words) if words is None else np.asarray(words)
        low = (words[:, None].astype(np.uint32) << np.uint32(5)) | np.arange(32, dtype=np.uint32)[None, :]
        return (np.uint32(tile << 17) | low).ravel()

    def run_offsets_of_layer_starts(self, ntx=TX):
        """{layer index in the group: offset of its first word inside the run that holds it}."""
        per = self.per(ntx)
        return {li: (li * LAYER_WORDS) % per for li in range(ntx * self.nr)}


def _i32(pattern):
    return int(np.uint32(pattern).view(np.int32))


def launch(hp, lay, keys, edges=None, cap=None, pattern=PATTERNS[0]):
    """One mg_keys_to_circles call on the one-cell grid.  keys: one uint32 array per plane (padded with MG_NO_KEY to
    a common length); edges: E per plane (default 1).  Returns (ukeys [P, cap], tile_ranges [P, n_tiles, 2],
    layer_starts [P, n_tiles, nr + 1], num_circles [P], cap) after checking the guard words."""
    from magnify_amd import _native as nat

    P = len(keys)
    num_iter = max(max(len(k) for k in keys), 1)
    host = np.full((P, num_iter), NO_KEY, dtype=np.uint32)
    for p, k in enumerate(keys):
        host[p, : len(k)] = k
    valid = host[host != NO_KEY]
    assert ((valid >> 17) < lay.n_tiles).all() and (((valid >> 12) & 31) < lay.nr).all()
    edges = [1] * P if edges is None else edges
    uniq = [len(np.unique(host[p][host[p] != NO_KEY])) if edges[p] else 0 for p in range(P)]
    cap = max(uniq) + 5 if cap is None else cap
    assert cap >= 0
    dev = torch.device("cuda")
    d_keys = torch.from_numpy(host.view(np.int32)).to(dev)
    d_starts = torch.zeros(P, dtype=torch.int32, device=dev)
    d_counts = torch.tensor(edges, dtype=torch.int32, device=dev)
    d_edges = d_counts.clone()
    sizes = dict(ukeys=P * cap, ranges=P * lay.n_tiles * 2, starts=P * lay.n_tiles * (lay.nr + 1), num=P)
    buf = {k: torch.full((n + GUARD,), _i32(pattern), dtype=torch.int32, device=dev) for k, n in sizes.items()}
    grid = max(lay.h, lay.w)
    rc = nat.lib().mg_keys_to_circles(d_keys.data_ptr(), num_iter, d_starts.data_ptr(), d_counts.data_ptr(),
                                      d_edges.data_ptr(), P, lay.h, lay.w, grid, lay.min_r, lay.max_r,
                                      buf["ukeys"].data_ptr(), cap, buf["ranges"].data_ptr(), buf["num"].data_ptr(),
                                      buf["starts"].data_ptr(), 0, hp._stream())
    assert rc == 0
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    for k, n in sizes.items():
        assert (out[k][n:].view(np.uint32) == np.uint32(pattern)).all(), f"guard words behind {k} were written"
    return (out["ukeys"][: sizes["ukeys"]].view(np.uint32).reshape(P, cap),
            out["ranges"][: sizes["ranges"]].reshape(P, lay.n_tiles, 2).astype(np.int64),
            out["starts"][: sizes["starts"]].reshape(P, lay.n_tiles, lay.nr + 1).astype(np.int64),
            out["num"][:P].astype(np.int64), cap)


def check_plane(lay, plane_keys, n_edges, ukeys, ranges, starts, num, cap, pattern):
    """One plane of a launch against the oracle; valid for cap above, at and below the unique count."""
    k = plane_keys[plane_keys != NO_KEY] if n_edges else np.zeros(0, dtype=np.uint32)
    want_all = np.unique(k)
    n = len(want_all)
    assert num == min(n, cap)
    tiles = (want_all >> 17).astype(np.int64)
    raw_start_known = []
    for t in range(lay.n_tiles):
        want = want_all[tiles == t]
        start, count = ranges[t]
        assert count == len(want), f"tile {t}"
        assert 0 <= start <= cap
        rel = np.concatenate([[0], np.cumsum(np.bincount((want >> 12) & 31, minlength=lay.nr)[: lay.nr])])
        if start < cap or n <= cap:  # the slice's true start is what was written
            np.testing.assert_array_equal(starts[t], np.minimum(start + rel, cap), err_msg=f"layer starts of tile {t}")
            seen = min(count, cap - start)
            np.testing.assert_array_equal(ukeys[start:start + seen], want[:seen], err_msg=f"keys of tile {t}")
            raw_start_known.append((start, count, t))
        else:  # clipped: everything of this tile lies at or beyond cap
            assert (starts[t] == cap).all()
    # tiles of a group back to back
    for tr in range(lay.ntr):
        for tc in range(0, lay.ntc - 1, TX):
            t = tr * lay.ntc + tc
            if ranges[t, 0] < cap or n <= cap:
                assert ranges[t + 1, 0] == min(ranges[t, 0] + ranges[t, 1], cap)
    # the slices tile [0, min(n, cap)) without gap or overlap
    pos = 0
    for start, count, t in sorted(s for s in raw_start_known if s[1] > 0):
        assert start == pos, f"tile {t}"
        pos = start + count
    assert pos >= min(n, cap) and (n > cap or pos == n)
    written = ukeys[: min(n, cap)]
    assert np.isin(written, want_all).all() and len(np.unique(written)) == len(written)
    assert (ukeys[min(n, cap):] == np.uint32(pattern)).all(), "keys stored behind the plane's count"


def run_case(hp, lay, keys, edges=None, cap=None):
    """Twice, into differently filled buffers; returns the first launch's outputs."""
    first = None
    for pattern in PATTERNS:
        ukeys, ranges, starts, num, used_cap = launch(hp, lay, keys, edges, cap, pattern)
        for p in range(len(keys)):
            check_plane(lay, keys[p], 1 if edges is None else edges[p], ukeys[p], ranges[p], starts[p], num[p],
                        used_cap, pattern)
        first = first or (ukeys, ranges, starts, num, used_cap)
    return first


def random_keys(lay, rng, n, tiles=None):
    tiles = np.arange(lay.n_tiles) if tiles is None else np.asarray(tiles)
    return ((rng.choice(tiles, n).astype(np.uint32) << np.uint32(17)) |
            rng.integers(0, lay.words * 32, n).astype(np.uint32))


# (min_r, max_r): the bench's range (nr 21), a wider one (25), a single radius, and nr = 32, the limit of s_cnt
RANGES = [(5, 25), (2, 26), (7, 7), (1, 32)]


@pytest.mark.parametrize("min_r,max_r", RANGES)
def test_random_keys_at_the_bench_density(hp, min_r, max_r):
    """~0.3 keys per word over every tile, listed in random order, every key 1-3 times, MG_NO_KEY in between."""
    lay = Layout(min_r, max_r)
    assert lay.nr == max_r - min_r + 1 and lay.nr <= 32
    rng = np.random.default_rng(100 + lay.nr)
    k = random_keys(lay, rng, int(0.3 * lay.n_tiles * lay.words))
    k = np.concatenate([k, k[::2], k[::3], np.full(len(k) // 4, NO_KEY)])
    rng.shuffle(k)
    run_case(hp, lay, [k])


@pytest.mark.parametrize("min_r,max_r", RANGES)
def test_runs_that_end_at_before_and_behind_a_layer_start(hp, min_r, max_r):
    """Keys in the last word of every layer, the first and the second of the next, so the thread that owns a layer
    start has keys on both sides of it wherever the start lies in its run.  The offsets of the layer starts inside
    their runs are derived from the run length and asserted: with more than one layer they include 0 (the run begins
    with the layer: every tile's first layer, PER * 128 being a multiple of 128 words), 1 and PER - 1."""
    lay = Layout(min_r, max_r)
    per = lay.per()
    assert per == lay.nr and per <= 32  # pairs: 2 * nr * 128 / 256 -- a run fits the 32-bit mask of its words
    offs = lay.run_offsets_of_layer_starts()
    # a tile's first layer always begins a run, (nr * 128) % nr == 0: in a pair the tile boundary is never inside a run
    assert offs[0] == 0 and offs[lay.nr] == 0
    if lay.nr in (21, 25):  # 128 and PER coprime: every offset occurs
        assert {0, 1, per - 1} <= set(offs.values()), offs
    if lay.nr == 21:  # the bench: layer 11 starts at word 1408 = 67 * 21 + 1, layer 10 at 1280 = 61 * 21 - 1
        assert offs[11] == 1 and offs[10] == per - 1
    if lay.nr in (1, 32):  # PER divides 128: every layer start begins a run
        assert set(offs.values()) == {0}
    keys = []
    for tr in range(lay.ntr):
        for tc0 in range(0, lay.ntc, TX):
            tile0, ntx = tr * lay.ntc + tc0, min(TX, lay.ntc - tc0)
            for li in range(ntx * lay.nr):
                for gw, bit in ((li * LAYER_WORDS - 1, 31), (li * LAYER_WORDS, 0), (li * LAYER_WORDS + 1, 17)):
                    if 0 <= gw < ntx * lay.words:
                        keys.append(lay.group_key(tile0, gw, bit))
    ukeys, ranges, starts, num, cap = run_case(hp, lay, [np.array(keys[::-1], dtype=np.uint32)])
    assert num[0] == len(keys)


BENCH = (5, 25)


def test_full_word_full_layer_full_tile(hp):
    """The largest counts: 32 keys in a word, 4 096 in a layer, nr * 4 096 in a tile (a thread stores 21 * 32 keys)."""
    lay = Layout(*BENCH)
    assert lay.nr == 21 and lay.ntc == 4 and lay.n_tiles == 16
    word = lay.tile_keys(5, [77])
    layer = lay.tile_keys(6, np.arange(3 * LAYER_WORDS, 4 * LAYER_WORDS))
    tile = lay.tile_keys(9)
    assert len(word) == 32 and len(layer) == 4096 and len(tile) == 21 * 4096
    ukeys, ranges, starts, num, cap = run_case(hp, lay, [word, layer, tile, np.concatenate([tile, layer, word])])
    assert list(num) == [32, 4096, 21 * 4096, 32 + 4096 + 21 * 4096]
    assert ranges[2, 9, 1] == 21 * 4096 and (np.diff(starts[2, 9]) == 4096).all()


def test_single_keys_first_word_last_word_second_tile_only(hp):
    lay = Layout(*BENCH)
    last = TX * lay.words - 1
    planes = [np.array([lay.group_key(4, 0, 0)], dtype=np.uint32),       # first word of a group
              np.array([lay.group_key(4, last, 31)], dtype=np.uint32),   # last word of a group
              np.array([lay.group_key(4, 0, 0), lay.group_key(4, last, 31)], dtype=np.uint32),
              np.array([lay.key(7, 0, 0), lay.key(7, 1300, 3), lay.key(7, lay.words - 1, 31)], dtype=np.uint32)]
    assert planes[1][0] >> 17 == 5 and all(k >> 17 == 7 for k in planes[3])  # tile 7: the second of the pair (6, 7)
    ukeys, ranges, starts, num, cap = run_case(hp, lay, planes)
    assert list(num) == [1, 1, 2, 3]
    assert ranges[3, 6, 1] == 0 and ranges[3, 7, 1] == 3 and ranges[3, 7, 0] == ranges[3, 6, 0]


def test_keys_that_differ_only_in_the_tile(hp):
    lay = Layout(*BENCH)
    low = [(0, 0), (1407, 5), (1408, 5), (lay.words - 1, 31)]
    k = np.array([lay.key(t, wd, b) for wd, b in low for t in range(lay.n_tiles)], dtype=np.uint32)
    ukeys, ranges, starts, num, cap = run_case(hp, lay, [k])
    assert num[0] == len(k) and (ranges[0, :, 1] == len(low)).all()


def test_empty_group_between_two_full_ones(hp):
    """Groups (0, 1) and (4, 5) with every bit set, group (2, 3) -- launched between them -- empty."""
    lay = Layout(*BENCH)
    k = np.concatenate([lay.tile_keys(t) for t in (0, 1, 4, 5)])
    ukeys, ranges, starts, num, cap = run_case(hp, lay, [k])
    assert num[0] == 4 * lay.words * 32
    assert (ranges[0, [2, 3], 1] == 0).all() and (ranges[0, [0, 1, 4, 5], 1] == lay.words * 32).all()


def test_plane_without_edges_beside_planes_with_keys(hp):
    """num_edges = 0: the plane's keys are not looked at, its count stays 0 and its ranges are empty."""
    lay = Layout(*BENCH)
    rng = np.random.default_rng(5)
    planes = [random_keys(lay, rng, 3000), random_keys(lay, rng, 3000), random_keys(lay, rng, 3000)]
    ukeys, ranges, starts, num, cap = run_case(hp, lay, planes, edges=[7, 0, 1])
    assert num[1] == 0 and num[0] > 2900 and num[2] > 2900
    assert (ranges[1] == 0).all() and (starts[1] == 0).all()


def test_last_tile_column_of_an_odd_tile_row(hp):
    """w = 208, max_r = 26: five tile columns, so the last group of a tile row holds one tile (ntx = 1) and a thread's
    run is 13 of its 3 200 words -- the last threads own a short run or none."""
    lay = Layout(2, 26, h=160, w=208)
    assert lay.ntc == 5 and lay.ntc % TX == 1 and lay.nr == 25
    per = lay.per(1)
    assert per == 13 and NT * per > lay.words and (lay.words // per) * per < lay.words  # a short last run exists
    last_col = [tr * lay.ntc + lay.ntc - 1 for tr in range(lay.ntr)]
    rng = np.random.default_rng(9)
    k = [random_keys(lay, rng, 4000, last_col)]
    for t in last_col:
        k.append(lay.tile_keys(t, [0, per - 1, per, lay.words - 2, lay.words - 1]))
        k.append(np.array([lay.key(t, li * LAYER_WORDS + d, 9) for li in range(1, lay.nr) for d in (-1, 0, 1)],
                          dtype=np.uint32))
    only_last = np.concatenate(k)
    both = np.concatenate([only_last, random_keys(lay, rng, 4000)])
    ukeys, ranges, starts, num, cap = run_case(hp, lay, [only_last, both])
    others = np.setdiff1d(np.arange(lay.n_tiles), last_col)
    assert (ranges[0, others, 1] == 0).all() and (ranges[0, last_col, 1] > 1000).all()


def test_heavy_duplication_no_key_runs_and_foreign_tiles(hp):
    """Every key 50 times; runs of MG_NO_KEY longer than a thread's batch of loads; every group meets the keys of all
    other tiles (one cell: every group scans the whole list)."""
    lay = Layout(*BENCH)
    rng = np.random.default_rng(50)
    base = random_keys(lay, rng, 2000)
    k = np.repeat(base, 50)
    rng.shuffle(k)
    gap = np.full(NT * 8 + 37, NO_KEY)
    k = np.concatenate([gap, k[:30000], gap, gap, k[30000:], gap])
    ukeys, ranges, starts, num, cap = run_case(hp, lay, [k])
    assert num[0] == len(np.unique(base)) and (ranges[0, :, 1] > 0).all()


@pytest.mark.parametrize("below", [0, 1, 700, "all"])
def test_circle_cap_at_and_below_the_unique_count(hp, below):
    """cap = unique count - below: num_circles == cap, what is stored is a subset of the oracle's set (checked slice
    by slice where the slice starts in front of cap), ranges and starts are clipped to cap, the words behind cap and
    the guard words keep their pattern.  cap is the true capacity of the buffer handed in."""
    lay = Layout(*BENCH)
    rng = np.random.default_rng(17)
    k = np.concatenate([random_keys(lay, rng, 5000), lay.tile_keys(3, [10, 11, 12])])
    n = len(np.unique(k))
    cap = 0 if below == "all" else n - below
    ukeys, ranges, starts, num, used = run_case(hp, lay, [k, k[: len(k) // 2]], cap=cap)
    assert used == cap and num[0] == cap
    assert ranges[0, :, 0].max() <= cap and starts[0].max() <= cap
    assert ranges[0, :, 1].sum() == n  # the counts are not clipped: the cursor advanced over every key


def test_bitmap_path_and_keyed_path_find_the_same_circles(hp):
    """End to end on two 512 x 512 planes: the keyed path's keys, decoded, are the bitmap path's circle list
    (k_layer_count / _scan / _emit), and both finders return the same circles and scores."""
    from synth import noisy_bead_image

    h = w = 512
    min_r, max_r, num_iter = 5, 25, 300000
    planes = np.stack([noisy_bead_image(21, (h, w), 40, r_lo=6, r_hi=22)[0],
                       noisy_bead_image(22, (h, w), 25, r_lo=8, r_hi=25)[0]])
    res = {}
    for keyed in (True, False):
        cf = hp.CircleFinder(2, h, w, min_r, max_r, num_iter)
        assert cf.keyed and cf.keyed_score
        cf.keyed, cf.keyed_score = keyed, keyed
        cf.keep_debug_maps = True
        out, _ = cf.find(torch.from_numpy(planes).cuda(), None, 0.1, 0.9, 0.3, 5, [3, 4])
        res[keyed] = (cf, out)
    ck, cb = res[True][0], res[False][0]
    ntc = (w + 2 * max_r + TS - 1) // TS
    nk, nb = ck.num_circles.cpu().numpy(), cb.num_circles.cpu().numpy()
    np.testing.assert_array_equal(nk, nb)
    for p in range(2):
        assert nk[p] > 1000
        kk = np.sort(ck.unique_keys[p, : nk[p]].cpu().numpy().view(np.uint32))
        tile = (kk >> 17).astype(np.int64)
        dec = np.stack([(tile // ntc) * TS + ((kk >> 6) & 63) - max_r, (tile % ntc) * TS + (kk & 63) - max_r,
                        min_r + ((kk >> 12) & 31)], axis=1)
        np.testing.assert_array_equal(dec, cb.circles[p, : nb[p]].cpu().numpy())
        assert len(res[True][1][p][0]) >= 3
        np.testing.assert_array_equal(res[True][1][p][0], res[False][1][p][0])
        np.testing.assert_array_equal(res[True][1][p][1].view(np.uint32), res[False][1][p][1].view(np.uint32))
