"""The flat-field correction (preprocess.py:83-87) restated in plain NumPy float64, and the fixtures that take the
device passes to their margins.  No GPU, no library: tests/test_cpu_flatfield_ref.py holds every fixture to the
condition it was built for, tests/test_gpu_flatfield_limits.py runs them.

    t = clip(x - dark, 0);  M1 = max t;  M2 = max (t / flat);  out = (((t / flat) * M1) / M2).astype(dtype)

`maxima` is pass 1 (one pair per group of tiles), `correct` pass 2 with the maxima it is given -- the device pass takes
a caller's maxima too, so any pair can be put in.  `representable` marks the pixels whose float64 result NumPy casts to
an integer the same way everywhere: finite and inside [0, dtype max]; the cast of NaN, of a negative or of a larger
value is the platform's.

Fixtures: `all_values_tile` (every pixel value once), `ratio_flat` (bands of flat values whose reciprocal is not a
float64: 3, 5, 7, 0.75, 1.5, ...), `near_tie_pairs` (two pixels whose exact quotients differ by a chosen relative gap, down
to nothing) and the scenes built from them.  `naive_wrong` simulates pass 2 WITHOUT its switch to the exact path: where
floor(t * (r * M1 / M2)) with a reciprocal r one ulp around 1 / flat is not the reference's truncation."""
import functools

import numpy as np

from synth import vignette

# ---- the reference ----------------------------------------------------------------------------------------------------


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def dark_subtracted(tiles, dark):
    with np.errstate(all="ignore"):
        return np.clip(np.asarray(tiles).astype(np.float64) - _f64(dark), 0, None)


def maxima(tiles, flat, dark, n_groups):
    """(n_groups, 2) float64 [M1, M2] of `n_groups` equal blocks of tiles (..., ty, tx) along the leading axes, with
    NumPy's own NaN and inf semantics: a NaN quotient (0 / 0, a NaN flat, a NaN pixel) makes the group's M2 NaN."""
    ty, tx = tiles.shape[-2:]
    with np.errstate(all="ignore"):
        t = dark_subtracted(tiles, dark).reshape(n_groups, -1, ty, tx)
        q = t / _f64(flat)
        return np.stack([t.max(axis=(1, 2, 3)), q.max(axis=(1, 2, 3))], axis=1)


def correct_f64(tiles, flat, dark, max2, planes_per_group):
    """((t / flat) * M1) / M2 in that order, before the cast: tiles (C, T, R, Cc, ty, tx), plane p = c T + t takes the
    maxima of group p // planes_per_group."""
    c, t, _, _, _, _ = tiles.shape
    max2 = _f64(max2).reshape(-1, 2)
    assert (c * t) % planes_per_group == 0 and len(max2) == (c * t) // planes_per_group
    group = np.arange(c * t) // planes_per_group
    m1 = max2[group, 0].reshape(c, t, 1, 1, 1, 1)
    m2 = max2[group, 1].reshape(c, t, 1, 1, 1, 1)
    with np.errstate(all="ignore"):
        return ((dark_subtracted(tiles, dark) / _f64(flat)) * m1) / m2


def correct(tiles, flat, dark, max2, planes_per_group):
    with np.errstate(all="ignore"):
        return correct_f64(tiles, flat, dark, max2, planes_per_group).astype(tiles.dtype)


def representable(tiles, flat, dark, max2, planes_per_group):
    """Where `correct`'s cast is defined by NumPy on every platform: all of a floating point type; of an integer type
    the pixels whose float64 value is finite and inside [0, dtype max]."""
    v = correct_f64(tiles, flat, dark, max2, planes_per_group)
    if tiles.dtype.kind == "f":
        return np.ones(v.shape, dtype=bool)
    with np.errstate(all="ignore"):
        return np.isfinite(v) & (v >= 0) & (v <= np.iinfo(tiles.dtype).max)


def same_maxima(a, b):
    """Bit for bit, NaN included.  Any NaN stands for any other: 0 / 0 is the negative quiet NaN on x86 and the
    positive one on the device, and which of a group's NaNs numpy.max hands back is its reduction order's choice."""
    a, b = _f64(a), _f64(b)
    canon = lambda x: np.where(np.isnan(x), np.float64(np.nan), x).tobytes()  # noqa: E731
    return a.shape == b.shape and canon(a) == canon(b)


# ---- pass 2: every pixel value against flats with inexact reciprocals -------------------------------------------------
RATIO_FLATS = (3.0, 5.0, 7.0, 0.75, 1.5, 1.0, 0.5, float(np.float32(0.6)))
SWITCH_FLATS = RATIO_FLATS[:5]  # flats whose reciprocal is no float64: where the simulation counts wrong truncations
# maxima the device tests supply: the four the suite has to have, then M2 = M1 / fl for the flats 0.75, 1.5 and 5 -- with
# (60000, 20000) for the flat of 3 the pairs at which the correctly rounded reciprocal alone truncates wrongly
SWITCH_MAX2 = ((60000.0, 60000.0), (60000.0, 20000.0), (4095.0, 5118.75), (65535.0, 21845.0),
               (60000.0, 80000.0), (60000.0, 40000.0), (60000.0, 12000.0))


def all_values_tile(dtype):
    """256 x 256 uint16 / 16 x 16 uint8 holding every value of the type once, in a fixed permutation."""
    n = np.iinfo(dtype).max + 1
    side = int(round(n ** 0.5))
    assert side * side == n
    return np.random.default_rng(65535).permutation(n).astype(dtype).reshape(side, side)


def band_rows(h):
    """Row ranges of the nine bands of `ratio_flat`: eight of h // 9 rows, the vignette band takes the rest."""
    b = h // 9
    return [(i * b, (i + 1) * b) for i in range(8)] + [(8 * b, h)]


def ratio_flat(shape, dtype=np.float32):
    flat = vignette(shape, dtype=dtype)
    for (lo, hi), value in zip(band_rows(shape[0]), RATIO_FLATS):
        flat[lo:hi] = value
    return flat


def all_values_tiles(dtype, n_planes, grid=(2, 2)):
    """(n_planes, 1, R, Cc, side, side): the all-values tile, every tile rolled down by another multiple of a band's
    height, so that every pixel value meets every band of `ratio_flat` once there are eleven tiles."""
    base = all_values_tile(dtype)
    step = base.shape[0] // 9
    n = n_planes * grid[0] * grid[1]
    tiles = np.stack([np.roll(base, k * step, axis=0) for k in range(n)])
    return tiles.reshape((n_planes, 1) + grid + base.shape)


def naive_wrong(t, fl, m1, m2, r="rn"):
    """Where the fast product alone gets pass 2 wrong: floor(t * (r * (m1 / m2))) != trunc(((t / fl) * m1) / m2), for a
    reciprocal r of fl that is the correctly rounded 1 / fl ("rn"), the float64 below it ("prev") or above it ("next").
    Scalars or arrays that broadcast."""
    t, fl, m1, m2 = _f64(t), _f64(fl), _f64(m1), _f64(m2)
    with np.errstate(all="ignore"):
        rn = np.float64(1.0) / fl
        r = {"rn": rn, "prev": np.nextafter(rn, 0.0), "next": np.nextafter(rn, np.inf)}[r] if isinstance(r, str) else _f64(r)
        want = np.trunc(((t / fl) * m1) / m2)
        return np.floor(t * (r * (m1 / m2))) != want


def at_risk(tiles, flat, dark, max2, planes_per_group, r="rn"):
    """`naive_wrong` for every pixel of tiles (C, T, R, Cc, ty, tx) with its own flat and its group's maxima, where the
    reference value is representable: the pixels only the switch gets right."""
    c, t, _, _, _, _ = tiles.shape
    max2 = _f64(max2).reshape(-1, 2)
    group = np.arange(c * t) // planes_per_group
    m1 = max2[group, 0].reshape(c, t, 1, 1, 1, 1)
    m2 = max2[group, 1].reshape(c, t, 1, 1, 1, 1)
    return naive_wrong(dark_subtracted(tiles, dark), flat, m1, m2, r) & representable(tiles, flat, dark, max2, planes_per_group)


def distance_to_integer(t, fl, m1, m2):
    """|v - round(v)| of the reference's own float64 value v."""
    v = ((_f64(t) / np.float64(fl)) * np.float64(m1)) / np.float64(m2)
    return np.abs(v - np.rint(v))


# ---- special flat values ----------------------------------------------------------------------------------------------
F32_DENORMAL = np.float32(1e-40)
SPECIAL_FLATS = np.array([0.0, -1.0, np.nan, np.inf, F32_DENORMAL, np.float32(1e-30), np.float32(1e30), np.float32(2e-30)],
                         dtype=np.float32)
assert 0 < F32_DENORMAL < np.finfo(np.float32).tiny
ZERO, MINUS, NAN, INF, DENORMAL, TINY, HUGE, TWO_TINY = range(8)
# Which specials a flat image holds, and under which pixels: "dark" = a row of them under pixels at or below the dark
# level (t == 0), "above" = a second row under pixels above it.  "all" is the case the suite has to have -- 0 / 0, t / 0
# and a NaN flat, M2 = NaN in every group; a NaN hides everything else, so the other cases drop the specials with the
# largest quotients one after the other: M2 = inf (t / 0), t / denormal, t / 1e-30f (the exact division: out of range),
# t / 2e-30f (in range: the float32 filters run, no threshold holds above 1e30), an ordinary maximum.
SPECIAL_CASES = {
    "all": (tuple(range(8)), ("dark", "above")),
    "zero": ((ZERO, MINUS, INF, DENORMAL, TINY, HUGE, TWO_TINY), ("above",)),
    "denormal": ((MINUS, INF, DENORMAL, TINY, HUGE, TWO_TINY), ("dark", "above")),
    "tiny": ((MINUS, INF, TINY, HUGE, TWO_TINY), ("dark", "above")),
    "two_tiny": ((MINUS, INF, HUGE, TWO_TINY), ("dark", "above")),
    "small": ((MINUS, INF, HUGE), ("dark", "above")),
}
SPECIAL_SHAPE = (32, 128)


def special_positions(shape, subset, rows):
    """[(y, x, index into SPECIAL_FLATS, row kind)]: sixteen pixels apart (each special in a 16-byte chunk of ordinary
    values whatever the pixel type), the "dark" row near the top, the "above" row near the bottom."""
    h, w = shape
    assert w >= 16 * len(SPECIAL_FLATS) and h >= 4
    return [(1 if kind == "dark" else h - 2, 16 * k + (3 if kind == "dark" else 5), k, kind) for kind in rows for k in subset]


def special_scene(dtype, dark, case, n_groups=3, tiles_per_group=5, shape=SPECIAL_SHAPE, flat_dtype=np.float32, seed=7):
    """Tiles (n_groups, tiles_per_group, ty, tx) over the type's whole range and a flat image in [0.6, 1.4) with the
    specials of SPECIAL_CASES[case] planted (a float64 flat holds the float32 values: its denormal is an ordinary
    float64).  Groups 0 and 2 have pixels at or below the dark level under the "dark" row and above it under the
    "above" row; group 1 is at or below the dark level under every special.  Returns (tiles, flat, positions)."""
    rng = np.random.default_rng(seed)
    kind = np.dtype(dtype).kind
    top = np.iinfo(dtype).max if kind == "u" else 60000
    level = max(int(np.floor(dark)), 0)
    assert level + 1 < top
    tiles = rng.integers(0, top + 1, size=(n_groups, tiles_per_group) + shape).astype(dtype)
    flat = (0.6 + 0.8 * rng.random(shape)).astype(flat_dtype)
    where = special_positions(shape, *SPECIAL_CASES[case])
    for y, x, k, row in where:
        flat[y, x] = SPECIAL_FLATS[k]
        lo, hi = (0, level + 1) if row == "dark" else (level + 1, top + 1)
        tiles[:, :, y, x] = rng.integers(lo, hi, size=(n_groups, tiles_per_group)).astype(dtype)
        tiles[1, :, y, x] = rng.integers(0, level + 1, size=tiles_per_group).astype(dtype)
    return tiles, flat, where


# ---- pass 1: near-ties -------------------------------------------------------------------------------------------------
GAP_BANDS = {"tie": (0.0, 0.0), "1e-10": (0.0, 1e-10), "1e-9": (1e-9, 1e-8), "5e-8": (5e-8, 5e-7), "2e-6": (2e-6, 8e-6),
             "2e-5": (2e-5, 1e-4)}
PLACEMENTS = ("chunk", "tiles", "ends")
ORDERS = ("lower_first", "higher_first")
N_CANDIDATES = 1_000_000


def gap_bands(dtype_name):
    """The bands of relative gap a pair is planted for.  uint8 pixels against float32 flats have no pair in (0, 1e-10]:
    two quotients t1 / f1 != t2 / f2 with t <= 255 and 24-bit flats differ by at least 1 / (255 2^24 2) = 1.2e-10 of
    themselves (a ratio of integers below 2^33), 3.8e-10 with the dark level of 100 taken off -- their smallest band is
    (0, 1e-9]."""
    bands = dict(GAP_BANDS)
    if dtype_name == "uint8":
        bands["1e-10"] = (0.0, 1e-9)
    return bands
STAIRS = 8


def rel_gap(qa, qb):
    return (qb - qa) / qb


@functools.lru_cache(maxsize=None)
def _candidates(dtype_name, dark, seed=20240611):
    """N_CANDIDATES candidates (x, fl), sorted by their float64 quotient max(x - dark, 0) / fl: x over the upper three quarters
    of the pixel type's range (so that the rest of a scene fits under half the planted maximum), fl float32 in [0.5, 2)
    -- three in four uniform, one in four a multiple of 1 / 64, without which no two quotients are equal."""
    rng = np.random.default_rng(seed)
    top, n = np.iinfo(dtype_name).max, N_CANDIDATES
    x = rng.integers(max(top // 4, int(dark)) + 1, top, size=n)  # (below the type's maximum: a larger decoy pixel exists)
    fl = (0.5 + 1.5 * rng.random(n)).astype(np.float32)
    coarse = rng.random(n) < 0.25
    fl[coarse] = (rng.integers(32, 128, size=int(coarse.sum())) / 64.0).astype(np.float32)
    fl = np.minimum(fl, np.nextafter(np.float32(2.0), np.float32(0.0)))
    q = np.clip(x.astype(np.float64) - dark, 0, None) / fl.astype(np.float64)
    keep = q > 0
    x, fl, q = x[keep], fl[keep], q[keep]
    order = np.argsort(q, kind="stable")
    return x[order], fl[order], q[order]


@functools.lru_cache(maxsize=None)
def near_tie_pairs(dtype_name, dark):
    """{band: ((xa, fla), (xb, flb))} with quotients qa <= qb whose relative gap (qb - qa) / qb lies in the band:
    "tie" is qa == qb from two different candidates, "1e-10" is 0 < gap <= 1e-10 (`gap_bands`).  Of the pairs found, the one with
    the largest quotient."""
    x, fl, q = _candidates(dtype_name, dark)
    out = {}
    for band, (lo, hi) in gap_bands(dtype_name).items():
        if band in ("tie", "1e-10"):
            j = np.arange(1, len(q))
        else:
            j = np.searchsorted(q, q[:-1] * (1.0 + np.sqrt(lo * hi)))
        i = np.arange(len(q) - 1)
        ok = j < len(q)
        i, j = i[ok], j[ok]
        gap = rel_gap(q[i], q[j])
        hit = (gap == 0) & ((x[i] != x[j]) | (fl[i] != fl[j])) if band == "tie" else (gap > 0) & (gap >= lo) & (gap <= hi)
        if band == "tie":
            hit &= x[i] != x[j]  # two different pixels on two different flats
        found = np.flatnonzero(hit)
        if len(found) == 0:
            continue
        k = found[-1]
        out[band] = ((int(x[i[k]]), fl[i[k]]), (int(x[j[k]]), fl[j[k]]))
    return out


@functools.lru_cache(maxsize=None)
def staircase(dtype_name, dark):
    """STAIRS candidates [(x, fl)], each quotient [2e-6, 8e-6] above the last, from the ninth decile of the
    candidates' quotients on (the very top of the range is too thinly set for such steps)."""
    x, fl, q = _candidates(dtype_name, dark)
    lo, hi = GAP_BANDS["2e-6"]
    for start in range(len(q) * 9 // 10, len(q)):  # (a step's window is empty once in a while: start one further up)
        steps = [start]
        while len(steps) < STAIRS:
            i = steps[-1]
            j = int(np.searchsorted(q, q[i] * (1.0 + 1.25 * lo)))
            if j >= len(q) or not lo <= rel_gap(q[i], q[j]) <= hi:
                break
            steps.append(j)
        if len(steps) == STAIRS:
            break
    assert len(steps) == STAIRS, "no staircase in the band"
    return [(int(x[i]), fl[i]) for i in steps]


TIE_SHAPE = (32, 64)
TIE_TILES = 6
DECOY_FLAT = np.float32(8.0)


def _quotient(x, fl, dark):
    return max(float(x) - dark, 0.0) / float(fl)


def _background(rng, dtype, dark, q_top, n_groups, tiles_per_group, shape):
    """Pixels and flats whose quotients stay at or below q_top / 2: flats in [0.5, 2), t <= q_top / 4."""
    t_max = int(np.floor(q_top / 4.0))
    hi = int(np.floor(dark)) + t_max  # x - dark <= t_max
    assert t_max >= 1 and hi >= 1
    px = rng.integers(0, hi + 1, size=(n_groups, tiles_per_group) + shape)
    flat = (0.5 + 1.5 * rng.random(shape)).astype(np.float32)
    return px.astype(dtype), flat


def near_tie_scene(dtype, dark, band, order, placement, n_groups=3, tiles_per_group=TIE_TILES, shape=TIE_SHAPE):
    """Tiles (n_groups, tiles_per_group, ty, tx) of `dtype` and a float32 flat image in which group 1's maximum
    quotient is decided between the two pixels of a near-tie pair; every other quotient of that group is at most half
    of it.  placement "chunk": both in one 16-byte chunk of uint16 pixels (8 pixels; one chunk or neighbouring ones of
    the other types); "tiles": the same chunk of tiles 0 and 5; "ends": the first and the last chunk of tile 2.
    order: which of the two the kernels meet first (lower element, lower tile, lower chunk).  For integer pixels the
    chunk of the pixel met second also holds a decoy: that chunk's LARGEST pixel, on a flat of 8, so that its quotient
    is small -- the chunk's maximum quotient comes from the smaller pixel on the smaller flat.  Group 0 has a brighter
    pixel than the pair, group 2 only the background (a single group holds the pair; "tiles" is then its first and
    its last tile).  Returns (tiles, flat, info)."""
    dtype = np.dtype(dtype)
    int_name = dtype.name if dtype.kind == "u" else "uint16"
    (xa, fla), (xb, flb) = near_tie_pairs(int_name, dark)[band]
    first, second = ((xa, fla), (xb, flb)) if order == "lower_first" else ((xb, flb), (xa, fla))
    ty, tx = shape
    elems = ty * tx
    group = min(1, n_groups - 1)
    rng = np.random.default_rng(sum(map(ord, int_name + band + order + placement)))
    tiles, flat = _background(rng, dtype, dark, _quotient(xa, fla, dark), n_groups, tiles_per_group, shape)
    c0 = 8 * 37  # a chunk in the middle of the tile (uint16 chunks of 8 pixels)
    if placement == "chunk":
        spots = [(2, c0 + 1), (2, c0 + 2)]
    elif placement == "tiles":
        spots = [(0, c0 + 1), (tiles_per_group - 1, c0 + 2)]
    else:
        spots = [(2, 1), (2, elems - 2)]
    flat_v, tiles_v = flat.reshape(-1), tiles.reshape(n_groups, tiles_per_group, elems)
    for (tile, p), (x, fl) in zip(spots, (first, second)):
        flat_v[p] = fl
        tiles_v[group, tile, p] = x
    decoy = None
    if dtype.kind == "u":
        tile, p = spots[1]
        decoy = (tile, p + 3 if placement != "ends" else p - 3)
        flat_v[decoy[1]] = DECOY_FLAT
        tiles_v[group, decoy[0], decoy[1]] = max(xa, xb) + 1
    if n_groups > 1:
        tiles_v[0, 3, 8 * 11 + 5] = np.iinfo(int_name).max  # group 0: a brighter pixel than the pair, on a background flat
    info = dict(pair=((xa, fla), (xb, flb)), spots=spots, decoy=decoy, group=group)
    return tiles, flat, info


def staircase_scene(dtype, dark, n_groups=3, tiles_per_group=TIE_TILES, shape=TIE_SHAPE):
    """The same background with STAIRS rising pixels in group 1: pixel k of chunk c0 in tile k for the first six, then
    the first two pixels of the neighbour chunk in the last tile."""
    dtype = np.dtype(dtype)
    int_name = dtype.name if dtype.kind == "u" else "uint16"
    steps = staircase(int_name, dark)
    rng = np.random.default_rng(99)
    tiles, flat = _background(rng, dtype, dark, _quotient(*steps[0], dark), n_groups, tiles_per_group, shape)
    elems = shape[0] * shape[1]
    c0 = 8 * 37
    assert tiles_per_group == TIE_TILES
    spots = [(k, c0 + k) for k in range(tiles_per_group)] + [(tiles_per_group - 1, c0 + 8 + k) for k in range(STAIRS - tiles_per_group)]
    flat_v, tiles_v = flat.reshape(-1), tiles.reshape(n_groups, tiles_per_group, elems)
    for (tile, p), (x, fl) in zip(spots, steps):
        flat_v[p] = fl
        tiles_v[1, tile, p] = x
    tiles_v[0, 3, 8 * 11 + 5] = np.iinfo(int_name).max
    return tiles, flat, dict(steps=steps, spots=spots, group=1)


def quotients(tiles, flat, dark):
    with np.errstate(all="ignore"):
        return dark_subtracted(tiles, dark) / _f64(flat)
