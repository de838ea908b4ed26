"""NumPy restatement of ``stitch(blend="linear")`` ("stitch: linear overlap blending"), from the values the
plain stitch writes for every tile.

Per axis: tile length t, overlap v, c = v // 2, r = v % 2, h = t - v, n tiles.  Canvas coordinate o in [0, n h), owner
tile i = o // h, j = o - i h, local coordinate p = j + c.
  * v > 0, i > 0 and j < c + r: k = j + c; tile i at p has numerator 2k + 1, tile i - 1 at p + h has 2v - (2k + 1);
  * else v > 0, i < n - 1 and j >= h - c: k = j - (h - c); tile i at p has 2v - (2k + 1), tile i + 1 at p - h has 2k + 1;
  * else tile i alone, numerator 2v.
Integer pixels: (sum of ny nx value + D // 2) // D with D = (2v)^2, in uint64.  Float pixels, in float64: along x first
for each contributing row, a = c0 (nx0 / 2v) + c1 (nx1 / 2v), then the rows the same way along y, then the cast; a
term without a second tile is not formed.
"""
import numpy as np


def axis_terms(n, t, v):
    """Per canvas coordinate of one axis: owner tile, local coordinate, the other tile (-1: none), its local
    coordinate (0 where none) and the owner's numerator."""
    if v < 0 or 2 * v > t:
        raise ValueError(f"2 * overlap ({v}) must not exceed the tile length ({t})")
    c, r, h = v // 2, v % 2, t - v
    o = np.arange(n * h)
    i = o // h
    j = o - i * h
    p = j + c
    other = np.full(n * h, -1)
    p_other = np.zeros(n * h, dtype=np.int64)
    num = np.full(n * h, 2 * v, dtype=np.int64)
    if v > 0:
        before = (i > 0) & (j < c + r)
        k = j + c
        num[before] = 2 * k[before] + 1
        other[before] = i[before] - 1
        p_other[before] = p[before] + h
        after = ~before & (i < n - 1) & (j >= h - c)
        k = j - (h - c)
        num[after] = 2 * v - (2 * k[after] + 1)
        other[after] = i[after] + 1
        p_other[after] = p[after] - h
    return i, p, other, p_other, num


def plain(tiles, v):
    """The crop / concat of the plain stitch: tiles (..., R, C, ty, tx) -> (..., R hy, C hx)."""
    tiles = np.asarray(tiles)
    R, C, ty, tx = tiles.shape[-4:]
    c, r = v // 2, v % 2
    kept = tiles[..., c : ty - c - r, c : tx - c - r]
    hy, hx = kept.shape[-2:]
    return np.moveaxis(kept, -3, -2).reshape(tiles.shape[:-4] + (R * hy, C * hx))


def _terms(tiles, v):
    R, C, ty, tx = tiles.shape[-4:]
    iy, py, oy, qy, ny = axis_terms(R, ty, v)
    ix, px, ox, qx, nx = axis_terms(C, tx, v)
    has_y, has_x = (oy >= 0)[:, None], (ox >= 0)[None, :]
    oy, ox = np.maximum(oy, 0), np.maximum(ox, 0)  # (gathered where there is no second tile too, then not used)
    at = lambda ti, pi, tj, pj: tiles[..., ti[:, None], tj[None, :], pi[:, None], pj[None, :]]  # noqa: E731
    values = at(iy, py, ix, px), at(iy, py, ox, qx), at(oy, qy, ix, px), at(oy, qy, ox, qx)
    return values, has_y, has_x, ny[:, None], nx[None, :]


def blend(tiles, v):
    """tiles (..., R, C, ty, tx): what the plain stitch writes for every tile's pixels -> the blended image."""
    tiles = np.asarray(tiles)
    (c00, c01, c10, c11), has_y, has_x, ny, nx = _terms(tiles, v)
    if v == 0:
        return c00.copy()
    if tiles.dtype.kind == "u":
        u = lambda a: np.asarray(a).astype(np.uint64)  # noqa: E731
        two_v = np.uint64(2 * v)
        D = two_v * two_v
        ny0, nx0 = u(ny), u(nx)
        ny1, nx1 = two_v - ny0, two_v - nx0
        acc = ny0 * nx0 * u(c00) + ny0 * nx1 * u(c01) * u(has_x) + ny1 * nx0 * u(c10) * u(has_y) \
            + ny1 * nx1 * u(c11) * u(has_x & has_y)
        assert acc.dtype == np.uint64
        return ((acc + D // np.uint64(2)) // D).astype(tiles.dtype)
    d = np.float64(2 * v)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    with np.errstate(all="ignore"):
        wx0, wx1 = f(nx) / d, f(2 * v - nx) / d
        a0 = np.where(has_x, f(c00) * wx0 + f(c01) * wx1, f(c00))
        a1 = np.where(has_x, f(c10) * wx0 + f(c11) * wx1, f(c10))
        out = np.where(has_y, a0 * (f(ny) / d) + a1 * (f(2 * v - ny) / d), a0)
        return out.astype(tiles.dtype)


def contributing_max(tiles, v):
    """max |value| over the tiles that contribute to each pixel (the scale of the float tolerance)."""
    (c00, c01, c10, c11), has_y, has_x, _, _ = _terms(np.asarray(tiles), v)
    z = np.float64(0)
    a = lambda c: np.abs(c.astype(np.float64))  # noqa: E731
    return np.maximum.reduce([a(c00), np.where(has_x, a(c01), z), np.where(has_y, a(c10), z),
                              np.where(has_x & has_y, a(c11), z)])


def band_mask(R, C, ty, tx, v):
    """(R hy, C hx) bool: the pixels that lie in a row band or a column band."""
    _, _, oy, _, _ = axis_terms(R, ty, v)
    _, _, ox, _, _ = axis_terms(C, tx, v)
    return (oy >= 0)[:, None] | (ox >= 0)[None, :]


def cut_tiles(scene, R, C, ty, tx, v):
    """Tiles (..., R, C, ty, tx) cut from one scene (..., R h + v, C h + v) with a stride of t - v: consistent tiles."""
    hy, hx = ty - v, tx - v
    out = np.empty(scene.shape[:-2] + (R, C, ty, tx), dtype=scene.dtype)
    for a in range(R):
        for b in range(C):
            out[..., a, b, :, :] = scene[..., a * hy : a * hy + ty, b * hx : b * hx + tx]
    return out
