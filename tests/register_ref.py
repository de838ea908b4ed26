"""NumPy restatement of ``stitch(register="ncc")`` ("stitch: registration by seam cross-correlation"),
independent of magnify_amd/register.py.

Tiles (ty, tx) on an R x Cc grid, overlap v, clip = v // 2, kept size hy = ty - v, hx = tx - v, m = max_shift.
``e[r, c] = (ey, ex)``: pixel q of tile (r, c) shows the scene point ``nominal origin + e + q``.

Seams: (r, c) | (r, c + 1) at index r (Cc - 1) + c, then (r, c) | (r + 1, c) at R (Cc - 1) + r Cc + c; A is the first
tile, B the second.  Patch (in B): rows [m, ty - m), columns [m, v - m), offset o = (0, tx - v) for the first kind;
rows [m, v - m), columns [m, tx - m), o = (ty - v, 0) for the second.  B[q] meets A[q + o + delta], delta in [-m, m]^2.
Sums: fixed = [n, sum B, sum B^2]; per delta [sum A, sum A^2, sum A B] (int64 for integer pixels, float64 else).
Score z = (n sAB - sA sB) / sqrt((n sAA - sA^2)(n sBB - sB^2)) in float64, 0 where a variance term is <= 0 or z is not
finite.  Pick: largest z, ties to the smallest dy^2 + dx^2, then dy, then dx.  A seam is used iff z >= min_score.
Solve per axis: minimum-norm least squares of e_B - e_A = delta over the used seams; per connected component subtract
the value at its first tile in raster order, round; subtract g = (min + max) // 2 of the component; clip to
[-clip, clip].  Registered stitch: tile'[y, x] = value[clamp(y - ey), clamp(x - ex)], then blend_ref.plain / .blend.
"""
import numpy as np

import blend_ref as br


def seams(R, Cc):
    out = []
    for r in range(R):
        for c in range(Cc - 1):
            out.append(((r, c), (r, c + 1)))
    for r in range(R - 1):
        for c in range(Cc):
            out.append(((r, c), (r + 1, c)))
    return out


def patch(kind_horizontal, ty, tx, v, m):
    """(rows, columns of the patch in B, offset of A)."""
    if kind_horizontal:
        return (m, ty - m), (m, v - m), (0, tx - v)
    return (m, v - m), (m, tx - m), (ty - v, 0)


def seam_sums(plane, v, m):
    """plane (R, Cc, ty, tx) -> sums (n_seams, 2m + 1, 2m + 1, 3), fixed (n_seams, 3), and for float pixels the sums of
    the terms' magnitudes (same shapes) that scale the error bound; None for integer pixels."""
    R, Cc, ty, tx = plane.shape
    integer = plane.dtype.kind == "u"
    acc = np.int64 if integer else np.float64
    w = 2 * m + 1
    pairs = seams(R, Cc)
    sums = np.zeros((len(pairs), w, w, 3), dtype=acc)
    fixed = np.zeros((len(pairs), 3), dtype=acc)
    mag = None if integer else np.zeros_like(sums)
    fmag = None if integer else np.zeros_like(fixed)
    for s, (a, b) in enumerate(pairs):
        (y0, y1), (x0, x1), (oy, ox) = patch(a[0] == b[0], ty, tx, v, m)
        A, B = plane[a].astype(acc), plane[b][y0:y1, x0:x1].astype(acc)
        fixed[s] = [B.size, B.sum(), (B * B).sum()]
        if not integer:
            fmag[s] = [0, np.abs(B).sum(), (B * B).sum()]
        for dy in range(-m, m + 1):
            for dx in range(-m, m + 1):
                Ad = A[y0 + oy + dy:y1 + oy + dy, x0 + ox + dx:x1 + ox + dx]
                assert Ad.shape == B.shape
                sums[s, dy + m, dx + m] = [Ad.sum(), (Ad * Ad).sum(), (Ad * B).sum()]
                if not integer:
                    mag[s, dy + m, dx + m] = [np.abs(Ad).sum(), (Ad * Ad).sum(), np.abs(Ad * B).sum()]
    return sums, fixed, mag, fmag


def scores(sums, fixed):
    """(n_seams, 2m + 1, 2m + 1) float64."""
    z = np.zeros(sums.shape[:-1], dtype=np.float64)
    for s in range(sums.shape[0]):
        n, sb, sbb = (np.float64(x) for x in fixed[s])
        vb = n * sbb - sb * sb
        for i in range(sums.shape[1]):
            for j in range(sums.shape[2]):
                sa, saa, sab = (np.float64(x) for x in sums[s, i, j])
                va = n * saa - sa * sa
                with np.errstate(all="ignore"):
                    val = (n * sab - sa * sb) / np.sqrt(va * vb)
                z[s, i, j] = val if (va > 0 and vb > 0 and np.isfinite(val)) else 0.0
    return z


def pick(z):
    """(delta (n_seams, 2), best (n_seams,)): plain loops, the tie-break written out."""
    m = (z.shape[-1] - 1) // 2
    delta, best = np.zeros((z.shape[0], 2), dtype=np.int64), np.zeros(z.shape[0])
    for s in range(z.shape[0]):
        key = None
        for dy in range(-m, m + 1):
            for dx in range(-m, m + 1):
                k = (-z[s, dy + m, dx + m], dy * dy + dx * dx, dy, dx)
                if key is None or k < key:
                    key = k
        delta[s], best[s] = (key[2], key[3]), -key[0]
    return delta, best


def solve(R, Cc, delta, best, min_score, clip):
    """(shift (R, Cc, 2) int, used (n_seams,) bool, clipped entries)."""
    pairs = seams(R, Cc)
    used = np.array([best[s] >= min_score for s in range(len(pairs))], dtype=bool)
    idx = lambda rc: rc[0] * Cc + rc[1]  # noqa: E731
    n = R * Cc
    # components by flood fill over the used seams, in raster order
    comp = [-1] * n
    for start in range(n):
        if comp[start] >= 0:
            continue
        comp[start], stack = start, [start]
        while stack:
            node = stack.pop()
            for s, (a, b) in enumerate(pairs):
                if used[s] and node in (idx(a), idx(b)):
                    other = idx(b) if node == idx(a) else idx(a)
                    if comp[other] < 0:
                        comp[other] = start
                        stack.append(other)
    shift = np.zeros((n, 2), dtype=np.int64)
    rows = [s for s in range(len(pairs)) if used[s]]
    if rows:
        M = np.zeros((len(rows), n))
        for i, s in enumerate(rows):
            M[i, idx(pairs[s][1])], M[i, idx(pairs[s][0])] = 1.0, -1.0
        for axis in range(2):
            sol = np.linalg.lstsq(M, np.asarray([delta[s][axis] for s in rows], dtype=np.float64), rcond=None)[0]
            for first in sorted(set(comp)):
                members = [i for i in range(n) if comp[i] == first]
                vals = [int(np.rint(sol[i] - sol[first])) for i in members]
                g = (min(vals) + max(vals)) // 2
                for i, val in zip(members, vals):
                    shift[i, axis] = val - g
    clipped = np.clip(shift, -clip, clip)
    return clipped.reshape(R, Cc, 2), used, int((clipped != shift).sum())


def register(plane, v, m, min_score=0.5):
    """plane (R, Cc, ty, tx) -> (shift (R, Cc, 2), delta, best, used, clipped)."""
    sums, fixed, _, _ = seam_sums(plane, v, m)
    delta, best = pick(scores(sums, fixed))
    shift, used, clipped = solve(plane.shape[0], plane.shape[1], delta, best, min_score, v // 2)
    return shift, delta, best, used, clipped


def shift_tiles(values, shifts):
    """values (..., R, Cc, ty, tx), shifts (R, Cc, 2): tile'[y, x] = value[clamp(y - ey), clamp(x - ex)]."""
    values = np.asarray(values)
    R, Cc, ty, tx = values.shape[-4:]
    out = np.empty_like(values)
    for r in range(R):
        for c in range(Cc):
            ey, ex = (int(x) for x in shifts[r, c])
            yy = np.clip(np.arange(ty) - ey, 0, ty - 1)
            xx = np.clip(np.arange(tx) - ex, 0, tx - 1)
            out[..., r, c, :, :] = values[..., r, c, :, :][..., yy[:, None], xx[None, :]]
    return out


def stitch(values, v, shifts, blend=None):
    """Shift every tile, then the plain stitch or the linear blend of blend_ref."""
    moved = shift_tiles(values, shifts)
    return br.plain(moved, v) if blend is None else br.blend(moved, v)


def cut_jittered(scene, R, Cc, ty, tx, v, e, pad):
    """Tiles (..., R, Cc, ty, tx): tile (r, c) cut from ``scene`` at pad + (r hy, c hx) + e[r, c]."""
    hy, hx = ty - v, tx - v
    out = np.empty(scene.shape[:-2] + (R, Cc, ty, tx), dtype=scene.dtype)
    for r in range(R):
        for c in range(Cc):
            y, x = pad + r * hy + int(e[r, c, 0]), pad + c * hx + int(e[r, c, 1])
            assert 0 <= y and y + ty <= scene.shape[-2] and 0 <= x and x + tx <= scene.shape[-1]
            out[..., r, c, :, :] = scene[..., y:y + ty, x:x + tx]
    return out


def expected_table(e):
    """The table a connected grid is solved to: e - e[0, 0] - g, g = (min + max) // 2 per axis; and g."""
    rel = np.asarray(e, dtype=np.int64) - np.asarray(e[0, 0], dtype=np.int64)
    g = (rel.min(axis=(0, 1)) + rel.max(axis=(0, 1))) // 2
    return rel - g, g


def scene_crop(scene, R, Cc, ty, tx, v, pad, e00, g):
    """What the registered stitch shows: the scene from pad + clip + e[0, 0] + g on, (R hy, C hx) pixels."""
    hy, hx, clip = ty - v, tx - v, v // 2
    y, x = pad + clip + int(e00[0]) + int(g[0]), pad + clip + int(e00[1]) + int(g[1])
    return scene[..., y:y + R * hy, x:x + Cc * hx]


def draw_errors(rng, R, Cc, m):
    """e (R, Cc, 2) with |e| <= m // 2: neighbours then differ by at most m, the search window."""
    return rng.integers(-(m // 2), m // 2 + 1, size=(R, Cc, 2))
