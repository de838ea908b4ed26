"""NumPy restatement of ``magnify_amd.plot``: the label map of the foreground masks in image
coordinates and the composite picture.  The kernels (csrc/mg_overview.hip) are held to it bit for bit; it is itself
held to plain loops and to the reference's own label loop by tests/test_cpu_plot.py.  Everything runs in float64, one
operation at a time.  Below ``s = 2**level``, ``hk = ceil(H / s)``, ``wk = ceil(W / s)``."""
import math

import numpy as np

MARK_COLORS = np.array([(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
                        (70, 240, 240), (240, 50, 230)], dtype=np.uint8)


def disk(L, cy, cx, r):
    yy, xx = np.mgrid[0:L, 0:L]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def scene(seed=0, h=96, w=96, L=40, n_t=2):
    """Five markers on an (h, w) image: one at a corner and one at an edge (their windows are pushed back into the
    image), two whose masks overlap, one with an empty mask; the masks of timepoint 1 differ from those of timepoint 0."""
    rng = np.random.default_rng(seed)
    x = np.array([3.7, 50.2, 60.9, 93.0, 30.5])[:, None] + np.array([0.0, 2.0])[None, :n_t]
    y = np.array([2.2, 48.8, 55.1, 40.6, 75.0])[:, None] + np.array([0.0, -3.0])[None, :n_t]
    fg = np.zeros((5, n_t, L, L), dtype=bool)
    for t in range(n_t):
        fg[0, t] = disk(L, 6, 5, 5 + t)
        fg[1, t] = disk(L, 20, 20, 12)
        fg[2, t] = disk(L, 18 + t, 19, 11)
        fg[3, t] = disk(L, 20, 33, 6) | (rng.random((L, L)) < 0.05)
    return x, y, fg  # (marker 4: empty)


def bounding_box(x, y, L, w, h):
    """(top, bottom, left, right) of the L x L window about (x, y), pushed back into the image (utils.py:60-80)."""
    def clamp(c, size):
        lo, hi = c - L // 2, c + -(L // -2)
        if lo < 0:
            lo, hi = 0, hi - lo
        if hi > size:
            lo, hi = lo - (hi - size), size
        return lo, hi

    top, bottom = clamp(int(y), h)
    left, right = clamp(int(x), w)
    return top, bottom, left, right


def origins(x, y, L, h, w):
    """(M, T, 2) int32 (top, left) of every marker's window: the truncating ``astype(int)`` of plot/image.py:88-89,
    then the box of :104-110."""
    xs, ys = np.asarray(x).astype(int), np.asarray(y).astype(int)
    out = np.zeros(xs.shape + (2,), dtype=np.int32)
    for i in range(xs.shape[0]):
        for t in range(xs.shape[1]):
            top, _, left, _ = bounding_box(xs[i, t], ys[i, t], L, w, h)
            out[i, t] = top, left
    return out


def image_labels(fg, origin, level, h, w):
    """fg (M, T, L, L) bool, origin (M, T, 2) -> int32 (T, hk, wk): every set pixel (ry, rx) of fg[i, t] claims
    ((top + ry) >> level, (left + rx) >> level) with i + 1; the largest claim wins.  Claims outside the image are
    dropped."""
    m, n_t = fg.shape[:2]
    s = 1 << level
    labels = np.zeros((n_t, -(h // -s), -(w // -s)), dtype=np.int32)
    for i in range(m):
        for t in range(n_t):
            ry, rx = np.nonzero(fg[i, t])
            yy, xx = origin[i, t, 0] + ry, origin[i, t, 1] + rx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            np.maximum.at(labels[t], (yy[ok] >> level, xx[ok] >> level), np.int32(i + 1))
    return labels


def block_sums(plane, level):
    """(sum, n) float64 (hk, wk) of the in-image pixels of every s x s block: the exact integer for integer pixels;
    float pixels are added in float64 row by row from the top, each row from the left."""
    h, w = plane.shape
    s = 1 << level
    hk, wk = -(h // -s), -(w // -s)
    inside = np.zeros((hk * s, wk * s), dtype=bool)
    inside[:h, :w] = True
    n = inside.reshape(hk, s, wk, s).sum(axis=(1, 3)).astype(np.float64)
    if plane.dtype.kind in "iu":
        padded = np.zeros((hk * s, wk * s), dtype=np.int64)
        padded[:h, :w] = plane
        return padded.reshape(hk, s, wk, s).sum(axis=(1, 3)).astype(np.float64), n
    padded = np.zeros((hk * s, wk * s), dtype=np.float64)
    padded[:h, :w] = plane
    total = np.zeros((hk, wk), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(s):
            for k in range(s):
                total = np.where(inside[r::s, k::s], total + padded[r::s, k::s], total)
    return total, n


def default_colors(n_c):
    if n_c == 1:
        return [(1.0, 1.0, 1.0)]
    if n_c == 2:
        return [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0)]
    cycle = [(0.0, 1.0, 1.0), (1.0, 1.0, 0.0), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    return [cycle[c % 6] for c in range(n_c)]


def default_level(h, w):
    for level in range(7):
        s = 1 << level
        if math.ceil(h / s) * math.ceil(w / s) <= 1024 ** 2:
            return level
    return 6


def color_table(n_marks, n_t, color_by="mark", valid=None):
    """(M, T, 3) uint8: the overlay colour of marker i at timepoint t."""
    if color_by == "mark":
        return np.ascontiguousarray(np.repeat(MARK_COLORS[np.arange(n_marks) % 8][:, None], n_t, axis=1))
    ok = np.ones((n_marks, n_t), dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(n_marks, n_t)
    return np.where(ok[..., None], np.array([0, 255, 0], dtype=np.uint8), np.array([255, 0, 0], dtype=np.uint8))


def overview(image, level, limits, colors, labels=None, table=None, overlay=None, alpha=0.7):
    """image (C, T, H, W) -> uint8 (T, hk, wk, 3): steps 1-6 of the contract.  ``labels`` (T, hk, wk) is the map of the
    same level, ``table`` (M, T, 3) uint8."""
    n_c, n_t, h, w = image.shape
    s = 1 << level
    hk, wk = -(h // -s), -(w // -s)
    acc = np.zeros((n_t, hk, wk, 3), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(n_c):
            lo, hi = np.float64(limits[c][0]), np.float64(limits[c][1])
            for t in range(n_t):
                total, n = block_sums(image[c, t], level)
                mean = total / n
                u = (mean - lo) / (hi - lo)
                u = np.where(np.isnan(u) | (u < 0) | (not hi > lo), 0.0, u)
                u = np.where(u > 1, 1.0, u)
                for j in range(3):
                    acc[t, ..., j] = np.minimum(acc[t, ..., j] + u * np.float64(colors[c][j]), 1.0)
    if overlay in ("fill", "outline") and labels is not None and table is not None and len(table):
        for t in range(n_t):
            lab = labels[t]
            on = lab > 0
            a = np.float64(alpha)
            if overlay == "outline":
                pad = np.pad(lab, 1)
                edge = ((pad[:-2, 1:-1] != lab) | (pad[2:, 1:-1] != lab) | (pad[1:-1, :-2] != lab) | (pad[1:-1, 2:] != lab))
                on, a = on & edge, np.float64(1.0)
            rgb = table[np.maximum(lab, 1) - 1, t].astype(np.float64)  # (hk, wk, 3)
            mixed = (1.0 - a) * acc[t] + (a * rgb) / 255.0
            acc[t] = np.where(on[..., None], mixed, acc[t])
    return np.floor(255.0 * acc + 0.5).astype(np.uint8)


def decode_png(data):
    """(h, w, 3) uint8 of an 8-bit RGB PNG whose rows all use filter 0, with zlib and struct only."""
    import struct
    import zlib

    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype = head[:4]
    assert (depth, ctype) == (8, 2)
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3).copy()
