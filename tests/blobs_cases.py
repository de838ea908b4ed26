"""The planes of the blob tests: structured masks that put every contact of the tile and seam passes where it can go
wrong, and the scene of the end-to-end test.  Masks are bool (h, w); the tests label ``mask.astype(uint8) > 0``."""
from __future__ import annotations

import numpy as np


def structured_shape(th, tw):
    return 3 * th + 2, 3 * tw + 2


def corners_and_tile_corner(h, w, th, tw):
    """One pixel at each image corner and at each of the four pixels round the interior tile corner (th, tw)."""
    m = np.zeros((h, w), dtype=bool)
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (th - 1, tw - 1), (th - 1, tw), (th, tw - 1), (th, tw)]:
        m[y, x] = True
    return m


def pair(h, w, a, b):
    m = np.zeros((h, w), dtype=bool)
    m[a], m[b] = True, True
    return m


def spiral(h, w):
    """A one-pixel-wide rectangular spiral of pitch 2 from (0, 0) inward -> (mask, path as a list of (y, x))."""
    m = np.zeros((h, w), dtype=bool)
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    y = x = d = 0
    m[0, 0] = True
    path = [(0, 0)]
    turns = 0
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, by, bx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= by < h and 0 <= bx < w and m[by, bx])
        if free:
            y, x, turns = ny, nx, 0
            m[y, x] = True
            path.append((y, x))
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m, path


def comb(h, w):
    """Teeth on every second column through all rows, joined by a bar on the last row: the root is found last."""
    m = np.zeros((h, w), dtype=bool)
    m[:, ::2] = True
    m[h - 1, :] = True
    return m


def nested_us(h, w):
    """U shapes opening upward, one inside the other with one pixel between them -> (mask, how many)."""
    m = np.zeros((h, w), dtype=bool)
    k = 0
    while 2 * k < w - 1 - 2 * k - 1 and h - 1 - 2 * k > 0:
        left, right, bottom = 2 * k, w - 1 - 2 * k, h - 1 - 2 * k
        m[: bottom + 1, left] = True
        m[: bottom + 1, right] = True
        m[bottom, left: right + 1] = True
        k += 1
    return m, k


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return (yy + xx) % 2 == 0


def ellipse(shape, cy, cx, a, b, angle):
    yy, xx = np.mgrid[: shape[0], : shape[1]]
    dy, dx = yy - cy, xx - cx
    u = dx * np.cos(angle) + dy * np.sin(angle)
    v = -dx * np.sin(angle) + dy * np.cos(angle)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def mark_of(labels, mask):
    """The number most of ``mask``'s labelled pixels carry."""
    v = labels[mask & (labels >= 0)]
    return int(np.bincount(v).argmax())


SCENE_SHAPE = (300, 400)
SCENE_BLOBS = 12
SCENE_RING = 5  # the sixth blob is a ring


def scene(seed=0, dtype=np.uint16):
    """300 x 400: background 100 + Poisson(20); a 3 x 4 grid of ellipses on a 90-pixel pitch from (50, 60), each
    jittered by up to 6 pixels, semi-axes 10 .. 16 by 8 .. 12 at a random angle, 1500 brighter; the sixth a ring 4 pixels
    thick; noise N(0, 30); rounded and clipped.  -> (plane, filled ellipse masks (12, h, w), the ring's own mask)."""
    rng = np.random.default_rng(seed)
    h, w = SCENE_SHAPE
    img = 100.0 + rng.poisson(20, size=(h, w))
    masks, ring = [], None
    for i in range(3):
        for j in range(4):
            cy, cx = 50 + 90 * i + rng.uniform(-6, 6), 60 + 90 * j + rng.uniform(-6, 6)
            a, b, angle = rng.uniform(10, 16), rng.uniform(8, 12), rng.uniform(0, np.pi)
            full = ellipse((h, w), cy, cx, a, b, angle)
            body = full
            if len(masks) == SCENE_RING:
                body = ring = full & ~ellipse((h, w), cy, cx, a - 4, b - 4, angle)
            img[body] += 1500.0
            masks.append(full)
    img += rng.normal(0.0, 30.0, size=(h, w))
    if np.dtype(dtype).kind == "u":
        img = np.clip(np.rint(img), 0, np.iinfo(dtype).max)
    return img.astype(dtype), np.stack(masks), ring
