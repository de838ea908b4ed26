"""Sub-pixel test pictures for the circle fit: ``synth.py`` paints disks at whole-pixel centres only.

``paint`` gives an 8x supersampled disk at a real-valued centre and radius -- pixel (i, j) has its centre at (i, j), as
the bilinear sampling of mg_roi_refine_circles has it -- in one of three kinds, blurred (Gaussian, sigma 0.8), scaled to
a contrast of 3000 over an offset of 500, with additive N(0, 40) noise, rounded to uint16."""
from __future__ import annotations

import numpy as np

KINDS = ("bright", "dark", "rim")  # a bright disk; a dark disk on a bright field; a bead with a dark rim inside
POLARITY = {"bright": -1, "dark": 1, "rim": -1}  # +1: brighter outside
SUPER, SIGMA, CONTRAST, OFFSET, NOISE = 8, 0.8, 3000.0, 500.0, 40.0


def disk(L, cy, cx, r):
    """Coverage in [0, 1] of every pixel of an L x L window by the disk of radius r about (cy, cx): the mean of SUPER x
    SUPER point samples."""
    if r <= 0:
        return np.zeros((L, L))
    pos = (np.arange(L * SUPER, dtype=np.float64) + 0.5) / SUPER - 0.5
    inside = (pos[:, None] - cy) ** 2 + (pos[None, :] - cx) ** 2 <= r * r
    return inside.reshape(L, SUPER, L, SUPER).mean(axis=(1, 3))


def blur(img, sigma=SIGMA):
    """Separable Gaussian, truncated at 4 sigma, the border pixel repeated."""
    half = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-half, half + 1) / sigma) ** 2)
    k /= k.sum()
    out = np.pad(img, half, mode="edge")
    out = sum(k[i] * out[i:i + img.shape[0]] for i in range(2 * half + 1))
    return sum(k[i] * out[:, i:i + img.shape[1]] for i in range(2 * half + 1))


def shape(kind, L, cy, cx, r):
    """The noiseless picture in [0, 1]."""
    if kind == "bright":
        return disk(L, cy, cx, r)
    if kind == "dark":
        return 1.0 - disk(L, cy, cx, r)
    if kind == "rim":
        return disk(L, cy, cx, r) - 0.8 * disk(L, cy, cx, r - 2.5)
    raise ValueError(kind)


def paint(kind, L, cy, cx, r, rng, noise=NOISE):
    img = OFFSET + CONTRAST * blur(shape(kind, L, cy, cx, r))
    if noise:
        img = img + rng.normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


def accuracy_cases(n=600, L=48, seed=20240607):
    """The cases of the accuracy test: true centre L / 2 +- U(-1, 1) on each axis, radius U(5, 16), the kinds in
    rotation; the start circle is the rounded truth moved by -1, 0 or +1 in each of cy, cx and r.  -> list of (kind,
    window uint16, truth (cy, cx, r), start int32 {cy, cx, r} in 1/16 pixel)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        cy, cx = L / 2 + rng.uniform(-1, 1, 2)
        r = rng.uniform(5, 16)
        start = np.rint([cy, cx, r]) + rng.integers(-1, 2, 3)
        out.append((kind, paint(kind, L, cy, cx, r, rng), (cy, cx, r), (start * 16).astype(np.int32)))
    return out
