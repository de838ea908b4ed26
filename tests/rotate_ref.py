"""NumPy restatement of the bilinear rotation (``mg_affine_bilinear`` / ``hotpath.rotate_image``): the arithmetic of
``scipy.ndimage.rotate(plane, angle, axes=(-1, -2), reshape=False, order=1, mode="constant", cval=0)`` in float64,
one NumPy operation per rounding, in the order the kernel uses (no fused multiply-add anywhere).

u8 / u16 / f32 results equal scipy's in every pixel; f64 differs from scipy in the last bits (scipy sums the
coordinate in another order; tests/test_cpu_rotate.py measures it)."""
from __future__ import annotations

import numpy as np
from scipy import special


def rotation_matrix_offset(angle_degrees: float, h: int, w: int):
    """(matrix (2, 2), offset (2,)) of scipy.ndimage.rotate with reshape=False on an (h, w) plane: output pixel o
    samples the input at ``matrix @ o + offset``."""
    c, s = special.cosdg(angle_degrees), special.sindg(angle_degrees)
    m = np.array([[c, s], [-s, c]], dtype=np.float64)
    ctr = np.array([(h - 1) / 2, (w - 1) / 2], dtype=np.float64)
    return m, ctr - m @ ctr


def affine_bilinear(plane: np.ndarray, matrix, offset) -> np.ndarray:
    """One (h, w) plane through the 2 x 2 affine resampler; output of the plane's dtype and size."""
    plane = np.asarray(plane)
    h, w = plane.shape
    out = np.zeros((h, w), dtype=plane.dtype)
    if h == 0 or w == 0:
        return out
    m = np.asarray(matrix, dtype=np.float64).reshape(4)
    off = np.asarray(offset, dtype=np.float64).reshape(2)
    oy = np.arange(h, dtype=np.float64)[:, None]
    ox = np.arange(w, dtype=np.float64)[None, :]
    cy = (off[0] + oy * m[0]) + ox * m[1]
    cx = (off[1] + oy * m[2]) + ox * m[3]
    inside = ~((cy < 0) | (cy > h - 1) | (cx < 0) | (cx > w - 1))
    cy = np.where(inside, cy, 0.0)
    cx = np.where(inside, cx, 0.0)
    fy, fx = np.floor(cy), np.floor(cx)
    ty, tx = cy - fy, cx - fx
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    src = plane.astype(np.float64)
    uy, ux = 1.0 - ty, 1.0 - tx
    v = (src[y0, x0] * uy) * ux
    v = v + (src[y0, x1] * uy) * tx
    v = v + (src[y1, x0] * ty) * ux
    v = v + (src[y1, x1] * ty) * tx
    v = np.where(inside, v, 0.0)
    if plane.dtype.kind == "u":
        return np.floor(v + 0.5).astype(plane.dtype)
    return v.astype(plane.dtype)


def rotate(image: np.ndarray, angle_degrees: float) -> np.ndarray:
    """Every (..., h, w) plane of ``image`` rotated by ``angle_degrees`` about its centre."""
    image = np.asarray(image)
    h, w = image.shape[-2:]
    m, off = rotation_matrix_offset(angle_degrees, h, w)
    planes = image.reshape((-1, h, w))
    out = np.stack([affine_bilinear(p, m, off) for p in planes]) if len(planes) else planes.copy()
    return out.reshape(image.shape)


def random_image(rng, dtype, shape) -> np.ndarray:
    """Test image of ``dtype`` covering its range (integers) or 0..65535 (floats)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    return (rng.random(shape) * 65535).astype(dtype)
