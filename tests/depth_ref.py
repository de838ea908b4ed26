"""NumPy restatement of the depth-stack folds (``mg_depth_project`` / ``mg_depth_focus_totals`` / ``mg_depth_fuse``,
``magnify_amd.depth``): int64 for integer pixels, float64 for float pixels, every loop written out in the order the
contract states (include/magnify_hip.h, "Depth stacks"), one NumPy operation per rounding.  Written from the contract,
not from the kernels.  A stack is (Z, H, W); the ``*_block`` helpers map over leading dimensions."""
from __future__ import annotations

import math

import numpy as np


def is_int(a) -> bool:
    return np.asarray(a).dtype.kind in "iu"


# ---- project ---------------------------------------------------------------------------------------------------------

def project_max(stack):
    """m = slice 0; for z = 1, 2, ...: m = s where s > m.  A NaN stays / enters; of equal values the first stays."""
    stack = np.asarray(stack)
    m = stack[0].copy()
    for z in range(1, stack.shape[0]):
        s = stack[z]
        if is_int(stack):
            m = np.where(s > m, s, m)
        else:
            with np.errstate(invalid="ignore"):
                m = np.where(np.isnan(m), m, np.where(np.isnan(s), s, np.where(s > m, s, m)))
    return m.astype(stack.dtype)


def project_mean(stack):
    stack = np.asarray(stack)
    nz = stack.shape[0]
    if is_int(stack):
        total = np.zeros(stack.shape[1:], dtype=np.int64)
        for z in range(nz):
            total = total + stack[z].astype(np.int64)
        return np.rint(total.astype(np.float64) / np.float64(nz)).astype(stack.dtype)  # exact below 2^53; half to even
    acc = np.zeros(stack.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(nz):
            acc = acc + stack[z].astype(np.float64)
        return (acc / np.float64(nz)).astype(stack.dtype)


def project_pick(stack, index):
    return np.asarray(stack)[int(index)].copy()


# ---- the modified Laplacian ------------------------------------------------------------------------------------------

def modified_laplacian(plane):
    """ML = |2c - l - r| + |2c - u - d|, neighbours outside the plane clamped to the edge pixel.  int64 / float64."""
    plane = np.asarray(plane)
    p = np.pad(plane.astype(np.int64 if is_int(plane) else np.float64), 1, mode="edge")
    c, l, r, u, d = p[1:-1, 1:-1], p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    with np.errstate(invalid="ignore", over="ignore"):
        c2 = 2 * c
        return np.abs((c2 - l) - r) + np.abs((c2 - u) - d)


def focus_totals(stack):
    """Per slice the sum of ML: exact Python integers for integer pixels, math.fsum (the correctly rounded sum) for
    float pixels -- the yardstick of a float64 sum taken in no defined order."""
    stack = np.asarray(stack)
    if is_int(stack):
        return np.array([int(modified_laplacian(s).sum(dtype=np.int64)) for s in stack], dtype=np.int64)
    out = []
    for s in stack:
        ml = modified_laplacian(s).ravel()
        out.append(math.fsum(ml.tolist()) if np.isfinite(ml).all() else float(np.sum(ml)))
    return np.array(out, dtype=np.float64)


def first_argmax(totals):
    """best = -inf, chosen = 0; for z = 0, 1, ...: total > best makes z the choice."""
    best, chosen = -math.inf, 0
    for z, t in enumerate(np.asarray(totals).tolist()):
        if t > best:
            best, chosen = t, z
    return chosen


# ---- fuse ------------------------------------------------------------------------------------------------------------

def window_measure(plane, k):
    """The sum of ML over the (2k + 1)^2 window of every pixel, window positions outside the plane left out: per window
    row a sum from 0 that adds the row's values left to right, then a sum from 0 that adds the row sums top to bottom."""
    ml = modified_laplacian(plane)
    h, w = ml.shape
    rows = np.zeros_like(ml)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(-k, k + 1):  # column x + j of every row, where it exists
            x0, x1 = max(0, -j), min(w, w - j)
            if x0 < x1:
                rows[:, x0:x1] = rows[:, x0:x1] + ml[:, x0 + j:x1 + j]
        out = np.zeros_like(ml)
        for i in range(-k, k + 1):  # row y + i, where it exists
            y0, y1 = max(0, -i), min(h, h - i)
            if y0 < y1:
                out[y0:y1] = out[y0:y1] + rows[y0 + i:y1 + i]
    return out


def fuse(stack, k):
    """-> (image, index uint8): per pixel the first slice with the strictly largest measure (a NaN measure never wins)."""
    stack = np.asarray(stack)
    shape = stack.shape[1:]
    best = np.full(shape, -1, dtype=np.int64) if is_int(stack) else np.full(shape, -np.inf)
    index = np.zeros(shape, dtype=np.uint8)
    image = stack[0].copy()
    for z in range(stack.shape[0]):
        m = window_measure(stack[z], k)
        with np.errstate(invalid="ignore"):
            better = m > best
        best = np.where(better, m, best)
        index[better] = z
        image[better] = stack[z][better]
    return image, index


# ---- leading dimensions and comparison ------------------------------------------------------------------------------

def over_stacks(fn, block, *args):
    """fn over every (Z, H, W) stack of a block (N, Z, H, W) -> list of results."""
    return [fn(s, *args) for s in np.asarray(block)]


def same(a, b) -> bool:
    """Bit-exact equality of pixel arrays: NaN equals NaN, -0.0 does not equal 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return bool(np.array_equal(a[~nan], b[~nan]) and np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan])))


def random_stack(rng, dtype, shape):
    """A block of ``dtype`` covering its range (integers) or 0..65535 with fractions (floats)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    return (rng.random(shape) * 65535).astype(dtype)
