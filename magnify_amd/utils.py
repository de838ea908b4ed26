"""Host-side helpers with the reference's names (src/magnify/utils.py:55-99, 398-465).  The digital
circle tables come from the native library (no GPU needed)."""
from __future__ import annotations

import inspect
import math
import numbers
import os
import re
from collections.abc import Iterable

import numpy as np

from . import _native

PathLike = (str, bytes, os.PathLike)
_SEED = {"value": None, "counter": 0}


def seed(value):
    """Fix the RNG stream of the circle finders (the reference draws from an unseeded numba RNG,
    utils.py:309-320; by default this build draws a fresh seed from OS entropy per call)."""
    _SEED["value"] = None if value is None else int(value)
    _SEED["counter"] = 0


def next_seed() -> int:
    if _SEED["value"] is None:
        return int(np.random.SeedSequence().generate_state(2, dtype=np.uint32).view(np.uint64)[0])
    _SEED["counter"] += 1
    return (_SEED["value"] + 0x632BE59BD9B4E019 * _SEED["counter"]) & 0xFFFFFFFFFFFFFFFF


def ceildiv(a: int, b: int) -> int:
    return -(a // -b)


def bounding_box(x: int, y: int, box_length: int, image_width: int, image_height: int):
    """(top, bottom, left, right) of the L x L window clamped into the image (utils.py:60-80)."""
    def clamp(c, size):
        lo, hi = c - box_length // 2, c + ceildiv(box_length, 2)
        if lo < 0:
            lo, hi = 0, hi - lo
        if hi > size:
            lo, hi = lo - (hi - size), size
        return lo, hi

    top, bottom = clamp(y, image_height)
    left, right = clamp(x, image_width)
    return top, bottom, left, right


def window_origin(c, L, size):
    """``bounding_box`` for integer arrays: where the L-wide window about every centre ``c`` begins once it is shifted
    into [0, size) -- int64, the shape of ``c``.  The caller rounds: the finders half to even, ``plot`` by truncation."""
    lo = np.maximum(np.asarray(c).astype(np.int64) - L // 2, 0)
    return np.where(lo + L > size, size - L, lo)


def roi_mark_chunk(bound: int, n_channels: int, n_times: int, roi_length: int, chunk_bytes: float = 1e6) -> int:
    """Markers per chunk of ``roi / fg / bg`` as the reference chunks them (find.py:185-188, 506-531): every channel
    and timepoint of a marker in one chunk, as many markers as make at least ``chunk_bytes`` -- counted in pixels, "since
    fg/bg bool arrays should also be 1MB" --, at most ``bound`` (the bead count; for chips the reference bounds by the
    number of marker ROWS, find.py:187)."""
    per_marker = roi_length ** 2 * n_channels * n_times
    return int(max(0, min(math.ceil(chunk_bytes / max(per_marker, 1)), bound)))


def circle_points(r, four_connected=False):
    return _native.circle_points(int(r), four_connected)


def filled_circle_points(r):
    r = int(r)
    hw = _native.disk_halfwidths(r)
    per = _native.circle_points(r)
    seen = {tuple(p) for p in per.tolist()}
    inner = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-hw[dy + r], hw[dy + r] + 1) if (dy, dx) not in seen]
    return np.concatenate([per, np.asarray(inner, dtype=np.int32).reshape(-1, 2)])


def valid_kwargs(kwargs, func):
    args = list(inspect.signature(func).parameters)
    return {k: kwargs[k] for k in kwargs if k in args}


def natural_sort_key(s: str):
    return [int(t) if t.isdigit() else t.lower() for t in re.split("([0-9]+)", s)]


def int_in(name, value, lo, hi=None):
    """``value`` as an int where it is an integer -- ``int`` or ``np.integer``; no bool, no float, not even an integral
    one -- in [lo, hi] (``hi`` None: no upper bound).  ValueError that names ``name`` and the range otherwise."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {value!r}")
    if value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} must be in [{lo}, {hi}], got {value}" if hi is not None else
                         f"{name} must be at least {lo}, got {value}")
    return int(value)


def number(name, v):
    """``v`` as a float where it is a finite real number -- no bool, no string.  ValueError that names ``name``
    otherwise."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real):
        raise ValueError(f"{name} must be a number, got {v!r}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {v!r}")
    return v


def to_list(x):
    if x is None:
        return []
    if not isinstance(x, Iterable) or isinstance(x, str):
        return [x]
    return list(x)
