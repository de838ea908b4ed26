"""Radial intensity profiles of the ROI windows: ``profile_rois`` (not in the reference, whose reductions stop at one
number per mask; DESIGN.md, "profile_rois: rings about the marker").

Per (marker, channel, timepoint) the window is cut into rings about the marker's centre -- ring ``k`` holds the pixels at
distance ``edges[k] <= d < edges[k + 1]`` -- and every ring is reduced to a count, a sum and a sum of squares by one
kernel (``hotpath.radial_profile``: mg_roi_radial_profile).  Centres and edges are quantised to 1/16 pixel on the host
and everything after that is integer arithmetic; ``tests/radial_ref.py`` restates the contract in plain Python.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native as nat
from . import registry
from .utils import int_in, number

MAX_RINGS, SUBPIXEL, MAX_LEN = (nat.DEFINES[k] for k in ("MG_PROFILE_MAX_RINGS", "MG_PROFILE_SUBPIXEL", "MG_PROFILE_MAX_LEN"))
MAX_EDGE, CENTRE_MIN, CENTRE_MAX = (nat.DEFINES[k] for k in ("MG_PROFILE_MAX_EDGE", "MG_PROFILE_CENTRE_MIN", "MG_PROFILE_CENTRE_MAX"))
PROFILE_VARS = ("profile_count", "profile_sum", "profile_sumsq")


def quantise(v):
    """``np.rint(v * 16)`` in float64: a length in pixels as the kernel's integer of 1/16 pixel (still float64)."""
    return np.rint(np.asarray(v, dtype=np.float64) * float(SUBPIXEL))


INT_LIMIT = 2.0**30  # what a caller's float is clipped to before it becomes an int32


def quantised(v):
    """``quantise(v)`` as the int32 the kernels take; they clamp to their own, narrower range."""
    return np.clip(quantise(v), -INT_LIMIT, INT_LIMIT).astype(np.int32)


def check_edges_q(edges_q):
    """Quantised edges as the kernel takes them: int32 (n_rings + 1,), 1 <= n_rings <= 128, 0 <= edges[0] < edges[1] <
    ... <= 46340.  ValueError otherwise."""
    e = np.asarray(edges_q)
    if e.ndim != 1 or e.dtype.kind not in "iu":
        raise ValueError(f"profile edges must be a 1-d integer array in 1/{SUBPIXEL} pixel, got {e.dtype} {e.shape}")
    if not 2 <= len(e) <= MAX_RINGS + 1:
        raise ValueError(f"profile needs 1 to {MAX_RINGS} rings, got {len(e) - 1}")
    e = e.astype(np.int64)
    if e[0] < 0 or e[-1] > MAX_EDGE:
        raise ValueError(f"profile edges must lie in [0, {MAX_EDGE / SUBPIXEL}] pixels, got {e[0] / SUBPIXEL} .. "
                         f"{e[-1] / SUBPIXEL}")
    if (np.diff(e) <= 0).any():
        raise ValueError(f"profile edges must increase by at least 1/{SUBPIXEL} pixel from one to the next")
    return np.ascontiguousarray(e, dtype=np.int32)


def ring_edges(width=1.0, rings=None, edges=None, roi_length=None):
    """The quantised ring edges (int32, in 1/16 pixel) of ``edges`` -- radii in pixels -- or of ``0, width, 2 width, ...``
    for ``rings`` rings, by default ``ceil(roi_length / (2 width))`` of them.  Quantised as ``np.rint(v * 16)`` in float64.
    ValueError for what ``check_profile`` refuses."""
    if edges is not None:
        e = np.asarray(edges)
        if e.ndim != 1 or e.dtype.kind not in "iuf" or e.dtype == np.bool_:
            raise ValueError(f"profile edges must be a 1-d sequence of numbers, got {edges!r}")
        e = e.astype(np.float64)
        if not np.isfinite(e).all():
            raise ValueError("profile edges must be finite")
        if not 2 <= len(e) <= MAX_RINGS + 1:
            raise ValueError(f"profile needs 1 to {MAX_RINGS} rings, got {len(e) - 1}")
        q = quantise(e)
    else:
        width = number("profile width", width)
        if quantise(width) < 1:
            raise ValueError(f"profile width must be at least 1/{SUBPIXEL} pixel, got {width}")
        if rings is None:
            if roi_length is None:
                raise ValueError("profile rings must be given where the window length is not known")
            rings = int(math.ceil(roi_length / (2.0 * width)))
        rings = int_in("profile rings", rings, 1, MAX_RINGS)
        q = quantise(np.arange(rings + 1, dtype=np.float64) * width)
    if q[0] < 0 or q[-1] > MAX_EDGE:
        raise ValueError(f"profile edges must lie in [0, {MAX_EDGE / SUBPIXEL}] pixels, got {q[0] / SUBPIXEL} .. "
                         f"{q[-1] / SUBPIXEL}")
    return check_edges_q(q.astype(np.int64))


def check_profile(width=1.0, rings=None, mask="own", roi_length=None, edges=None):
    """The settings of ``profile_rois`` as the pipelines take them.  ``width``: a finite number of pixels that is at
    least 1/16 after quantisation; ``rings``: None or an integer in [1, 128] (None needs ``roi_length``, and
    ``ceil(roi_length / (2 width))`` must not exceed 128); ``edges`` (instead of both): 2 to 129 finite, strictly
    increasing radii in [0, 2896.25] pixels that stay distinct at 1/16 pixel; ``mask``: "own", None, or a coordinate
    name; ``roi_length``: None or an integer in [1, 1024].  ValueError otherwise.  Returns the quantised edges, or None
    where they depend on a window length that is not known yet."""
    if mask is not None and not isinstance(mask, str):
        raise ValueError(f'profile mask must be "own", None or the name of a coordinate, got {mask!r}')
    if roi_length is not None:
        int_in("roi_length", roi_length, 1, None)
        if roi_length > MAX_LEN:
            raise ValueError(f"profile_rois takes windows up to {MAX_LEN} pixels, got roi_length {roi_length}")
    if edges is None and rings is None and roi_length is None:
        width = number("profile width", width)
        if quantise(width) < 1:
            raise ValueError(f"profile width must be at least 1/{SUBPIXEL} pixel, got {width}")
        return None
    return ring_edges(width, rings, edges, roi_length)


def ring_coords(edges_q):
    """{ring, ring_inner, ring_outer}: mid, inner and outer radius of every ring in pixels, from the quantised edges."""
    e = np.asarray(edges_q, dtype=np.float64) / float(SUBPIXEL)
    return {"ring": (e[:-1] + e[1:]) / 2.0, "ring_inner": e[:-1].copy(), "ring_outer": e[1:].copy()}


@registry.component("profile_rois")
def profile_rois(assay, width=1.0, rings=None, mask="own"):
    """Adds ``profile_count`` int32 (mark, channel, time, ring) and ``profile_sum`` / ``profile_sumsq`` float64 on the same
    dimensions -- the radial profile of every window about its marker (``reduce.radial_profile`` with
    ``centre="marker"``) -- with the coordinates ``ring`` (mid radius in pixels), ``ring_inner`` and ``ring_outer``.
    ``mask="own"``: a bead's own fg | bg, so that a neighbour's disk never enters its profile; every pixel on a chip.
    With no markers the variables are empty and nothing is launched."""
    from . import reduce
    from .xr_lite import DataArray

    roi_var = assay.data_vars["roi"]
    L = roi_var.sizes["roi_y"]
    edges_q = check_profile(width, rings, mask, L)
    count, moments = reduce.radial_profile(assay, edges=edges_q / float(SUBPIXEL), mask=mask, centre="marker")
    dims = ("mark", "channel", "time", "ring")
    out = assay.assign_coords({k: (("ring",), v) for k, v in ring_coords(edges_q).items()})
    out["profile_count"] = DataArray(count.data, dims)
    out["profile_sum"] = DataArray(moments.data[..., 0], dims)
    out["profile_sumsq"] = DataArray(moments.data[..., 1], dims)
    return out
