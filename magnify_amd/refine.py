"""Sub-pixel circle fit of every marker: ``refine_markers`` (``refine="edge"``; not in the reference, whose finders return
the integer circle of the RANSAC vote and drop its radius; DESIGN.md, "refine_markers: the circle below the pixel").

Per (marker, timepoint) the window of ONE channel is sampled along rays about the finder's circle, the steepest radial
change on every ray is located below the sample spacing, and a circle is fitted to those edge points algebraically, with
one round of rejection.  All of it is one kernel (``hotpath.refine_circles``: mg_roi_refine_circles);
``tests/refine_ref.py`` restates the contract in plain NumPy.  The fitted radius is the radius of steepest radial change:
on a blurred disk it reads about a tenth of a pixel under the geometric edge.
"""
from __future__ import annotations

import numpy as np

from . import _native as nat
from . import registry
from .utils import int_in, number

MAX_RAYS, MAX_REACH, MAX_LEN = (nat.DEFINES[k] for k in ("MG_REFINE_MAX_RAYS", "MG_REFINE_MAX_REACH", "MG_REFINE_MAX_LEN"))
MIN_RAYS = 8
SUBPIXEL = nat.DEFINES["MG_PROFILE_SUBPIXEL"]
POLARITIES = {"auto": 0, "brighter": 1, "darker": -1}
FLOAT_VARS = ("x_fit", "y_fit", "radius_fit", "fit_rms", "fit_strength")
INT_VARS = ("fit_rays", "fit_status", "fit_polarity", "radius")
REFINE_VARS = FLOAT_VARS + INT_VARS


def check_refine(rays=64, reach=3, polarity="auto", reject=1.0, min_strength=0.25, min_rays=None, roi_length=None):
    """The settings of ``refine_markers`` as the pipelines take them: ``8 <= rays <= 128`` and ``1 <= reach <= 8``
    (pixels), integers; ``polarity`` "auto", "brighter" (outside the circle) or "darker", or 0, +1, -1; ``reject`` a
    finite number of pixels > 0; ``0 <= min_strength <= 1``; ``min_rays`` None (``rays // 2``) or an integer in
    [3, rays]; with ``roi_length`` also ``1 <= roi_length <= 1024``.  ValueError otherwise.  Returns (rays, reach,
    polarity as -1 / 0 / +1, reject, min_strength, min_rays)."""
    rays = int_in("refine rays", rays, MIN_RAYS, MAX_RAYS)
    reach = int_in("refine reach", reach, 1, MAX_REACH)
    if isinstance(polarity, str):
        if polarity not in POLARITIES:
            raise ValueError(f'refine polarity must be "auto", "brighter" or "darker" (or 0, +1, -1), got {polarity!r}')
        polarity = POLARITIES[polarity]
    else:
        polarity = int_in("refine polarity", polarity, -1, 1)
    reject = number("refine reject", reject)
    if not reject > 0:
        raise ValueError(f"refine reject must be a number of pixels > 0, got {reject}")
    min_strength = number("refine min_strength", min_strength)
    if not 0.0 <= min_strength <= 1.0:
        raise ValueError(f"refine min_strength must be in [0, 1], got {min_strength}")
    min_rays = rays // 2 if min_rays is None else int_in("refine min_rays", min_rays, 3, rays)
    if roi_length is not None:
        int_in("roi_length", roi_length, 1, None)
        if roi_length > MAX_LEN:
            raise ValueError(f"refine_markers takes windows up to {MAX_LEN} pixels, got roi_length {roi_length}")
    return rays, reach, polarity, reject, min_strength, min_rays


def check_method(refine):
    """``refine=`` of the pipelines: None or "edge".  ValueError otherwise."""
    if refine is not None and not (isinstance(refine, str) and refine == "edge"):
        raise ValueError(f'refine must be None or "edge", got {refine!r}')
    return refine


def finder_radius(xp, radius=None):
    """(mark, time) int64: the integer radius of every marker's found circle -- ``radius`` where given (a number, or an
    array on (mark,) or (mark, time)), else what the finder left behind: ``(mark,)`` for beads, ``(row, col, time)`` on
    a chip.  ValueError where neither is there."""
    m, n_t = xp.data_vars["roi"].sizes["mark"], xp.data_vars["roi"].sizes["time"]
    if radius is None:
        if "radius" in xp.coords:
            radius = xp.coords["radius"].transpose(*[d for d in ("mark", "time") if d in xp.coords["radius"].dims]).values
        else:
            radius = xp._cache.get("radius")
        if radius is None:
            raise ValueError("refine: this dataset does not carry the finder's radii (a loaded dataset?): pass radius= "
                             "(pixels: one number, or an array on (mark,) or (mark, time))")
    r = np.asarray(radius)
    if r.dtype.kind not in "iuf" or (r.dtype.kind == "f" and not (np.isfinite(r).all() and (r == np.rint(r)).all())):
        raise ValueError(f"refine: radius must be whole pixels, got {radius!r}")
    r = r.astype(np.int64)
    if r.ndim == 3 and r.size == m * n_t:  # a chip's (row, col, time)
        r = r.reshape(m, n_t)
    if r.ndim == 0:
        r = np.full((m, n_t), int(r), dtype=np.int64)
    elif r.ndim == 1 and r.shape[0] == m:
        r = np.repeat(r[:, None], n_t, axis=1)
    if r.shape != (m, n_t):
        raise ValueError(f"refine: radius must be a number or an array on (mark,) or (mark, time) = {(m, n_t)}, got "
                         f"shape {np.shape(radius)}")
    if (r < 0).any():
        raise ValueError("refine: a radius is negative")
    return np.ascontiguousarray(r)


@registry.component("refine_markers")
def refine_markers(assay, channel=None, rays=64, reach=3, polarity="auto", reject=1.0, min_strength=0.25, min_rays=None,
                   radius=None):
    """Adds the sub-pixel circle of every (marker, timepoint) as coordinates on (mark, time) -- ``x_fit``, ``y_fit``
    (image coordinates, as ``x`` / ``y``), ``radius_fit``, ``fit_rms`` (the root mean squared distance of the edge
    points from the circle) and ``fit_strength`` (their mean edge strength), float64 and NaN where ``fit_status`` != 0;
    ``fit_rays`` (edge points used), ``fit_status`` (0 ok, 1 too few rays, 2 degenerate, 3 out of reach) and
    ``fit_polarity`` (+1 brighter outside, -1 darker outside), int32; ``radius``, the finder's own, int32
    (``reduce.refine_circles`` with the markers' circles).  The start circle is each timepoint's ``x``, ``y`` and the
    finder's radius in the windows of ``channel`` (None: the first).  ``x``, ``y``, ``roi``, ``fg``, ``bg`` and ``valid``
    are untouched.  With no markers the coordinates are empty and nothing is launched."""
    from . import reduce

    out = reduce.refine_circles(assay, channel=channel, rays=rays, reach=reach, polarity=polarity, reject=reject,
                                min_strength=min_strength, min_rays=min_rays, radius=radius)
    return assay.assign_coords(out)
