"""Data-driven fg / bg masks: ``segment_rois`` (not in the reference, whose masks are drawn shapes -- the fitted circle of
a bead, find.py:561-586, the disk and annulus of a chip marker, find.py:383-400; DESIGN.md, "segment_rois: masks from
the pixels").

Per (marker, timepoint) the window of ONE channel decides: a threshold (Otsu on the window's 256 ``to_uint8`` bins, or a
number), a 3x3 opening, the drawn foreground's part of the opened mask grown inside it by at most ``max_grow`` pixels,
and the drawn background without a guard band around everything bright.  A window where nothing is left (a blank
chamber, a flat window) keeps its drawn masks.  All of it is one kernel (``hotpath.threshold_masks``:
mg_roi_threshold_masks); ``tests/segment_ref.py`` restates the contract in NumPy + scipy.ndimage.
"""
from __future__ import annotations

import numpy as np

from . import _dataset
from . import _native as nat
from . import registry
from .utils import int_in

MAX_LEN = nat.DEFINES["MG_SEGMENT_MAX_LEN"]
MAX_OPEN, MAX_GROW, MAX_GUARD = (nat.DEFINES[k] for k in ("MG_SEGMENT_MAX_OPEN", "MG_SEGMENT_MAX_GROW",
                                                           "MG_SEGMENT_MAX_GUARD"))


def check_segment(method="otsu", open_radius=1, max_grow=4, bg_guard=2, min_area=1, roi_length=None):
    """The settings of ``segment_rois`` as the pipelines take them: ``method`` "otsu" or a (non-NaN) number;
    ``0 <= open_radius <= 8``, ``0 <= max_grow <= 32``, ``0 <= bg_guard <= 16``, ``min_area >= 0``, all integers; with
    ``roi_length`` also ``1 <= roi_length <= 128``.  ValueError otherwise.  Returns (use_otsu, threshold)."""
    if isinstance(method, str):
        if method != "otsu":
            raise ValueError(f'segment method must be "otsu" or a number, got {method!r}')
        use_otsu, threshold = True, 0.0
    else:
        if isinstance(method, (bool, np.bool_)) or not isinstance(method, (int, float, np.integer, np.floating)):
            raise ValueError(f'segment method must be "otsu" or a number, got {method!r}')
        use_otsu, threshold = False, float(method)
        if threshold != threshold:
            raise ValueError("segment threshold must not be NaN")
    int_in("open_radius", open_radius, 0, MAX_OPEN)
    int_in("max_grow", max_grow, 0, MAX_GROW)
    int_in("bg_guard", bg_guard, 0, MAX_GUARD)
    int_in("min_area", min_area, 0, None)
    if roi_length is not None:
        int_in("roi_length", roi_length, 1, None)
        if roi_length > MAX_LEN:
            raise ValueError(f"segment_rois holds a window's masks in LDS: roi_length must not exceed {MAX_LEN}, "
                             f"got {roi_length}")
    return use_otsu, threshold


def channel_index(assay, channel):
    """Index of ``channel`` -- a name of the ``channel`` coordinate, or an index; None: the first channel
    (``_dataset.channel_index``; an unknown channel is a ValueError and a KeyError)."""
    return _dataset.channel_index(assay, channel, default=0)


@registry.component("segment_rois")
def segment_rois(assay, method="otsu", channel=None, open_radius=1, max_grow=4, bg_guard=2, min_area=1):
    """Replace ``fg`` / ``bg`` of every (marker, timepoint) by masks derived from the window's pixels in ``channel``
    (module docstring); adds ``segmented`` (bool) and ``seg_threshold`` (float64) on (mark, time).  Beads (no ``tag``
    coordinate): only pixels of the bead's own drawn fg or bg can become its foreground, so a neighbour's disk and
    contested pixels never do.  ``roi``, ``x``, ``y`` and ``valid`` are untouched."""
    import torch

    from . import hotpath
    from .xr_lite import DataArray

    roi_var = assay.data_vars["roi"]
    L, m, n_t = roi_var.sizes["roi_y"], roi_var.sizes["mark"], roi_var.sizes["time"]
    check_segment(method, open_radius, max_grow, bg_guard, min_area, L)
    ch = channel_index(assay, channel)
    if m == 0:
        return assay.assign_coords(segmented=(("mark", "time"), np.zeros((0, n_t), dtype=bool)),
                                   seg_threshold=(("mark", "time"), np.zeros((0, n_t), dtype=np.float64)))
    hotpath.require_gpu()
    roi = _dataset.device_tensor(roi_var, _dataset.ROI_DIMS)
    old_fg, old_bg = assay.coords["fg"], assay.coords["bg"]
    fg0, bg0 = (_dataset.device_tensor(a, _dataset.MASK_DIMS, as_mask=True) for a in (old_fg, old_bg))
    allowed = None if "tag" in assay.coords else _dataset.own_mask(fg0, bg0)
    fg, bg, threshold, counts, segmented = hotpath.threshold_masks(
        roi[:, ch], fg0, bg0, allowed, method=method, open_radius=open_radius, max_grow=max_grow, bg_guard=bg_guard,
        min_area=min_area)
    out = assay.assign_coords(
        fg=DataArray(fg.view(torch.bool), _dataset.MASK_DIMS, None, "fg", dict(old_fg.attrs)),
        bg=DataArray(bg.view(torch.bool), _dataset.MASK_DIMS, None, "bg", dict(old_bg.attrs)),
        segmented=(("mark", "time"), segmented.view(torch.bool)),
        seg_threshold=(("mark", "time"), threshold),
    )
    # the finder's fused reductions answered for the drawn masks: counts come from the kernel, sums are recomputed on demand
    out._cache["roi_counts"] = counts  # (mark, time, {fg, bg}) int32, the layout of the tracked path
    out._cache.pop("roi_sums", None)
    return out
