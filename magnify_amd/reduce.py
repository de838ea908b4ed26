"""Per-ROI reductions on the device: the expressions users and the reference's
identify/filter steps write with xarray (README.md:21-22, identify.py:76-80, filter.py:21-22),
computed by the fused HIP reductions instead of a float64 NaN-masked copy of ``roi``.

All functions take the Dataset returned by ``find_beads`` / ``find_buttons`` *before*
``restore_format`` squeezes dimensions, or any Dataset holding ``roi (mark, channel, time, roi_y,
roi_x)`` with ``fg`` / ``bg (mark, time, roi_y, roi_x)``."""
from __future__ import annotations

import numpy as np
import torch

from . import hotpath
from ._dataset import (MASK_DIMS, ROI_DIMS, channel_index, device_tensor, marker_centres, marker_windows, per_marker,
                       roi_windows, time_pick)
from .xr_lite import DataArray


def _sums_counts(xp, mask):
    """(sums (M, C, T) float64, counts (M, T) int64) of roi under a mask: one call of the masked-sum kernel
    (mg_masked_sums), which reads the mask of every timepoint where it lies."""
    roi = device_tensor(xp.data_vars["roi"], ROI_DIMS)
    sums, cnt = hotpath.masked_sums(roi, device_tensor(xp.coords[mask], MASK_DIMS, as_mask=True))
    return sums[..., 0], cnt[..., 0].to(torch.int64).expand(roi.shape[0], roi.shape[2])


def counts(xp, mask="fg"):
    """xp.fg.sum(dim=["roi_x", "roi_y"])  (README.md:21) -> (mark, time) int64."""
    cached = xp._cache.get("roi_counts")
    n_t = xp.sizes.get("time", 1)
    if cached is not None and mask in ("fg", "bg") and "mark" in xp.sizes and cached.shape[0] == xp.sizes["mark"]:
        if cached.dim() == 3:  # (mark, time, 2): beads followed through time have masks of their own per timepoint
            return DataArray(cached[..., 0 if mask == "fg" else 1].to(torch.int64), ("mark", "time"))
        return DataArray(cached[:, 0 if mask == "fg" else 1].to(torch.int64)[:, None].expand(-1, n_t), ("mark", "time"))
    return DataArray(_sums_counts(xp, mask)[1], ("mark", "time"))


def masked_sum(xp, mask="fg"):
    """roi.where(mask).sum(dim=[roi_y, roi_x]) -> (mark, channel, time) float64 (exact for integers)."""
    cached = xp._cache.get("roi_sums")
    if cached is not None and mask in ("fg", "bg"):
        return DataArray(cached[..., 0 if mask == "fg" else 1], ("mark", "channel", "time"))
    return DataArray(_sums_counts(xp, mask)[0], ("mark", "channel", "time"))


def masked_mean(xp, mask="fg"):
    """roi.where(mask).mean(dim=[roi_y, roi_x]) (README.md:22): sum / count, NaN for an empty mask."""
    if xp._cache.get("roi_sums") is None and xp._cache.get("roi_counts") is None:  # no answer yet: one pass gives both
        s, n = _sums_counts(xp, mask)
    else:
        s, n = masked_sum(xp, mask).data, counts(xp, mask).data
    return DataArray(s / n.to(torch.float64)[:, None], ("mark", "channel", "time"))


def masked_median(xp, mask="bg", time=None):
    """roi.where(mask).median(dim=[roi_y, roi_x]) with numpy nanmedian semantics -> (mark, channel, time) float64.
    Any roi dtype the hot path carries (uint8, uint16, float32, float64); the masks may differ between timepoints (a
    chip searched at several timesteps, find.py:119-140).  ``time=k``: of timepoint ``k`` only, selected BEFORE the
    reduction as ``assay.isel(time=0)`` does in filter.py:20-22, 69-75 and identify.py:76 -- the other timepoints are
    neither read nor reduced; the result keeps a time axis of length 1."""
    return DataArray(hotpath.masked_median(*roi_windows(xp, mask, time)), _MCT)


def fg_mean_minus_bg_median(xp, time=None):
    """identify.py:76-80 (``time=0``: ``assay.roi.isel(time=0)`` first, as the reference does)."""
    mean = masked_mean(xp, "fg").data
    if time is not None:
        mean = mean[:, :, time:time + 1]
    return DataArray(mean - masked_median(xp, "bg", time=time).data, ("mark", "channel", "time"))


# ---- every statistic of a masked ROI from one read of each window (mg_roi_masked_stats) --------------------------------
_MCT = ("mark", "channel", "time")


def masked_stats(xp, mask="fg", q=(), time=None):
    """(count, stats, order) of roi under ``mask`` -- a coordinate name, or a DataArray on (mark[, time], roi_y, roi_x)
    -- as DataArrays on the device: count (mark, channel, time) int32, stats (mark, channel, time, stat) =
    {sum, m2, min, max} and order (mark, channel, time, quantile, bound) = the two order statistics every fraction of
    ``q`` falls between (``hotpath.masked_stats``).  A pixel takes part iff the mask is set and it is not NaN.
    ``time=k``: of timepoint ``k`` only, selected before the reduction as ``masked_median`` does."""
    count, stats, order = hotpath.masked_stats(*roi_windows(xp, mask, time), q)
    return (DataArray(count, _MCT), DataArray(stats, _MCT + ("stat",)), DataArray(order, _MCT + ("quantile", "bound")))


def interpolate_quantiles(count, order, q):
    """numpy's ``method="linear"`` between the order statistics of ``hotpath.masked_stats``, operation for operation
    in float64: pos = (n - 1) q, g = pos - floor(pos), d = b - a; b - d (1 - g) where g >= 0.5, else a + d g.
    count (...), order (..., n_q, 2), q (n_q,) -> (..., n_q); torch tensors or NumPy arrays alike."""
    xp_ = torch if isinstance(order, torch.Tensor) else np
    if xp_ is torch:
        qv = torch.as_tensor(np.asarray(q, dtype=np.float64).reshape(-1), device=order.device)
        n = count.to(torch.float64)[..., None]
    else:
        qv = np.asarray(q, dtype=np.float64).reshape(-1)
        n = np.asarray(count).astype(np.float64)[..., None]
    pos = (n - 1.0) * qv
    g = pos - xp_.floor(pos)
    a, b = order[..., 0], order[..., 1]
    d = b - a
    return xp_.where(g >= 0.5, b - d * (1.0 - g), a + d * g)


def variance_from_m2(count, m2, ddof=0):
    """m2 / (n - ddof), NaN where n - ddof <= 0 (torch tensors)."""
    dof = count.to(torch.float64) - float(ddof)
    return torch.where(dof > 0, m2 / dof, torch.full_like(m2, float("nan")))


def masked_count(xp, mask="fg", time=None):
    """roi.where(mask).count(dim=[roi_y, roi_x]) -> (mark, channel, time) int64."""
    return DataArray(masked_stats(xp, mask, (), time)[0].data.to(torch.int64), _MCT)


def masked_min(xp, mask="fg", time=None):
    """roi.where(mask).min(dim=[roi_y, roi_x]) -> (mark, channel, time) float64, NaN for an empty mask."""
    return DataArray(masked_stats(xp, mask, (), time)[1].data[..., 2], _MCT)


def masked_max(xp, mask="fg", time=None):
    """roi.where(mask).max(dim=[roi_y, roi_x]) -> (mark, channel, time) float64, NaN for an empty mask."""
    return DataArray(masked_stats(xp, mask, (), time)[1].data[..., 3], _MCT)


def masked_var(xp, mask="fg", ddof=0, time=None):
    """roi.where(mask).var(dim=[roi_y, roi_x], ddof=ddof): m2 / (n - ddof), NaN where n - ddof <= 0."""
    count, stats, _ = masked_stats(xp, mask, (), time)
    return DataArray(variance_from_m2(count.data, stats.data[..., 1], ddof), _MCT)


def masked_std(xp, mask="fg", ddof=0, time=None):
    """roi.where(mask).std(dim=[roi_y, roi_x], ddof=ddof): the square root of ``masked_var``."""
    return DataArray(torch.sqrt(masked_var(xp, mask, ddof, time).data), _MCT)


def masked_quantile(xp, q, mask="fg", time=None):
    """roi.where(mask).quantile(q, dim=[roi_y, roi_x]) -> (mark, channel, time) for a scalar ``q``, (quantile, mark,
    channel, time) for a sequence, as xarray has it; NaN for an empty mask.  The order statistics are exact and the
    interpolation between them is numpy's ``method="linear"`` operation for operation, so the result equals
    ``np.nanquantile`` bit for bit.  ``masked_quantile(xp, 0.5)`` therefore follows ``nanquantile`` while
    ``masked_median`` follows ``nanmedian`` (the mean of the two middle values): for float64 pixels the two can
    differ in the last bit."""
    count, _, order = masked_stats(xp, mask, np.atleast_1d(q), time)
    val = interpolate_quantiles(count.data, order.data, np.atleast_1d(q))
    if np.ndim(q) == 0:
        return DataArray(val[..., 0], _MCT)
    return DataArray(val.permute(3, 0, 1, 2), ("quantile",) + _MCT, {"quantile": np.asarray(q, dtype=np.float64)})


# ---- radial profiles: R numbers per window instead of one (mg_roi_radial_profile) -----------------------------------------
_MCTR = _MCT + ("ring",)


def radial_profile(xp, width=1.0, rings=None, edges=None, mask="own", centre="marker", time=None):
    """(count, moments) of roi in rings about every marker, as DataArrays on the device: count (mark, channel, time,
    ring) int32 and moments (mark, channel, time, ring, moment) float64 = {sum x, sum x^2} (``hotpath.radial_profile``),
    with the coordinates ``ring`` (mid radius in pixels), ``ring_inner`` and ``ring_outer``.
    ``edges``: radii in pixels; otherwise ``0, width, 2 width, ...`` for ``rings`` rings, by default
    ``ceil(L / (2 width))``.  Edges and centres are quantised on the host as ``np.rint(v * 16)`` in float64 and the
    coordinates report the quantised values; ring k holds the pixels with edges[k] <= d < edges[k + 1].
    ``centre``: "marker" -- x - left, y - top of each timepoint's own x, y, the window origin being the finder's;
    "window" -- L // 2 on both axes; or a DataArray / array on (mark[, time], 2) = {y, x} in window coordinates.
    ``mask``: "own" -- fg | bg for beads (a dataset without a ``tag`` coordinate), so that a neighbour's disk never
    enters a bead's profile, every pixel for chips; None -- every pixel; a coordinate name or a DataArray as in
    ``masked_stats``.  A pixel takes part iff the mask is set and it is not NaN.  ``time=k``: of timepoint ``k`` only,
    selected before the reduction."""
    from . import profile

    roi_var = xp.data_vars["roi"]
    L, m = roi_var.sizes["roi_y"], roi_var.sizes["mark"]
    if mask is not None and not isinstance(mask, (str, DataArray)):
        raise ValueError(f'radial_profile: mask must be "own", None, a coordinate name or a DataArray, got {mask!r}')
    edges_q = profile.check_profile(width, rings, mask if isinstance(mask, str) else None, L, edges)
    one = time_pick(time)
    n_t = roi_var.sizes["time"] if one is None else len(range(roi_var.sizes["time"])[one])
    # the centres, float64 (mark, 1 or time, 2) in pixels
    if isinstance(centre, str):
        if centre == "marker":
            c = marker_centres(xp, L, time)
        elif centre == "window":
            c = np.full((m, 1, 2), float(L // 2))
        else:
            raise ValueError(f'radial_profile: centre must be "marker", "window" or the centres, got {centre!r}')
    else:
        c = per_marker("radial_profile", centre, m, roi_var.sizes["time"], 2, "centre")
        if one is not None and c.shape[1] != 1:
            c = c[:, one]
    centre_q = profile.quantised(c)  # (finite: per_marker checked a caller's, find._rounded_centres the markers')
    coords = profile.ring_coords(edges_q)
    r = len(edges_q) - 1
    if m == 0:
        n_c = roi_var.sizes["channel"]
        return (DataArray(np.zeros((0, n_c, n_t, r), dtype=np.int32), _MCTR, coords),
                DataArray(np.zeros((0, n_c, n_t, r, 2), dtype=np.float64), _MCTR + ("moment",), coords))
    count, moments = hotpath.radial_profile(*roi_windows(xp, mask, time), centre_q, edges_q)
    return DataArray(count, _MCTR, coords), DataArray(moments, _MCTR + ("moment",), coords)


# ---- the circle below the pixel: edge points along rays, then a circle fit (mg_roi_refine_circles) ------------------------
def refine_circles(xp, channel=None, rays=64, reach=3, polarity="auto", reject=1.0, min_strength=0.25, min_rays=None,
                   radius=None, circle="marker"):
    """The sub-pixel circle of every (marker, timepoint) in the windows of ``channel`` (None: the first), as a dict of
    DataArrays on (mark, time) (``hotpath.refine_circles``): ``x_fit``, ``y_fit``, ``radius_fit``, ``fit_rms``,
    ``fit_strength`` float64, NaN where ``fit_status`` != 0; ``fit_rays``, ``fit_status``, ``fit_polarity`` and ``radius``
    int32 (``refine.refine_markers`` tells what each holds).  ``circle``: "marker" -- each timepoint's own x, y about
    the finder's window origin with the finder's radius, or ``radius`` (whole pixels: a number, or an array on (mark,)
    or (mark, time)) where the dataset no longer carries it; the fitted centre is then in image coordinates.  Or a
    DataArray / array on (mark[, time], 3) = {y, x, r} in window coordinates, in pixels: the fitted centre is in window
    coordinates too, and ``radius`` reports the start radius rounded to whole pixels.  Start circles are quantised as
    ``np.rint(v * 16)`` in float64.  The two square roots -- the radius from R^2, the rms from the mean square -- are
    taken here with NumPy."""
    from . import profile, refine

    roi_var = xp.data_vars["roi"]
    L, m, n_t = roi_var.sizes["roi_y"], roi_var.sizes["mark"], roi_var.sizes["time"]
    settings = refine.check_refine(rays, reach, polarity, reject, min_strength, min_rays, L)
    ch = channel_index(xp, channel, default=0)  # (a name or an index; None: the first channel)
    if isinstance(circle, str):
        if circle != "marker":
            raise ValueError(f'refine_circles: circle must be "marker" or the circles, got {circle!r}')
        y, x, top, left = (np.broadcast_to(v, (m, n_t)) for v in marker_windows(xp, L, None, "refine_circles", "circle"))
        r = refine.finder_radius(xp, radius)
        c = np.stack([y - top, x - left], axis=-1)  # as reduce.radial_profile(centre="marker") has them
        origin = np.stack([top, left], axis=-1).astype(np.float64)
        start = np.concatenate([c, r[..., None].astype(np.float64)], axis=-1)
    else:
        start = np.broadcast_to(per_marker("refine_circles", circle, m, n_t, 3, "circle"), (m, n_t, 3))
        origin = np.zeros((m, n_t, 2), dtype=np.float64)
        r = np.rint(np.clip(start[..., 2], 0.0, profile.INT_LIMIT)).astype(np.int64)
    circle_q = np.ascontiguousarray(profile.quantised(start))
    if m == 0:
        info, fit = np.zeros((0, n_t, 4), dtype=np.int32), np.zeros((0, n_t, 5), dtype=np.float64)
    else:
        roi = device_tensor(roi_var, ROI_DIMS)
        info, fit = hotpath.refine_circles(roi[:, ch], circle_q, *settings)
        info, fit = info.cpu().numpy(), fit.cpu().numpy()
    centre = origin + circle_q[..., :2].astype(np.float64) / 16.0  # the start centre as the kernel had it
    dims = ("mark", "time")
    return {
        "x_fit": DataArray(centre[..., 1] + fit[..., 1], dims), "y_fit": DataArray(centre[..., 0] + fit[..., 0], dims),
        "radius_fit": DataArray(np.sqrt(fit[..., 2]), dims), "fit_rms": DataArray(np.sqrt(fit[..., 3]), dims),
        "fit_strength": DataArray(np.ascontiguousarray(fit[..., 4]), dims),
        "fit_rays": DataArray(np.ascontiguousarray(info[..., 1]), dims),
        "fit_status": DataArray(np.ascontiguousarray(info[..., 0]), dims),
        "fit_polarity": DataArray(np.ascontiguousarray(info[..., 3]), dims),
        "radius": DataArray(r.astype(np.int32), dims),
    }


def profile_mean(count, moments):
    """sum / n of a radial profile (torch tensors: count (...), moments (..., 2)), NaN where n = 0."""
    n = count.to(torch.float64)
    return torch.where(n > 0, moments[..., 0] / n, torch.full_like(n, float("nan")))


def profile_std(count, moments, ddof=0):
    """sqrt((sum x^2 - (sum x)^2 / n) / (n - ddof)) of a radial profile (torch tensors), NaN where n - ddof <= 0 (and
    where n = 0).  Raw moments cancel: the difference of two numbers of size n mean^2 carries an absolute error of about
    2^-53 n mean^2 even where both are exact, so the variance is only good to a relative 2^-53 (mean / std)^2 -- fine
    for 16-bit pixels (a ring of 600 pixels at 60000 +- 50 keeps 9 digits), useless for a float ring whose spread is
    below 1e-8 of its level; a result below zero is returned as 0.  ``masked_std`` has the two-pass form."""
    n = count.to(torch.float64)
    dof = n - float(ddof)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    m2 = torch.clamp(moments[..., 1] - moments[..., 0] * moments[..., 0] / safe, min=0.0)
    return torch.where((dof > 0) & (n > 0), torch.sqrt(m2 / torch.where(dof > 0, dof, torch.ones_like(dof))),
                       torch.full_like(n, float("nan")))


# ---- per-pixel unmixing: the channels combined at every pixel, then reduced per bead (mg_roi_unmix_stats) ------------------
_MTD = ("mark", "time", "derived")


def unmixed_stats(xp, matrix, channels=None, offset="bg_median", mask="fg", q=(0.5,), time=None):
    """(count, sum, order) of the per-pixel lanthanide volumes ``v = matrix @ (roi - offset)`` and ratios ``v_k / v_0``
    under ``mask``, as DataArrays on the device: count (mark, time, derived) int32, sum (mark, time, derived) float64
    and order (mark, time, derived, quantile, bound) = the two order statistics every fraction of ``q`` falls between
    (``hotpath.unmix_stats``; ``interpolate_quantiles`` turns them into quantiles).  ``derived``: the n_ln volumes, then
    the n_ln - 1 ratios to the first.  ``matrix`` (lanthanide, channel) over ``channels`` -- names of the channel
    coordinate or indices, default all.  ``offset``: "bg_median" -- ``masked_median(xp, "bg", time=time)``, handed over
    without leaving the device; None; or a DataArray on (mark, channel, time).  ``mask``: a coordinate name, a DataArray
    as in ``masked_stats``, or None: every pixel.  ``time=k``: of timepoint ``k`` only, selected before anything is
    read, as ``masked_median`` does."""
    from . import unmix

    roi_var = xp.data_vars["roi"]
    names = np.asarray(xp.coords["channel"].values).tolist() if "channel" in xp.coords else \
        list(range(roi_var.sizes["channel"]))
    idx = unmix.channel_indices(names, channels)
    w, ch = unmix.check_table(matrix, idx, roi_var.sizes["channel"])
    qs = unmix.check_q(q)
    if isinstance(offset, str) and offset != "bg_median":
        raise ValueError(f'unmixed_stats: offset must be "bg_median", None or a DataArray, got {offset!r}')
    if offset is not None and not isinstance(offset, (str, DataArray)):
        raise ValueError(f'unmixed_stats: offset must be "bg_median", None or a DataArray, got {type(offset).__name__}')
    if mask is not None and not isinstance(mask, (str, DataArray)):
        raise ValueError(f"unmixed_stats: mask must be None, a coordinate name or a DataArray, got {mask!r}")
    roi, mk = roi_windows(xp, mask, time)
    if isinstance(offset, str):
        off = masked_median(xp, "bg", time=time).data
    elif offset is not None:
        off = offset
        if time is not None and off.sizes.get("time", 1) != 1:
            off = off.isel(time=time_pick(time))
        off = device_tensor(off, _MCT).to(torch.float64)
    else:
        off = None
    count, total, order = hotpath.unmix_stats(roi, mk, w, ch, off, qs)
    coords = {"quantile": qs}
    return (DataArray(count, _MTD), DataArray(total, _MTD), DataArray(order, _MTD + ("quantile", "bound"), coords))
