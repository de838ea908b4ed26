"""A picture of a result, made where the result lies (reference: src/magnify/plot/image.py).

The reference's ``imshow`` opens a napari window; before it does, it builds a multiscale pyramid of the image
(plot/image.py:60-62), blends one additive colour layer per channel (:64-72) and paints the label map of the foreground
masks in image coordinates (``roi_to_image_labels``, :157-168).  That pixel work is done here on the device, in one
read-once pass over the ``(channel, time, im_y, im_x)`` image (csrc/mg_overview.hip), and what comes back is a small
RGB picture per timepoint -- not a viewer (deliberate differences).  tests/plot_ref.py restates the
contract in NumPy; the kernels match it bit for bit.

    rgb = mg.plot.overview(xp)                        # uint8 (time, y, x, rgb), device-resident
    mg.plot.write_png("t0.png", rgb[0].values)

``roishow`` is the other half of the reference's package (plot/image.py:14-49): every marker's ROI window side by side,
grouped by tag, ``bg`` in red and ``fg`` in green on top (csrc/mg_montage.hip); ``percentile_limits`` gives exact
percentiles of a resident stack as contrast limits (csrc/mg_percentile.hip).  tests/roishow_ref.py restates both
(DESIGN.md, section 19).

    lim = mg.plot.percentile_limits(xp, 1, 99.8, source="roi")
    rgb = mg.plot.roishow(xp, contrast_limits=lim)    # rgb.attrs["marks"]: the mark of every cell
"""
from __future__ import annotations

import math
import struct
import zlib

import numpy as np
import torch

from . import hotpath, preprocess, xr_lite
from ._dataset import MASK_DIMS, device_tensor
from .utils import window_origin
from .xr_lite import DataArray

MAX_LEVEL = hotpath.OVERVIEW_MAX_LEVEL
OVERLAYS = (None, "none", "outline", "fill")
COLOR_BY = ("mark", "valid")
# the colour of marker i is entry i % 8 (color_by="mark")
MARK_COLORS = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
               (70, 240, 240), (240, 50, 230))
# napari's choice for channel_axis: gray for one channel, magenta / green for two, this cycle beyond
_CYCLE = ((0.0, 1.0, 1.0), (1.0, 1.0, 0.0), (1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def default_level(h: int, w: int) -> int:
    """The smallest level in 0 .. 6 whose picture has at most 1024**2 pixels; 6 if none has."""
    for level in range(MAX_LEVEL + 1):
        s = 1 << level
        if -(h // -s) * -(w // -s) <= 1024 ** 2:
            return level
    return MAX_LEVEL


def default_colors(n_channels: int):
    if n_channels == 1:
        return [(1.0, 1.0, 1.0)]
    if n_channels == 2:
        return [(1.0, 0.0, 1.0), (0.0, 1.0, 0.0)]
    return [_CYCLE[c % len(_CYCLE)] for c in range(n_channels)]


def _check_level(level):
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= int(level) <= MAX_LEVEL:
        raise ValueError(f"level must be an integer in 0..{MAX_LEVEL}, got {level!r}")
    return int(level)


def _image(xp):
    """The dataset (stacked marks are handled by ``_markers``) and its image as a (C, T, H, W) device tensor: a missing
    ``channel`` / ``time`` counts as size 1; a host image is moved to the device."""
    xp = xr_lite.from_any(xp)
    if isinstance(xp, DataArray) or "image" not in xp.data_vars:
        raise AttributeError("Dataset must contain 'image' data variable.")
    v = xp.data_vars["image"]
    extra = [d for d in v.dims if d not in ("channel", "time", "im_y", "im_x")]
    if extra or "im_y" not in v.dims or "im_x" not in v.dims:
        raise ValueError(f"plot: image must have the dimensions (channel, time, im_y, im_x) or a subset, got {v.dims}")
    for d in ("time", "channel"):
        if d not in v.dims:
            v = v.expand_dims(d)
    data = v.transpose("channel", "time", "im_y", "im_x").data
    if not isinstance(data, torch.Tensor) or not data.is_cuda:
        data = preprocess.to_device(data)
    h, w = data.shape[2:]
    if data.stride(3) != 1 and w > 1 or data.stride(2) != w and h > 1:  # the kernels read contiguous planes
        data = data.contiguous()
    return xp, data


def _marker_var(xp, name, tail):
    """Variable ``name`` as a DataArray on (mark, time) + tail, marks stacked as the reference does
    (plot/image.py:55-56); a missing ``time`` counts as size 1.  Views only: nothing is copied."""
    v = xp.coords[name] if name in xp.coords else xp.data_vars[name]
    if "mark" not in v.dims and "mark_row" in v.dims and "mark_col" in v.dims:
        v = v.transpose("mark_row", "mark_col", ...)
        v = DataArray(v.data.reshape((v.shape[0] * v.shape[1],) + tuple(v.shape[2:])), ("mark",) + v.dims[2:])
    extra = [d for d in v.dims if d not in ("mark", "time") + tail]
    if extra or "mark" not in v.dims:
        raise ValueError(f"plot: {name} must have the dimensions {('mark', 'time') + tail} or a subset, got {v.dims}")
    v = v.transpose("mark", "time", *tail)
    return v if "time" in v.dims else v.expand_dims("time", 1)


def _has_rois(xp):
    return "roi" in xp and all(k in xp for k in ("fg", "x", "y"))


def _mask(xp, name, m, n_t, L):
    """Coordinate ``name`` as a (M, T, L, L) bool / uint8 device view (stride 0 along a time of size 1).  ``m`` / ``L``
    None: whatever the coordinate has."""
    a = device_tensor(_marker_var(xp, name, ("roi_y", "roi_x")), MASK_DIMS, as_mask=True)
    if m is None:
        m, L = a.shape[0], a.shape[-1]
        if a.shape[2] != L:
            raise ValueError(f"plot: {name} windows must be square, got {tuple(a.shape[2:])}")
        if a.shape[1] not in (1, n_t):
            raise ValueError(f"plot: {a.shape[1]} {name} timepoints for {n_t} image timepoints")
    elif tuple(a.shape[2:]) != (L, L) or a.shape[0] != m or a.shape[1] not in (1, n_t):
        raise ValueError(f"plot: {name} of shape {tuple(a.shape)} does not match {m} marks, {n_t} timepoints, L = {L}")
    return a.expand(m, n_t, L, L)


def _markers(xp, n_t, h, w):
    """(fg (M, T, L, L) device view, origin (M, T, 2) int32 on the host, valid (M, T) bool) of a dataset with ROIs."""
    fg = _mask(xp, "fg", None, n_t, None)
    m, L = fg.shape[0], fg.shape[-1]
    if L > h or L > w:
        raise ValueError(f"plot: roi windows of length {L} do not fit a {h} x {w} image")

    def per_time(name, dtype):
        a = _marker_var(xp, name, ()).data
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return np.broadcast_to(a.reshape(m, -1) if m else a.reshape(0, 1), (m, n_t)).astype(dtype)

    x, y = per_time("x", np.float64), per_time("y", np.float64)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("plot: marker positions x / y must be finite")
    valid = per_time("valid", bool) if "valid" in xp else np.ones((m, n_t), dtype=bool)
    # truncated as the reference's roi_to_image_labels does; the finders round half to even
    origin = np.stack([window_origin(y.astype(int), L, h), window_origin(x.astype(int), L, w)], axis=-1)
    return fg, origin.astype(np.int32), valid


def _labels(xp, image, level):
    """(labels (T, hk, wk) int32 on the device, valid (M, T)) of a dataset with ROIs."""
    n_t, h, w = image.shape[1:]
    fg, origin, valid = _markers(xp, n_t, h, w)
    return hotpath.image_labels(fg, origin, level, h, w), valid


def roi_to_image_labels(xp, level=0):
    """The label map of the foreground masks in image coordinates, int32 ``(time, y, x)`` on the device: marker
    ``i + 1`` (stacked mark order) where a set pixel of ``fg[i, t]`` falls, 0 elsewhere; where masks overlap the largest
    index wins -- at ``level=0`` the reference's ``roi_to_image_labels`` (plot/image.py:157-168), at ``level=k`` its
    ``2**k`` block maximum."""
    level = _check_level(level)
    xp, image = _image(xp)
    if not _has_rois(xp):
        raise AttributeError("Dataset must contain 'roi' data variable with 'fg', 'x' and 'y' coordinates.")
    labels, _ = _labels(xp, image, level)
    return DataArray(labels, ("time", "y", "x"), name="fg_labels")


def _picture_args(what, xp, level, overlay, alpha, colors, contrast_limits):
    """What ``overview`` and ``roishow`` (``what``) check alike, the arguments that need no data first -> (dataset, its
    (C, T, H, W) image or (M, C, T, L, L) roi on the device, level or None, alpha, colors (C, 3) float64,
    contrast_limits (C, 2) float64 or None)."""
    if level is not None:
        level = _check_level(level)
    if overlay not in OVERLAYS:
        raise ValueError(f"overlay must be one of {OVERLAYS}, got {overlay!r}")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha!r}")
    xp, data = _image(xp) if what == "overview" else _roi(xp)
    c = data.shape[0 if what == "overview" else 1]
    if c > hotpath.OVERVIEW_MAX_CHANNELS:
        raise ValueError(f"plot.{what} composes at most {hotpath.OVERVIEW_MAX_CHANNELS} channels, got {c}")
    cols = np.asarray(default_colors(c) if colors is None else colors, dtype=np.float64)
    if cols.shape != (c, 3):
        raise ValueError(f"colors must be one RGB triple per channel: {c} triples, got shape {cols.shape}")
    if not (np.isfinite(cols).all() and (cols >= 0).all() and (cols <= 1).all()):
        raise ValueError("colors must lie in [0, 1]")
    if contrast_limits is not None:
        contrast_limits = np.asarray(contrast_limits, dtype=np.float64)
        if contrast_limits.shape != (c, 2):
            raise ValueError("contrast_limits must be one (lo, hi) pair per channel: "
                             f"{c} pairs, got shape {contrast_limits.shape}")
    return xp, data, level, alpha, cols, contrast_limits


def _limits(xp, image, contrast_limits):
    c, t, h, w = image.shape
    if contrast_limits is not None:
        return contrast_limits
    cached = xp._cache.get("image_minmax")
    if cached is not None and cached[0] == image.data_ptr() and cached[1] is not None and cached[1].numel() == c * t * 2:
        mm = cached[1]
    else:
        mm = torch.stack([hotpath.plane_minmax(image[k]) for k in range(c)])
    mm = mm.view(c, t, 2).cpu().numpy()
    lim = np.stack([mm[..., 0].min(axis=1), mm[..., 1].max(axis=1)], axis=1)
    if not np.isfinite(lim).all():
        raise ValueError(f"plot: the image's min / max are not finite ({lim.tolist()}); pass contrast_limits")
    return lim


def overview(xp, level=None, contrast_limits=None, colors=None, overlay="outline", color_by="mark", alpha=0.7):
    """The composite picture of a result, uint8 ``(time, y, x, rgb)`` on the device.

    ``xp``: what ``mg.beads``, ``mg.mrbles``, ``mg.microfluidic_chip``, ``mg.image`` or their ``*_pipe`` forms return,
    before or after ``restore_format``.  Every ``2**level`` block of a plane becomes one pixel (its mean; ``level=None``:
    the smallest level whose picture has at most 1024**2 pixels), scaled by the channel's ``contrast_limits`` (``(lo,
    hi)`` per channel; None: its min / max over all timepoints) and added in the channel's colour (``colors``: RGB in
    [0, 1] per channel; None: white, magenta / green, or the cycle cyan, yellow, magenta, red, green, blue).  A dataset
    with ROIs gets the foreground masks on top, where each timepoint's masks sit at that timepoint: ``overlay="fill"``
    blends the marker's colour with weight ``alpha``, ``"outline"`` paints the rim of every mask, ``"none"`` / None
    leaves the image alone.  ``color_by="mark"``: a colour per marker (``MARK_COLORS[i % 8]``); ``"valid"``: green
    where ``valid[i, t]``, red elsewhere."""
    if color_by not in COLOR_BY:
        raise ValueError(f"color_by must be one of {COLOR_BY}, got {color_by!r}")
    xp, image, level, alpha, cols, contrast_limits = _picture_args("overview", xp, level, overlay, alpha, colors,
                                                                   contrast_limits)
    c, t, h, w = image.shape
    if level is None:
        level = default_level(h, w)
    limits = _limits(xp, image, contrast_limits)
    labels = table = None
    if overlay in ("outline", "fill") and _has_rois(xp):
        labels, valid = _labels(xp, image, level)
        m = valid.shape[0]
        if color_by == "mark":
            tab = np.repeat(np.asarray(MARK_COLORS, dtype=np.uint8)[np.arange(m) % len(MARK_COLORS)][:, None], t, axis=1)
        else:
            tab = np.where(valid[..., None], np.array([0, 255, 0], dtype=np.uint8), np.array([255, 0, 0], dtype=np.uint8))
        table = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.uint8)).to(image.device)
    rgb = hotpath.render_overview(image, level, limits, cols, labels, table, overlay, alpha)
    return DataArray(rgb, ("time", "y", "x", "rgb"), name="overview", attrs={"level": level})


def write_png(path, rgb):
    """One ``(y, x, 3)`` uint8 array (NumPy, tensor or DataArray) as an 8-bit RGB PNG; standard library only."""
    if isinstance(rgb, DataArray):
        rgb = rgb.values
    elif isinstance(rgb, torch.Tensor):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f"write_png takes one (y, x, 3) uint8 array, got {rgb.dtype} {rgb.shape}")
    h, w = rgb.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)  # filter type 0 in front of every row
    rows[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


# ---- roishow: every marker's window side by side; percentile contrast limits ------------------------------------------

percentile_rank = hotpath.percentile_rank
SOURCES = ("image", "roi")


def _roi(xp):
    """The dataset and its ``roi`` as a (M, C, T, L, L) device view, marks stacked as ``_marker_var`` stacks them; a
    missing ``channel`` / ``time`` counts as size 1; a host block is moved to the device."""
    xp = xr_lite.from_any(xp)
    if isinstance(xp, DataArray) or "roi" not in xp.data_vars:
        raise AttributeError("Dataset must contain 'roi' data variable.")
    has_channel = "channel" in xp.data_vars["roi"].dims
    data = _marker_var(xp, "roi", ("channel", "roi_y", "roi_x")).data  # (mark, time, [channel,] roi_y, roi_x)
    if not isinstance(data, torch.Tensor) or not data.is_cuda:
        data = preprocess.to_device(data)
    data = data.permute(0, 2, 1, 3, 4) if has_channel else data.unsqueeze(1)
    if data.shape[3] != data.shape[4]:
        raise ValueError(f"plot: roi windows must be square, got {tuple(data.shape[3:])}")
    return xp, data


def _check_percentiles(lo, hi, source):
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= 100.0 and 0.0 <= hi <= 100.0) or lo > hi:
        raise ValueError(f"percentiles must satisfy 0 <= lo <= hi <= 100, got lo={lo!r}, hi={hi!r}")
    if source not in SOURCES:
        raise ValueError(f"source must be one of {SOURCES}, got {source!r}")
    return lo, hi


def percentile_limits(xp, lo=1.0, hi=99.8, source="image"):
    """Per channel the ``lo``-th and ``hi``-th percentile of its pixels over all timepoints (``source="roi"``: of its
    window pixels over all marks and timepoints), float64 ``(channel, 2)`` on the host: what ``contrast_limits=`` of
    ``overview`` and ``roishow`` takes.  Exact order statistics of the non-NaN values: ``sorted(values)[k]`` with ``k =
    percentile_rank(N, q)``, the lower one where a percentile falls between two values; float64 pixels are rounded to
    float32 first.  The stack is read where it lies, once per pass (``hotpath.percentiles``)."""
    lo, hi = _check_percentiles(lo, hi, source)
    if source == "image":
        xp, image = _image(xp)
        views = [image[c] for c in range(image.shape[0])]
    else:
        xp, roi = _roi(xp)
        views = [roi[:, c] for c in range(roi.shape[1])]
    out = np.empty((len(views), 2), dtype=np.float64)
    for c, view in enumerate(views):
        try:
            out[c] = hotpath.percentiles(view, (lo, hi))
        except ValueError as e:
            raise ValueError(f"plot.percentile_limits: channel {c} of {source!r} has no value that is not NaN") from e
    return out


def montage_layout(tags, m, columns=None):
    """int32 ``(rows, cols)``: the mark shown in every cell of the montage, -1 for an empty one.  With ``tags`` (one per
    mark): the reference's grid (plot/image.py:16-23) -- one column per ``np.unique`` tag in that order, the marks of a
    tag from the top in ascending order, as many rows as the largest group.  ``tags=None``: mark order, row-major, over
    ``columns`` columns (None: ``ceil(sqrt(m))``)."""
    m = int(m)
    if tags is not None:
        tags = np.asarray(tags).reshape(-1)
        if len(tags) != m:
            raise ValueError(f"montage_layout: {len(tags)} tags for {m} marks")
        if m == 0:
            return np.zeros((0, 0), dtype=np.int32)
        names, inverse, counts = np.unique(tags, return_inverse=True, return_counts=True)
        layout = np.full((int(counts.max()), len(names)), -1, dtype=np.int32)
        for j in range(len(names)):
            marks = np.nonzero(inverse.reshape(-1) == j)[0]
            layout[:len(marks), j] = marks
        return layout
    if columns is not None and (isinstance(columns, bool) or not isinstance(columns, (int, np.integer)) or columns < 1):
        raise ValueError(f"columns must be an integer >= 1, got {columns!r}")
    if m == 0:
        return np.zeros((0, 0), dtype=np.int32)
    if columns is None:
        columns = math.isqrt(m - 1) + 1  # ceil(sqrt(m))
    columns = int(columns)
    layout = np.full(-(m // -columns) * columns, -1, dtype=np.int32)
    layout[:m] = np.arange(m, dtype=np.int32)
    return layout.reshape(-1, columns)


def montage_level(rows, cols, L):
    """The smallest level in 0 .. 6 at which the montage has at most 1024**2 pixels per timepoint; 6 if none has."""
    for level in range(MAX_LEVEL + 1):
        lk = -(L // -(1 << level))
        if rows * lk * cols * lk <= 1024 ** 2:
            return level
    return MAX_LEVEL


def roishow(xp, level=None, contrast_limits=None, colors=None, overlay="fill", alpha=0.7, group_by="tag", columns=None):
    """Every marker's ROI window side by side, uint8 ``(time, y, x, rgb)`` on the device: the picture the reference's
    ``roishow`` (plot/image.py:14-49) hands to a viewer.

    With ``group_by="tag"`` and a ``tag`` coordinate there is one column per tag (sorted) and the marks of a tag run
    from the top (``montage_layout``); otherwise the marks fill a grid of ``columns`` columns in mark order.  A cell
    is the window at ``2**level`` (block means; ``level=None``: the smallest level whose montage has at most 1024**2
    pixels), scaled and coloured per channel as in ``overview`` (``contrast_limits=None``: the min / max of the
    channel's windows), with the ``bg`` mask in red and the ``fg`` mask in green on top, each timepoint with its own
    masks: ``overlay="fill"`` blends with weight ``alpha``, ``"outline"`` paints the rim, ``"none"`` / None leaves the
    window alone.  Attributes of the result: ``level``, ``cell`` (the side of a cell), ``marks`` (the layout: the mark
    of every cell, -1 for an empty one), ``tags`` (the tag of every column, or None)."""
    if group_by not in (None, "tag"):
        raise ValueError(f"group_by must be 'tag' or None, got {group_by!r}")
    if columns is not None and (isinstance(columns, bool) or not isinstance(columns, (int, np.integer)) or columns < 1):
        raise ValueError(f"columns must be an integer >= 1, got {columns!r}")
    xp, roi, level, alpha, cols, limits = _picture_args("roishow", xp, level, overlay, alpha, colors, contrast_limits)
    m, c, t, L, _ = roi.shape
    tags = names = None
    if group_by == "tag" and "tag" in xp.coords:
        tags = np.asarray(_marker_tags(xp)).reshape(-1)
        names = np.unique(tags) if m else tags[:0]
    layout = montage_layout(tags, m, columns)
    if level is None:
        level = montage_level(layout.shape[0], layout.shape[1], L)
    lk = -(L // -(1 << level))
    attrs = {"level": level, "cell": lk, "marks": layout, "tags": names}
    if m == 0:
        empty = torch.zeros((t, 0, 0, 3), dtype=torch.uint8, device=roi.device)
        return DataArray(empty, ("time", "y", "x", "rgb"), name="roishow", attrs=attrs)
    if limits is None:
        limits = percentile_limits(xp, 0.0, 100.0, source="roi")
    fg = bg = None
    if overlay in ("outline", "fill"):
        fg, bg = (_mask(xp, name, m, t, L) if name in xp else None for name in ("fg", "bg"))
    rgb = hotpath.render_roi_montage(roi, layout, level, limits, cols, fg, bg, overlay, alpha)
    return DataArray(rgb, ("time", "y", "x", "rgb"), name="roishow", attrs=attrs)


def _marker_tags(xp):
    """The ``tag`` coordinate per stacked mark (over ``mark``, or over ``mark_row, mark_col`` row-major)."""
    v = xp.coords["tag"]
    if "mark" not in v.dims and "mark_row" in v.dims and "mark_col" in v.dims:
        v = v.transpose("mark_row", "mark_col")
    elif v.dims != ("mark",):
        raise ValueError(f"plot: tag must lie over mark or over (mark_row, mark_col), got {v.dims}")
    return np.asarray(v.values).reshape(-1)
