"""What every component asks of a Dataset before it calls the device: a variable as a device tensor in a given order of
dimensions, the gathered windows with a mask and one timepoint of them (``roi_windows``), a caller's array per marker, a
channel name or index as an index, the pages of a variable as a block of planes (``page_view``) and a
tensor of planes as the contiguous block an entry of the library takes (``plane_block``)."""
from __future__ import annotations

import collections
import dataclasses
import functools

import numpy as np
import torch

from . import _native as nat
from . import hotpath
from .utils import to_list, window_origin
from .xr_lite import DataArray, from_any


def device_tensor(var, dims, as_mask=False):
    """``var`` (a DataArray) on the device with its dimensions in the order of ``dims`` (those it has).  A host array is
    brought to native byte order and uploaded; a device tensor is used where it lies, nothing is copied.  ``as_mask``:
    bool / uint8 stay as they are, any other type becomes ``!= 0``.  ``time`` in ``dims`` but not in ``var`` (one mask
    for all timepoints) becomes an axis of size 1 at its place, which the window kernels read with stride 0."""
    have = [d for d in dims if d in var.dims]
    data = var.transpose(*have).data
    if not isinstance(data, torch.Tensor):
        data = np.asarray(data)
        if data.dtype.byteorder not in ("=", "|"):
            data = data.astype(data.dtype.newbyteorder("="))
        data = torch.from_numpy(np.ascontiguousarray(data))
    if as_mask and data.dtype not in (torch.bool, torch.uint8):
        data = data != 0
    if not data.is_cuda:
        hotpath.require_gpu()
        data = data.cuda()
    if "time" in dims and "time" not in var.dims:
        data = data.unsqueeze([d for d in dims if d in var.dims or d == "time"].index("time"))
    return data


ROI_DIMS, MASK_DIMS = ("mark", "channel", "time", "roi_y", "roi_x"), ("mark", "time", "roi_y", "roi_x")


def time_pick(time):
    """Timepoint ``time`` (-1: the last) as the slice of length 1 that keeps the time axis; None -- every timepoint --
    stays None."""
    if time is None:
        return None
    return slice(time, time + 1) if time != -1 else slice(-1, None)


def own_mask(fg, bg):
    """fg | bg, uint8, of the mask tensors (M, T', L, L) ``device_tensor`` gives: the pixels a bead owns (what
    ``segment_rois`` allows its foreground to grow into, what ``radial_profile`` reads).  One drawn mask for all
    timepoints -- T' = 1 or a time stride of 0 in both -- gives one union, a time axis of 1."""
    if all(t.shape[1] == 1 or t.stride(1) == 0 for t in (fg, bg)):
        fg, bg = fg[:, :1], bg[:, :1]
    return fg.view(torch.uint8) | bg.view(torch.uint8)


def roi_windows(xp, mask, time=None):
    """(roi (M, C, T, L, L), mask (M, T', L, L) or None) on the device.  ``mask``: a coordinate name, a DataArray on
    (mark[, time], roi_y, roi_x), None -- every pixel -- or "own": ``own_mask`` of a bead's fg and bg, every pixel on a
    chip (a dataset with a ``tag`` coordinate).  ``time=k``: timepoint ``k`` only, selected where the data lies: the
    others are neither moved nor read.  TypeError for a roi that is not uint8 / uint16 / float32 / float64."""
    roi, one = xp.data_vars["roi"], time_pick(time)
    if isinstance(mask, str) and mask == "own":
        mask = None if "tag" in xp.coords else DataArray(
            own_mask(*(device_tensor(xp.coords[k], MASK_DIMS, as_mask=True) for k in ("fg", "bg"))), MASK_DIMS)
    elif isinstance(mask, str):
        mask = xp.coords[mask]
    if one is not None:
        roi = roi.isel(time=one)
        if mask is not None and mask.sizes.get("time", 1) != 1:
            mask = mask.isel(time=one)
    roi = device_tensor(roi, ROI_DIMS)
    nat.dtype_code(roi.dtype)
    return roi, None if mask is None else device_tensor(mask, MASK_DIMS, as_mask=True)


def per_marker(what, value, m, n_t, k, keyword):
    """``value`` -- the ``keyword=`` argument of ``what``: a DataArray or an array on (mark[, time], k) -- as finite
    float64 (M, 1 or n_t, k).  ValueError otherwise."""
    if isinstance(value, DataArray):
        value = value.transpose(*[d for d in ("mark", "time") if d in value.dims], ...).values
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 2:
        a = a[:, None]
    if a.ndim != 3 or a.shape[0] != m or a.shape[2] != k or a.shape[1] not in (1, n_t):
        raise ValueError(f"{what}: {keyword}= must be (mark[, time], {k}) = {(m, n_t, k)}, got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: {keyword}= holds a value that is not finite")
    return a


def marker_windows(xp, L, time, what, keyword):
    """(y, x, top, left), each (mark, time): every marker's position and the origin of its window, the one the finder
    cut -- ``utils.window_origin`` of ``find._rounded_centres`` of that timepoint's x, y.  ``what`` and ``keyword``: who
    asks with ``keyword="marker"``, for the message where the dataset no longer knows the image size."""
    from .find import _rounded_centres

    if "im_y" not in xp.sizes or "im_x" not in xp.sizes:
        raise ValueError(f'{what}: {keyword}="marker" needs the image sizes im_y / im_x to find the window origins, and '
                         f"this dataset no longer has them (roi_only?): pass {keyword}= in window coordinates")
    x, y = (np.asarray(xp.coords[k].transpose(*[d for d in ("mark", "time") if d in xp.coords[k].dims]).values,
                       dtype=np.float64) for k in ("x", "y"))
    if x.ndim == 1:
        x, y = x[:, None], y[:, None]
    if time is not None:
        x, y = x[:, time_pick(time)], y[:, time_pick(time)]
    if x.size == 0:
        return y, x, np.zeros(x.shape, dtype=np.int64), np.zeros(x.shape, dtype=np.int64)
    rc = _rounded_centres(y, x).reshape(x.shape + (2,))
    return y, x, window_origin(rc[..., 0], L, xp.sizes["im_y"]), window_origin(rc[..., 1], L, xp.sizes["im_x"])


def marker_centres(xp, L, time, what="radial_profile", keyword="centre"):
    """(mark, time, 2) float64 {y - top, x - left}: every marker's position inside its own window
    (``marker_windows``)."""
    y, x, top, left = marker_windows(xp, L, time, what, keyword)
    return np.stack([y - top, x - left], axis=-1)


class ChannelError(KeyError, ValueError):
    """No such channel: caught as either type, as the finders (KeyError) and the filters (ValueError) raised it."""


def channel_index(assay, channel, default=None):
    """Index of ``channel``: a name of the ``channel`` coordinate, else a (non-bool) integer in range; None gives
    ``default``.  ChannelError otherwise."""
    if channel is None:
        return default
    names = np.asarray(assay.coords["channel"].values).tolist() if "channel" in assay.coords else None
    if names is not None and channel in names:
        return names.index(channel)
    if isinstance(channel, (int, np.integer)) and not isinstance(channel, (bool, np.bool_)) and \
            0 <= channel < assay.sizes["channel"]:
        return int(channel)
    raise ChannelError(f"channel {channel!r} not found: names {names}, {assay.sizes.get('channel', 0)} channels")


def channel_indexes(assay, channels):
    """Indices of ``channels`` (one or a list; None: every channel), each as ``channel_index`` has it."""
    if channels is None:
        return list(range(assay.sizes["channel"]))
    return [channel_index(assay, c) for c in to_list(channels)]


# ``block``: the planes as a contiguous device tensor ``lead + (h, w)`` or ``lead + (z, h, w)``; ``n``: the product of
# ``lead``; ``code``: the dtype's MG_* code; ``z``: None for planes
PlaneBlock = collections.namedtuple("PlaneBlock", "block lead n h w code z")


def plane_block(x, what, trailing=2):
    """``x`` (..., H, W), or with ``trailing=3`` a depth stack (..., Z, H, W), as a ``PlaneBlock``.  Raises before any
    launch: TypeError for anything but a tensor of uint8, uint16, float32 or float64, ValueError for too few dimensions,
    a host tensor or a stack without a slice."""
    shape, noun = ("(..., Z, H, W)", "a stack") if trailing == 3 else ("(..., H, W)", "planes")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what} takes a device tensor {shape}, got {type(x).__name__}")
    code = nat.dtype_code(x.dtype)  # TypeError for an unsupported dtype
    if x.dim() < trailing:
        raise ValueError(f"{what} takes {noun} {shape}, got shape {tuple(x.shape)}")
    hotpath.require_gpu()
    if not x.is_cuda:
        raise ValueError(f"{what} takes a device tensor; move it with preprocess.to_device")
    lead, (h, w) = tuple(x.shape[:-trailing]), (int(v) for v in x.shape[-2:])
    z = int(x.shape[-3]) if trailing == 3 else None
    if z is not None and z < 1:
        raise ValueError(f"{what}: a depth stack needs at least one slice")
    return PlaneBlock(x.contiguous(), lead, int(np.prod(lead, dtype=np.int64)), h, w, code, z)


@dataclasses.dataclass(frozen=True)
class PageView:
    """The variable ``var``, called ``name``, of ``source`` (a DataArray: itself) seen as planes: ``pages`` are its two
    page dimensions, ``fold`` a dimension the component folds (or None), ``lead`` all the others, as planes are counted."""
    source: object
    name: str
    var: DataArray
    lead: tuple
    pages: tuple
    fold: str | None = None
    is_array = property(lambda self: isinstance(self.source, DataArray))

    @functools.cached_property
    def planes(self):
        """The variable as a contiguous device tensor ``lead + pages``, or ``lead + (fold,) + pages`` (uploaded once)."""
        from .preprocess import to_device

        data = self.var.transpose(*self.lead, *(() if self.fold is None else (self.fold,)), *self.pages).data
        return to_device(np.ascontiguousarray(data) if isinstance(data, np.ndarray) else data)

    def rebuild(self, out, extra_attrs):
        """``out`` (``lead + pages``) in the variable's place and order of dimensions: a DataArray with the source's
        coordinates, name and attributes, or a copy of the Dataset with the variable replaced; ``extra_attrs`` added to
        the attributes either way.  The source is left as it is."""
        var, src = self.var, self.source
        new = DataArray(out, self.lead + self.pages, None, var.name, var.attrs).transpose(*var.dims)
        if self.is_array:
            return DataArray(new.raw, var.dims, dict(src.coords), src.name, dict(src.attrs, **extra_attrs))
        res = src.copy()
        res.attrs.update(extra_attrs)
        res[self.name] = new
        return res


def page_view(xp, name, page_names, what, fold=None, first=()):
    """``xp`` itself (a DataArray) or its variable ``name`` (a Dataset) as a ``PageView``.  ``page_names``: the pairs of
    page dimensions to look for, in that order; ``what``: the component, for the messages; ``fold``: a dimension kept out
    of ``lead``, or a function that picks it from the variable's dimensions; ``first``: dimensions that come first in
    ``lead`` where the variable has them.  ValueError for a Dataset without the variable and for a variable without page
    dimensions.  Nothing is uploaded yet."""
    xp = from_any(xp)
    if not isinstance(xp, DataArray) and name not in xp.data_vars:
        raise ValueError(f"{what}: the Dataset has no {name!r} variable")
    var = xp if isinstance(xp, DataArray) else xp.data_vars[name]
    fold = fold(var.dims) if callable(fold) else fold
    pages = next((p for p in page_names if p[0] in var.dims and p[1] in var.dims), None)
    if pages is None:
        raise ValueError(f"{what}: no page dimensions {' or '.join(f'({a}, {b})' for a, b in page_names)} in {var.dims}")
    rest = tuple(d for d in var.dims if d not in pages and d != fold)
    return PageView(xp, name, var, tuple(d for d in first if d in rest) + tuple(d for d in rest if d not in first), pages, fold)
