"""What every component asks of a Dataset before it calls the device: a variable as a device tensor in a given order of
dimensions, a channel name or index as an index, the pages of a variable as a block of planes (``page_view``) and a
tensor of planes as the contiguous block an entry of the library takes (``plane_block``)."""
from __future__ import annotations

import collections
import dataclasses
import functools

import numpy as np
import torch

from . import _native as nat
from . import hotpath
from .utils import to_list
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
