"""What every component asks of a Dataset before it calls the device: a variable as a device tensor in a given order of
dimensions, and a channel name or index as an index."""
from __future__ import annotations

import numpy as np
import torch

from . import hotpath
from .utils import to_list


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
