"""Per-pixel linear unmixing (not in the reference, which unmixes one mean per bead -- identify.py:72-83): every pixel's
channels are combined into lanthanide volumes ``v = W x`` and ratios ``v_k / v_0`` on the device
(``mg_roi_unmix_stats`` reduces them per bead, ``mg_unmix_planes`` gives whole lanthanide images).  This module holds
what the host side decides: the unmixing matrix, the setting ``unmix=`` of ``identify_mrbles`` and the labels of the
derived values.  ``include/magnify_hip.h`` states the contract of the kernels, ``tests/unmix_ref.py`` restates it."""
from __future__ import annotations

import numpy as np

from . import _native as nat

MAX_CHANNELS, MAX_LN, MAX_Q, MAX_LEN = (nat.DEFINES[k] for k in ("MG_UNMIX_MAX_CHANNELS", "MG_UNMIX_MAX_LN",
                                                                  "MG_UNMIX_MAX_Q", "MG_UNMIX_MAX_LEN"))
MODES = ("pixel",)


def unmixing_matrix(spectra) -> np.ndarray:
    """The least-squares unmixing matrix W (lanthanide, channel), float64, of a (lanthanide, channel) table of
    reference spectra S: ``pinv(S.T)``, so that ``W @ I`` is the solution of ``S.T V = I`` that ``lstsq`` gives."""
    sp = np.asarray(spectra, dtype=np.float64)
    if sp.ndim != 2 or 0 in sp.shape:
        raise ValueError(f"unmixing_matrix: spectra must be a (lanthanide, channel) table, got shape {sp.shape}")
    if not np.isfinite(sp).all():
        raise ValueError("unmixing_matrix: a spectrum is not finite")
    return np.ascontiguousarray(np.linalg.pinv(sp.T), dtype=np.float64)


def check_unmix(unmix):
    """``unmix=`` of ``identify_mrbles`` and the mrbles pipelines: None (one least-squares system per bead, as the
    reference) or "pixel" (unmix every pixel, bead medians of the ratios).  ValueError for anything else."""
    if unmix is not None and not (isinstance(unmix, str) and unmix in MODES):
        raise ValueError(f'unmix must be None or one of {MODES}, got {unmix!r}')
    return unmix


def derived_names(lanthanides) -> list:
    """Labels of the D = 2 n - 1 derived values of a pixel, in the kernels' order: the volumes ``name``, then the ratios
    ``name/reference`` of every lanthanide but the first (the reference lanthanide)."""
    names = [str(n) for n in lanthanides]
    if not names:
        raise ValueError("derived_names: no lanthanides")
    return names + [f"{n}/{names[0]}" for n in names[1:]]


def check_table(matrix, channels, n_c):
    """(W float64 (n_ln, n_k) contiguous, channels int32 (n_k,)) as the kernels take them; ``channels`` None: all
    ``n_c`` in order.  ValueError for what they refuse: a matrix that is not 2-D, has 0 or more than MAX_LN rows or a
    non-finite entry; 0 or more than MAX_CHANNELS channels, a channel outside [0, n_c), a repeated one, a count that
    differs from the matrix's columns."""
    w = np.ascontiguousarray(matrix, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError(f"unmix: the matrix must be (lanthanide, channel), got shape {w.shape}")
    ch = np.arange(n_c, dtype=np.int32) if channels is None else np.asarray(channels)
    if ch.ndim != 1 or (ch.size and not np.issubdtype(ch.dtype, np.integer)):
        raise ValueError(f"unmix: channels must be a list of indices, got {channels!r}")
    ch = np.ascontiguousarray(ch, dtype=np.int32)
    if not 1 <= w.shape[0] <= MAX_LN:
        raise ValueError(f"unmix: 1 to {MAX_LN} lanthanides, got {w.shape[0]}")
    if not 1 <= len(ch) <= MAX_CHANNELS:
        raise ValueError(f"unmix: 1 to {MAX_CHANNELS} channels, got {len(ch)}")
    if w.shape[1] != len(ch):
        raise ValueError(f"unmix: the matrix has {w.shape[1]} columns for {len(ch)} channels")
    if ch.min() < 0 or ch.max() >= n_c:
        raise ValueError(f"unmix: channels {ch.tolist()} outside [0, {n_c})")
    if len(set(ch.tolist())) != len(ch):
        raise ValueError(f"unmix: a channel is repeated in {ch.tolist()}")
    if not np.isfinite(w).all():
        raise ValueError("unmix: a matrix entry is not finite")
    return w, ch


def check_q(q):
    """float64 (n_q,) of up to MAX_Q fractions in [0, 1]; ValueError otherwise."""
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1))
    if len(qs) > MAX_Q:
        raise ValueError(f"unmix: at most {MAX_Q} quantiles, got {len(qs)}")
    if len(qs) and not ((qs >= 0.0) & (qs <= 1.0)).all():  # (NaN fails both)
        raise ValueError(f"unmix: quantiles must lie in [0, 1], got {qs.tolist()}")
    return qs


def channel_indices(names, channels):
    """Indices of ``channels`` -- names of the dataset's channel coordinate, or indices -- None: all of them."""
    names = [str(c) for c in names]
    if channels is None:
        return list(range(len(names)))
    out = []
    for c in channels:
        if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
            out.append(int(c))
        elif str(c) in names:
            out.append(names.index(str(c)))
        else:
            raise ValueError(f"unmix: no channel {c!r} among {names}")
    return out


def planes(image, matrix, channels=None, offset=None, ratios=False):
    """Lanthanide images: ``image`` -- a device tensor (C, H, W) or (C, T, H, W), or a dataset's ``image`` DataArray on
    (channel, time, im_y, im_x) -- unmixed at every pixel by ``matrix`` (lanthanide, channel) over ``channels`` (indices;
    for a DataArray also names; default all).  ``offset``: one constant per used channel, subtracted first.  Returns
    float32 (n_out, [T,] H, W) on the device: the volumes, followed by the ratios to the first lanthanide where
    ``ratios`` (``hotpath.unmix_planes``).  A DataArray gives a DataArray on (derived, time, im_y, im_x)."""
    import torch

    from . import hotpath
    from ._dataset import device_tensor
    from .xr_lite import DataArray

    if isinstance(image, DataArray):
        dims = ("channel", "time", "im_y", "im_x")
        names = np.asarray(image.coords["channel"].values).tolist() if "channel" in image.coords else \
            list(range(image.sizes["channel"]))
        idx = channel_indices(names, channels)
        out = hotpath.unmix_planes(device_tensor(image, dims), matrix, idx, offset, ratios)
        return DataArray(out, ("derived",) + dims[1:])
    if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4):
        raise ValueError("unmix.planes: a device tensor (C, H, W) or (C, T, H, W), or a dataset's image")
    out = hotpath.unmix_planes(image if image.dim() == 4 else image[:, None], matrix, channels, offset, ratios)
    return out if image.dim() == 4 else out[:, 0]
