"""Depth stacks: fold the Z axis of a focal series on the device (not in the reference, whose reader refuses a Z axis,
reader.py:256-257; DESIGN.md, "Depth stacks").

A stack is a device tensor ``(..., Z, H, W)`` of uint8, uint16, float32 or float64.  ``project`` folds it to
``(..., H, W)`` -- the maximum, the mean, or one chosen slice per stack; ``focus_totals`` sums the modified Laplacian of
every slice; ``sharpest`` keeps the slice with the largest total; ``fuse`` picks per pixel the slice whose
neighbourhood is sharpest ("extended depth of field").  The component ``project_depth`` does one of these to a
DataArray / Dataset with a ``depth`` (or ``z``) dimension before ``standardize_format``; the pipelines take it as
``depth=``.  Every fold is one kernel of ``mg_depth.hip``; ``tests/depth_ref.py`` restates the contract in NumPy.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as nat
from . import registry
from ._dataset import page_view, plane_block
from .utils import int_in
from .xr_lite import DataArray, Dataset

TILE = nat.DEFINES["MG_DEPTH_TILE"]  # mg_depth_fuse: output tile of a workgroup (TILE x TILE pixels)
MAX_K, MAX_Z = nat.DEFINES["MG_DEPTH_MAX_K"], nat.DEFINES["MG_DEPTH_MAX_Z"]
METHODS = ("max", "mean", "sharpest", "focus")
_PROJECT = {"max": nat.DEFINES["MG_DEPTH_MAX"], "mean": nat.DEFINES["MG_DEPTH_MEAN"], "pick": nat.DEFINES["MG_DEPTH_PICK"]}


def check_window(window):
    """``window`` of ``fuse``: an odd integer, 3 .. 2 * MAX_K + 1.  Returns the half-width k."""
    if int_in("depth window", window, 3, 2 * MAX_K + 1) % 2 == 0:
        raise ValueError(f"depth window must be odd, got {window}")
    return int(window) // 2


def check_depth(method="max", window=9, z=None):
    """The settings of ``project_depth`` as the pipelines take them: ``method`` one of "max", "mean", "sharpest",
    "focus"; ``window`` as ``check_window``; with ``z`` (the stack's depth) also ``z >= 1`` and, for "focus",
    ``z <= 255`` (the index map is uint8).  ValueError otherwise."""
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"depth method must be one of {METHODS}, got {method!r}")
    check_window(window)
    if z is not None:
        if z < 1:
            raise ValueError("a depth stack needs at least one slice")
        if method == "focus" and z > MAX_Z:
            raise ValueError(f'depth method "focus" takes at most {MAX_Z} slices, got {z}')


def project(stack, method, pick=None):
    """(..., Z, H, W) -> (..., H, W) of the same dtype.  ``method`` "max": the maximum over z (a NaN in any slice gives
    NaN); "mean": integers rint(exact sum / Z), half to even; floats a float64 sum in slice order, / Z, cast; "pick":
    slice ``pick[...]`` of every stack (``pick``: integers of the leading shape, each in [0, Z): ValueError otherwise,
    checked on the host before the launch)."""
    from . import hotpath

    if method not in _PROJECT:
        raise ValueError(f'project method must be "max", "mean" or "pick", got {method!r}')
    b = plane_block(stack, "depth.project", trailing=3)
    picks = None
    if method == "pick":
        if pick is None:
            raise ValueError('project(..., "pick") needs the slice index of every stack')
        host = (pick.detach().cpu().numpy() if isinstance(pick, torch.Tensor) else np.asarray(pick)).reshape(-1)
        if host.dtype.kind not in "iu" or host.size != b.n:
            raise ValueError(f"pick must hold one integer per stack ({b.n}), got {host.size} of {host.dtype}")
        if b.n and (host.min() < 0 or host.max() >= b.z):
            raise ValueError(f"pick index outside [0, {b.z})")
        picks = torch.from_numpy(host.astype(np.int32)).to(b.block.device)
    out = torch.empty(b.lead + (b.h, b.w), dtype=b.block.dtype, device=b.block.device)
    if out.numel() == 0:
        return out
    hotpath._call("mg_depth_project", b.block.data_ptr(), out.data_ptr(), b.code, b.n, b.z, b.h, b.w, _PROJECT[method],
                  hotpath._ptr(picks), hotpath._stream())
    return out


def focus_totals(stack):
    """(..., Z, H, W) -> (..., Z): the modified Laplacian |2c - l - r| + |2c - u - d| (edge-clamped neighbours) summed
    over every slice.  int64 and exact for integer pixels (never negative, below 2^63), float64 for float pixels (a sum
    in no defined order)."""
    from . import hotpath

    b = plane_block(stack, "depth.focus_totals", trailing=3)
    integer = b.code in (nat.MG_U8, nat.MG_U16)
    totals = torch.empty(b.lead + (b.z,), dtype=torch.int64 if integer else torch.float64, device=b.block.device)
    if b.block.numel() == 0:  # no pixel: every total is zero
        return totals.zero_()
    hotpath._call("mg_depth_focus_totals", b.block.data_ptr(), b.code, b.n, b.z, b.h, b.w, totals.data_ptr(),
                  hotpath._stream())
    return totals


def first_argmax(totals):
    """The slice choice of ``sharpest`` on a host table (..., Z): best = -inf, chosen = 0, and for z = 0, 1, ...:
    total > best makes z the choice -- the first of equal totals wins, a NaN total never does.  -> int32 (...)."""
    totals = np.asarray(totals)
    chosen = np.zeros(totals.shape[:-1], dtype=np.int32)
    if totals.dtype.kind == "f":
        best = np.full(totals.shape[:-1], -np.inf)
    else:
        best = np.full(totals.shape[:-1], -1, dtype=np.int64)
    for z in range(totals.shape[-1]):
        better = totals[..., z] > best
        chosen[better] = z
        best = np.where(better, totals[..., z], best)
    return chosen


def sharpest(stack):
    """-> (image (..., H, W): the slice of every stack with the largest focus total, chosen (...) int32 on the device).
    The arg-max is taken on the host, where the table is tiny: on the exact totals for integer pixels, ties to the
    lowest z."""
    totals = focus_totals(stack)
    chosen = first_argmax(totals.cpu().numpy())
    image = project(stack, "pick", chosen)
    return image, torch.from_numpy(chosen).to(image.device)


def fuse(stack, window=9, want_index=True):
    """-> (image (..., H, W), index (..., H, W) uint8 or None): per pixel the slice whose modified Laplacian, summed
    over the ``window`` x ``window`` neighbourhood (positions outside the plane left out), is strictly largest -- the
    lowest z among equals, z = 0 for an all-equal stack, never a slice whose measure is NaN.  ``window`` odd, 3 .. 31;
    Z <= 255."""
    from . import hotpath

    k = check_window(window)
    b = plane_block(stack, "depth.fuse", trailing=3)
    if b.z > MAX_Z:
        raise ValueError(f"depth.fuse takes at most {MAX_Z} slices, got {b.z}")
    out = torch.empty(b.lead + (b.h, b.w), dtype=b.block.dtype, device=b.block.device)
    index = torch.empty(b.lead + (b.h, b.w), dtype=torch.uint8, device=b.block.device) if want_index else None
    if out.numel() == 0:
        return out, index
    hotpath._call("mg_depth_fuse", b.block.data_ptr(), b.code, b.n, b.z, b.h, b.w, k, out.data_ptr(), hotpath._ptr(index),
                  hotpath._stream())
    return out, index


def _depth_dim(dims, dim):
    if dim in dims:
        return dim
    if dim == "depth" and "z" in dims:
        return "z"
    raise ValueError(f"project_depth: no dimension {dim!r} in {tuple(dims)}")


@registry.component("project_depth")
def project_depth(xp, method="max", window=9, dim="depth"):
    """Fold the depth dimension of the tiles (a DataArray, or the ``tile`` of a Dataset, as the reader or the user
    hands it over, before ``standardize_format``): ``method`` "max", "mean", "sharpest" (the slice with the largest
    focus total, one per stack) or "focus" (per pixel, ``fuse`` with ``window``).  A dimension named ``z`` is taken for
    ``depth``; the pages are ``tile_y`` / ``tile_x`` or ``y`` / ``x``.  Every other dimension, coordinate and attribute
    is kept; ``attrs["depth_method"]`` records the method and, for "sharpest", ``attrs["depth_chosen"]`` the chosen
    slice of every stack as a nested list over the leading dimensions."""
    check_depth(method, window)
    view = page_view(xp, "tile", (("tile_y", "tile_x"), ("y", "x")), "project_depth",
                     fold=lambda dims: _depth_dim(dims, dim))
    xp, tile, name = view.source, view.var, view.fold
    check_depth(method, window, z=tile.sizes[name])
    chosen = None
    if method == "focus":
        image, _ = fuse(view.planes, window, want_index=False)
    elif method == "sharpest":
        image, chosen = sharpest(view.planes)
    else:
        image = project(view.planes, method)
    dims = view.lead + view.pages
    attrs = dict(xp.attrs, depth_method=method)
    if chosen is not None:
        attrs["depth_chosen"] = chosen.cpu().numpy().tolist()
    if view.is_array:
        coords = {k: v for k, v in xp.coords.items() if name not in v.dims}
        return DataArray(image, dims, coords, xp.name, attrs)
    out = Dataset(attrs=attrs)
    for k, v in xp.coords.items():
        if name not in v.dims:
            out.coords[k] = v
    for k, v in xp.data_vars.items():
        if k != "tile" and name not in v.dims:
            out.data_vars[k] = v
    out["tile"] = DataArray(image, dims, name="tile", attrs=tile.attrs)
    out._cache.update(xp._cache)
    return out
