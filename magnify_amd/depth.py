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
from . import registry, xr_lite
from .xr_lite import DataArray, Dataset

TILE = nat.DEFINES["MG_DEPTH_TILE"]  # mg_depth_fuse: output tile of a workgroup (TILE x TILE pixels)
MAX_K, MAX_Z = nat.DEFINES["MG_DEPTH_MAX_K"], nat.DEFINES["MG_DEPTH_MAX_Z"]
METHODS = ("max", "mean", "sharpest", "focus")
_PROJECT = {"max": nat.DEFINES["MG_DEPTH_MAX"], "mean": nat.DEFINES["MG_DEPTH_MEAN"], "pick": nat.DEFINES["MG_DEPTH_PICK"]}


def check_window(window):
    """``window`` of ``fuse``: an odd integer, 3 .. 2 * MAX_K + 1.  Returns the half-width k."""
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)):
        raise ValueError(f"depth window must be an integer, got {window!r}")
    if window % 2 == 0 or window < 3 or window > 2 * MAX_K + 1:
        raise ValueError(f"depth window must be odd and in [3, {2 * MAX_K + 1}], got {window}")
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


def _block(stack, what):
    """-> (the stack as a contiguous tensor, leading shape, n, z, h, w, dtype code).  Raises before any launch."""
    from . import hotpath

    if not isinstance(stack, torch.Tensor):
        raise TypeError(f"{what} takes a device tensor (..., Z, H, W), got {type(stack).__name__}")
    code = nat.dtype_code(stack.dtype)  # TypeError for an unsupported dtype
    if stack.dim() < 3:
        raise ValueError(f"{what} takes a stack (..., Z, H, W), got shape {tuple(stack.shape)}")
    hotpath.require_gpu()
    if not stack.is_cuda:
        raise ValueError(f"{what} takes a device tensor; move it with preprocess.to_device")
    lead = tuple(stack.shape[:-3])
    z, h, w = (int(v) for v in stack.shape[-3:])
    if z < 1:
        raise ValueError(f"{what}: a depth stack needs at least one slice")
    return stack.contiguous(), lead, int(np.prod(lead, dtype=np.int64)), z, h, w, code


def project(stack, method, pick=None):
    """(..., Z, H, W) -> (..., H, W) of the same dtype.  ``method`` "max": the maximum over z (a NaN in any slice gives
    NaN); "mean": integers rint(exact sum / Z), half to even; floats a float64 sum in slice order, / Z, cast; "pick":
    slice ``pick[...]`` of every stack (``pick``: integers of the leading shape, each in [0, Z): ValueError otherwise,
    checked on the host before the launch)."""
    from . import hotpath

    if method not in _PROJECT:
        raise ValueError(f'project method must be "max", "mean" or "pick", got {method!r}')
    block, lead, n, z, h, w, code = _block(stack, "depth.project")
    picks = None
    if method == "pick":
        if pick is None:
            raise ValueError('project(..., "pick") needs the slice index of every stack')
        host = (pick.detach().cpu().numpy() if isinstance(pick, torch.Tensor) else np.asarray(pick)).reshape(-1)
        if host.dtype.kind not in "iu" or host.size != n:
            raise ValueError(f"pick must hold one integer per stack ({n}), got {host.size} of {host.dtype}")
        if n and (host.min() < 0 or host.max() >= z):
            raise ValueError(f"pick index outside [0, {z})")
        picks = torch.from_numpy(host.astype(np.int32)).to(block.device)
    out = torch.empty(lead + (h, w), dtype=block.dtype, device=block.device)
    if out.numel() == 0:
        return out
    hotpath._call("mg_depth_project", block.data_ptr(), out.data_ptr(), code, n, z, h, w, _PROJECT[method],
                  hotpath._ptr(picks), hotpath._stream())
    return out


def focus_totals(stack):
    """(..., Z, H, W) -> (..., Z): the modified Laplacian |2c - l - r| + |2c - u - d| (edge-clamped neighbours) summed
    over every slice.  int64 and exact for integer pixels (never negative, below 2^63), float64 for float pixels (a sum
    in no defined order)."""
    from . import hotpath

    block, lead, n, z, h, w, code = _block(stack, "depth.focus_totals")
    integer = code in (nat.MG_U8, nat.MG_U16)
    totals = torch.empty(lead + (z,), dtype=torch.int64 if integer else torch.float64, device=block.device)
    if block.numel() == 0:  # no pixel: every total is zero
        return totals.zero_()
    hotpath._call("mg_depth_focus_totals", block.data_ptr(), code, n, z, h, w, totals.data_ptr(), hotpath._stream())
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
    block, lead, n, z, h, w, code = _block(stack, "depth.fuse")
    if z > MAX_Z:
        raise ValueError(f"depth.fuse takes at most {MAX_Z} slices, got {z}")
    out = torch.empty(lead + (h, w), dtype=block.dtype, device=block.device)
    index = torch.empty(lead + (h, w), dtype=torch.uint8, device=block.device) if want_index else None
    if out.numel() == 0:
        return out, index
    hotpath._call("mg_depth_fuse", block.data_ptr(), code, n, z, h, w, k, out.data_ptr(), hotpath._ptr(index),
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
    from .preprocess import to_device

    check_depth(method, window)
    xp = xr_lite.from_any(xp)
    is_array = isinstance(xp, DataArray)
    if not is_array and "tile" not in xp.data_vars:
        raise ValueError("project_depth: the Dataset has no 'tile' variable")
    tile = xp if is_array else xp.data_vars["tile"]
    name = _depth_dim(tile.dims, dim)
    pages = next((p for p in (("tile_y", "tile_x"), ("y", "x")) if p[0] in tile.dims and p[1] in tile.dims), None)
    if pages is None:
        raise ValueError(f"project_depth: no page dimensions (tile_y, tile_x) or (y, x) in {tile.dims}")
    lead = tuple(d for d in tile.dims if d != name and d not in pages)
    check_depth(method, window, z=tile.sizes[name])
    moved = tile.transpose(*lead, name, *pages)
    data = moved.data
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data)
    stack = to_device(data)
    chosen = None
    if method == "focus":
        image, _ = fuse(stack, window, want_index=False)
    elif method == "sharpest":
        image, chosen = sharpest(stack)
    else:
        image = project(stack, method)
    dims = lead + pages
    attrs = dict(xp.attrs, depth_method=method)
    if chosen is not None:
        attrs["depth_chosen"] = chosen.cpu().numpy().tolist()
    if is_array:
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
