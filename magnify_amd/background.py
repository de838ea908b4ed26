"""Background: estimate the additive, slowly varying part of every plane as its grey opening with a large square
window and subtract it, on the device (not in the reference, whose finders scale every plane by its global minimum and
maximum, utils.py:20-27, so that a gradient across the plane takes the grey levels the markers need; DESIGN.md,
"Background").

Planes are a device tensor ``(..., H, W)`` of uint8, uint16, float32 or float64.  ``estimate`` is the opening --
``scipy.ndimage.grey_opening(size=2 * radius + 1, mode="nearest")`` on planes without NaN -- of the planes themselves
or, with ``smooth`` = 1 or 2, of their window median of that radius (``despeckle.median``), so that a dark pixel does
not pull the background down around it; ``subtract`` is the plane minus it, clamped at 0.  The window has to be wider
than the widest marker: what fits into it is kept, what does not is background.  The component ``subtract_background``
does this to the ``image`` of a Dataset; the pipelines take it as ``background=``.  The kernels are in
``mg_background.hip``; ``tests/background_ref.py`` restates the contract in NumPy.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as nat
from . import registry, xr_lite
from .utils import to_list
from .xr_lite import DataArray

MAX_RADIUS = nat.DEFINES["MG_BACKGROUND_MAX_RADIUS"]
ROWS = nat.DEFINES["MG_BACKGROUND_ROWS"]  # the vertical kernel: output rows / columns (at most) of a workgroup's step
COLS = nat.DEFINES["MG_BACKGROUND_COLS"]
SPAN = nat.DEFINES["MG_BACKGROUND_SPAN"]  # the horizontal kernels: output columns of a workgroup's step
SMOOTH = (0, 1, 2)
SCRATCH_LIMIT = 512 << 20  # bytes of scratch per call of the entry (one plane's, where a single plane needs more)
_MODES = {"estimate": nat.DEFINES["MG_BACKGROUND_ESTIMATE"], "subtract": nat.DEFINES["MG_BACKGROUND_SUBTRACT"]}


def check_background(radius, smooth=0, channel=None):
    """The settings of ``subtract_background`` as the pipelines take them: ``radius`` an integer in 1 .. MAX_RADIUS,
    ``smooth`` 0, 1 or 2, ``channel`` None, a name (a string or an integer index) or a list of them.  ValueError
    otherwise."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"background radius must be an integer in 1 .. {MAX_RADIUS}, got {radius!r}")
    if isinstance(smooth, (bool, np.bool_)) or not isinstance(smooth, (int, np.integer)) or smooth not in SMOOTH:
        raise ValueError(f"background smooth must be one of {SMOOTH}, got {smooth!r}")
    if channel is not None:
        names = to_list(channel)
        if not names or any(isinstance(c, (bool, np.bool_)) or not isinstance(c, (str, int, np.integer)) for c in names):
            raise ValueError(f"background channel must be a channel name or a list of names, got {channel!r}")


def _run(planes, radius, smooth, what):
    from . import hotpath
    from .despeckle import _ALL, _block

    check_background(radius, smooth)
    block, lead, n, h, w, code = _block(planes, f"background.{what}")
    out = torch.empty_like(block)
    if block.numel() == 0:
        return out
    per_plane = nat.lib().mg_background_scratch_bytes(code, 1, h, w, radius)  # (a host function: nothing is launched)
    if per_plane < 0:
        raise ValueError(f"background.{what}: planes of {h} x {w} are refused (mg_background_scratch_bytes)")
    plane_bytes = h * w * block.element_size()
    held = per_plane + (plane_bytes if smooth else 0)  # with smoothing the filtered planes of a group are held too
    group = min(n, max(1, SCRATCH_LIMIT // held))
    scratch = torch.empty(group * held, dtype=torch.uint8, device=block.device)
    src, dst = block.view(n, h, w), out.view(n, h, w)
    for i in range(0, n, group):
        m = min(group, n - i)
        part, filtered, work = src[i:i + m], 0, scratch.data_ptr()
        if smooth:
            filtered, work = work, work + group * plane_bytes
            hotpath._call("mg_despeckle_planes", part.data_ptr(), filtered, code, m, h, w, smooth, _ALL, 0.0, 0, 0,
                          hotpath._stream())
        hotpath._call("mg_background_planes", part.data_ptr(), filtered, dst[i:i + m].data_ptr(), code, m, h, w, radius,
                      _MODES[what], work, m * per_plane, hotpath._stream())
    return out


def estimate(planes, radius, smooth=0):
    """(..., H, W) -> the background of every plane: the maximum over the (2 * radius + 1)^2 window of the minimum over
    that window (positions outside the plane and NaN pixels left out) of the plane, or of its median of radius
    ``smooth``."""
    return _run(planes, radius, smooth, "estimate")


def subtract(planes, radius, smooth=0):
    """(..., H, W) -> plane - background where the plane is above it, else 0, in the planes' dtype; NaN where either
    is.  Without smoothing the background is nowhere above the plane; with it the clamp does take part."""
    return _run(planes, radius, smooth, "subtract")


@registry.component("subtract_background")
def subtract_background(xp, radius, smooth=0, channel=None):
    """Subtract the background of the stitched image (a DataArray, or the ``image`` of a Dataset).  The pages are
    ``im_y`` / ``im_x`` or ``y`` / ``x``; every other dimension counts planes.  ``channel``: a name or a list of names
    -- only these channels' planes are changed, the others pass through bit for bit (None: every plane).  Every
    dimension, coordinate and attribute is kept; ``attrs["background_radius"]`` is the radius."""
    from ._dataset import channel_indexes
    from .preprocess import to_device

    check_background(radius, smooth, channel)
    xp = xr_lite.from_any(xp)
    is_array = isinstance(xp, DataArray)
    if not is_array and "image" not in xp.data_vars:
        raise ValueError("subtract_background: the Dataset has no 'image' variable")
    image = xp if is_array else xp["image"]  # (with the dataset's coordinates: the channel names)
    pages = next((p for p in (("im_y", "im_x"), ("y", "x")) if p[0] in image.dims and p[1] in image.dims), None)
    if pages is None:
        raise ValueError(f"subtract_background: no page dimensions (im_y, im_x) or (y, x) in {image.dims}")
    picked = None
    if channel is not None:
        if "channel" not in image.dims:
            raise ValueError(f"subtract_background: channel={channel!r}, but the image has no channel dimension")
        picked = sorted(set(channel_indexes(image, channel)))  # ChannelError (a ValueError) for an unknown name
    lead = tuple(d for d in image.dims if d not in pages and d != "channel")
    if "channel" in image.dims:
        lead = ("channel",) + lead
    data = image.transpose(*lead, *pages).data
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data)
    planes = to_device(data)
    if picked is None:
        out = subtract(planes, radius, smooth)
    else:
        out = planes.clone()
        for c in picked:
            out[c] = subtract(planes[c], radius, smooth)
    extra = {"background_radius": int(radius)}
    cleaned = DataArray(out, lead + pages, None, image.name, image.attrs).transpose(*image.dims)
    if is_array:
        return DataArray(cleaned.raw, image.dims, dict(xp.coords), xp.name, dict(xp.attrs, **extra))
    res = xp.copy()
    res.attrs.update(extra)
    res["image"] = cleaned
    res._cache.pop("image_minmax", None)  # (the stitch's min / max of the image as it was: the finders take their own)
    return res
