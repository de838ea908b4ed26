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
from . import despeckle, registry
from ._dataset import channel_indexes, page_view, plane_block
from .utils import int_in, to_list

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
    int_in("background radius", radius, 1, MAX_RADIUS)
    int_in("background smooth", smooth, SMOOTH[0], SMOOTH[-1])
    if channel is not None:
        names = to_list(channel)
        if not names or any(isinstance(c, (bool, np.bool_)) or not isinstance(c, (str, int, np.integer)) for c in names):
            raise ValueError(f"background channel must be a channel name or a list of names, got {channel!r}")


def _run(planes, radius, smooth, what):
    from . import hotpath

    check_background(radius, smooth)
    block, _, n, h, w, code, _ = plane_block(planes, f"background.{what}")
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
            hotpath._call("mg_despeckle_planes", part.data_ptr(), filtered, code, m, h, w, smooth, despeckle.ALL, 0.0, 0, 0,
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
    check_background(radius, smooth, channel)
    view = page_view(xp, "image", (("im_y", "im_x"), ("y", "x")), "subtract_background", first=("channel",))
    picked = None
    if channel is not None:
        if "channel" not in view.var.dims:
            raise ValueError(f"subtract_background: channel={channel!r}, but the image has no channel dimension")
        # (the source has the channel names; ChannelError, a ValueError, for an unknown one)
        picked = sorted(set(channel_indexes(view.source, channel)))
    if picked is None:
        out = subtract(view.planes, radius, smooth)
    else:
        out = view.planes.clone()
        for c in picked:
            out[c] = subtract(view.planes[c], radius, smooth)
    res = view.rebuild(out, {"background_radius": int(radius)})
    if not view.is_array:
        res._cache.pop("image_minmax", None)  # (the stitch's min / max of the image as it was: the finders take their own)
    return res
