"""Skew: the tilt of a chip's grid in the stitched image, estimated on the device (not in the reference, whose ``rotate``
is a stub that takes the angle from the user).

A grid projected along its own axes gives the sharpest profiles.  ``profiles`` is the kernel (``mg_skew.hip``): the sums
and counts of the pixels of one plane along every angle of a table, over the inscribed disk, in integers.  ``score``
turns them into one number per angle on the host: the sum of the squared steps of the mean profile.
``estimate_rotation`` runs a coarse table on the binned plane, a fine one on the plane itself, and returns the
``rotation`` that puts the grid straight with a confidence; ``rotate(rotation="auto")`` and the pipelines' ``rotation=
"auto"`` use it.  ``tests/skew_ref.py`` restates all of it in NumPy.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as nat
from ._dataset import channel_index

MAX_ANGLES = nat.DEFINES["MG_SKEW_MAX_ANGLES"]
MAX_SIDE = nat.DEFINES["MG_SKEW_MAX_SIDE"]
MIN_SIDE = 8
FINE_HALF = 25  # the fine pass: 2 * FINE_HALF + 1 angles, FINE_HALF to a coarse step


def check_rotation(rotation, feature=16, max_angle=10.0, min_confidence=2.0):
    """The settings of ``rotate`` as the pipelines take them: ``rotation`` a finite number of degrees or "auto", and for
    "auto" ``feature >= 4`` pixels, ``0 < max_angle < 45`` degrees and a ``min_confidence`` that is not negative.
    ValueError otherwise.  True for "auto"."""
    if isinstance(rotation, str):
        if rotation != "auto":
            raise ValueError(f"rotation must be a number of degrees or 'auto', got {rotation!r}")
        for name, value in (("rotation_feature", feature), ("rotation_max", max_angle),
                            ("rotation_min_confidence", min_confidence)):
            if isinstance(value, (bool, np.bool_, str)) or not isinstance(value, (int, float, np.integer, np.floating)):
                raise ValueError(f"{name} must be a number, got {value!r}")
        if not (math.isfinite(feature) and feature >= 4):
            raise ValueError(f"rotation_feature must be at least 4 pixels, got {feature!r}")
        if not 0 < max_angle < 45:
            raise ValueError(f"rotation_max must be above 0 and below 45 degrees, got {max_angle!r}")
        if not min_confidence >= 0:
            raise ValueError(f"rotation_min_confidence must not be negative, got {min_confidence!r}")
        return True
    if not math.isfinite(float(rotation)):
        raise ValueError(f"rotation must be a finite number of degrees, got {rotation!r}")
    return False


def angle_table(angles_deg):
    """(n, 2) int32 (rint(32768 cos), rint(32768 sin)) of the angles, in degrees."""
    a = np.radians(np.asarray(angles_deg, dtype=np.float64).reshape(-1))
    return np.stack([np.rint(32768.0 * np.cos(a)), np.rint(32768.0 * np.sin(a))], axis=1).astype(np.int32)


def _float_range(plane):
    from . import hotpath

    lo, hi = hotpath.plane_minmax(plane[None])[0].tolist()
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"skew.profiles: the plane's min / max is not finite ({lo}, {hi})")
    return lo, (65535.0 / (hi - lo) if hi > lo else 0.0)


def profiles(plane, angles_deg, lo=None, scale=None):
    """plane (H, W) on the device, a view with any row stride -> (sums uint64, counts uint32), NumPy arrays
    (n_angles, 2, min(H, W) + 2): mg_skew_profiles, MAX_ANGLES angles to a launch.  A float plane is quantised as
    ``floor((p - lo) * scale)`` clamped to 0 .. 65535; ``lo`` and ``scale`` default to its minimum and
    65535 / (max - min) (0 for a flat plane; ValueError where the minimum or the maximum is not finite)."""
    from . import hotpath

    if not isinstance(plane, torch.Tensor) or plane.dim() != 2:
        raise ValueError("skew.profiles takes one (H, W) device tensor")
    if plane.stride(1) != 1:
        plane = plane.contiguous()
    hotpath.require_gpu()
    if not plane.is_cuda:
        raise ValueError("skew.profiles takes a device tensor; move it with preprocess.to_device")
    h, w, code = int(plane.shape[0]), int(plane.shape[1]), nat.dtype_code(plane.dtype)
    if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
        raise ValueError(f"skew.profiles: planes of {MIN_SIDE} .. {MAX_SIDE} pixels a side, got {h} x {w}")
    table = angle_table(angles_deg)
    if not len(table):
        raise ValueError("skew.profiles: no angles")
    if plane.dtype.is_floating_point and (lo is None or scale is None):
        lo, scale = _float_range(plane)
    lo, scale = (0.0, 0.0) if lo is None or scale is None else (float(lo), float(scale))
    nb = min(h, w) + 2
    d_table = torch.from_numpy(table).to(plane.device)
    # (uint64 / uint32 as the int64 / int32 of the same bits: exact, a bin stays below 2^53 and a count below 2^31)
    sums = torch.zeros((len(table), 2, nb), dtype=torch.int64, device=plane.device)
    counts = torch.zeros((len(table), 2, nb), dtype=torch.int32, device=plane.device)
    for a in range(0, len(table), MAX_ANGLES):
        n = min(MAX_ANGLES, len(table) - a)
        hotpath._call("mg_skew_profiles", plane.data_ptr(), code, h, w, plane.stride(0), lo, scale, d_table[a:].data_ptr(),
                      n, sums[a:].data_ptr(), counts[a:].data_ptr(), hotpath._stream())
    return sums.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def score(sums, counts):
    """(n_angles,) float64: over the bins with ``|2 (k - nb // 2) + 1| <= floor(0.8 D)`` -- the middle of the disk, where
    every projection line is long -- the sum over both axes of ``diff(sums / counts) ** 2``.  The division is what makes
    it work on a lit background: the floor in the bin index lets the counts of neighbouring bins differ (a moire that
    moves with the angle), and the sums carry that pattern times the background level."""
    nb = sums.shape[-1]
    k = np.arange(nb)
    keep = np.abs(2 * (k - nb // 2) + 1) <= math.floor(0.8 * (nb - 2))
    m = sums[..., keep].astype(np.float64) / counts[..., keep].astype(np.float64)
    return (np.diff(m, axis=-1) ** 2).sum(axis=(-2, -1))


def coarse_bin(feature):
    """The bin of the coarse pass: the largest of 8, 4, 2 that leaves the feature 8 binned pixels wide, else 1."""
    return next((b for b in (8, 4, 2) if feature / b >= 8), 1)


def coarse_angles(feature, b, d_b, max_angle):
    """(step, angles) in degrees: the step moves the rim of a disk of ``d_b`` binned pixels by half a binned feature."""
    step = math.degrees((feature / b) / (2 * d_b))
    n = math.ceil(max_angle / step)
    return step, np.arange(-n, n + 1, dtype=np.float64) * step


def _vertex(scores, angles):
    j = int(np.argmax(scores))
    best = float(angles[j])
    if 0 < j < len(scores) - 1:
        left, mid, right = float(scores[j - 1]), float(scores[j]), float(scores[j + 1])
        curve = left - 2.0 * mid + right
        if curve < 0:
            best += 0.5 * (left - right) / curve * float(angles[j + 1] - angles[j])
    return best


def _plane_of(image_or_xp, channel, time):
    """The (H, W) device plane to estimate on: a 2-D array itself, else plane (channel, time) of a (channel, time, y, x)
    array or of the ``image`` of a Dataset."""
    from .preprocess import to_device
    from .xr_lite import DataArray, Dataset

    if isinstance(image_or_xp, (Dataset, DataArray)):
        from . import find

        xp = image_or_xp
        if isinstance(xp, DataArray):
            raise ValueError("skew.estimate_rotation takes a Dataset with an image, a device tensor or an array")
        if "image" not in xp:
            raise AttributeError("Dataset must contain 'image' data variable.")
        image = find._image_tensor(xp)
        c = channel_index(xp, channel, default=0)
    else:
        image = image_or_xp if isinstance(image_or_xp, torch.Tensor) and image_or_xp.is_cuda else to_device(image_or_xp)
        if image.dim() == 2:
            return image
        if image.dim() != 4:
            raise ValueError(f"skew.estimate_rotation takes a (y, x) plane or a (channel, time, y, x) image, got "
                             f"{tuple(image.shape)}")
        c = 0 if channel is None else int(channel)
    if not (0 <= c < image.shape[0] and -image.shape[1] <= int(time) < image.shape[1]):
        raise ValueError(f"skew.estimate_rotation: no plane (channel {channel!r}, time {time!r}) in {tuple(image.shape)}")
    return image[c, int(time)]


def estimate_rotation(image_or_xp, feature, channel=None, time=0, max_angle=10.0, min_confidence=2.0):
    """(rotation, confidence): the ``rotation`` in degrees, within ``max_angle`` (and a coarse step) of 0, that puts the
    grid of the plane straight -- minus its tilt -- and how far the best coarse score stands above the median one.
    ``feature``: the width in pixels of what the grid is made of (a button's diameter); it sets the coarse binning and
    the angle steps.  Below ``min_confidence`` nothing periodic was seen: the fine pass is left out and the rotation is
    0.0."""
    from . import track

    check_rotation("auto", feature, max_angle, min_confidence)
    plane = _plane_of(image_or_xp, channel, time)
    b = coarse_bin(feature)
    coarse = track.bin_planes(plane[None], b)[0] if b > 1 else plane
    step, angles = coarse_angles(feature, b, min(coarse.shape), max_angle)
    s = score(*profiles(coarse, angles))
    j = int(np.argmax(s))
    median = float(np.median(s))
    confidence = float(s[j]) / median if median > 0 else 0.0
    if confidence < min_confidence:
        return 0.0, confidence
    fine = float(angles[j]) + np.arange(-FINE_HALF, FINE_HALF + 1, dtype=np.float64) * (step / FINE_HALF)
    return _vertex(score(*profiles(plane, fine)), fine), confidence
