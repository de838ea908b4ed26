"""Following beads through a time series for ``find_beads(track="ncc")`` (not in the reference, which cuts every
timepoint's ROI at the bead's time-0 position -- find.py:564: "TODO: Don't assume beads don't move across timesteps";
DESIGN.md, "find_beads: following beads through time").

Per bead and timepoint the integer displacement in [-max_drift, max_drift]^2 at which the patch around the bead
correlates best (zero-mean normalised cross-correlation) with the patch at the reference timepoint.  The sums, the
scores and the pick are made on the device (``track_beads``: mg_track_beads, with the score and the tie-breaks of
``register.seam_scores`` / ``register.pick_displacements``); the per-timepoint bead tables are NumPy on (M, T) rows.
"""
from __future__ import annotations

import numpy as np

TRACK_MODES = (None, "ncc")
MAX_DRIFT_LIMIT = 16   # (2 * 16 + 1)^2 displacements per (bead, timepoint)
MAX_PATCH_SIDE = 95    # 2 * half + 1
MAX_WINDOW_SIDE = 127  # 2 * half + 1 + 2 * max_drift: the window mg_track_beads stages


def check_track(track, max_drift=8, half=None):
    """``track`` as ``find_beads`` takes it: None or "ncc"; ``1 <= max_drift <= 16``; with ``half`` (the patch reaches
    ``half`` pixels from the centre) also ``1 <= half``, ``2 half + 1 <= 95`` and ``2 half + 1 + 2 max_drift <= 127``."""
    if track not in TRACK_MODES:
        raise ValueError(f"track must be one of {TRACK_MODES}, got {track!r}")
    if isinstance(max_drift, bool) or int(max_drift) != max_drift:
        raise ValueError(f"max_drift must be an integer, got {max_drift!r}")
    if max_drift < 1 or max_drift > MAX_DRIFT_LIMIT:
        raise ValueError(f"max_drift must be in [1, {MAX_DRIFT_LIMIT}], got {max_drift}")
    if half is not None:
        if isinstance(half, bool) or int(half) != half:
            raise ValueError(f"the patch half-width must be an integer, got {half!r}")
        if half < 1 or 2 * half + 1 > MAX_PATCH_SIDE:
            raise ValueError(f"the patch half-width must be in [1, {(MAX_PATCH_SIDE - 1) // 2}], got {half}")
        if 2 * half + 1 + 2 * max_drift > MAX_WINDOW_SIDE:
            raise ValueError(f"2 * half + 1 + 2 * max_drift must not exceed {MAX_WINDOW_SIDE}: half {half}, "
                             f"max_drift {max_drift}")
    return track


def track_beads(planes, beads, half: int, max_drift: int, t_ref: int = 0, want_sums: bool = False):
    """planes (T, H, W) on the device -- the timepoints of one channel, a view with any plane stride --, beads (M, 3)
    [row, col, r] (host or device) -> {"shift" (M, T, 2) int32 (dy, dx), "score" (M, T) float64} device tensors; row
    ``t_ref`` is (0, 0) with score 1.  ``want_sums``: also "sums" (M, T, 2 md + 1, 2 md + 1, 3) and "fixed" (M, 3), the
    correlation sums as ``register.seam_sums`` lays them out (int64 for integer pixels, float64 for float pixels)."""
    import torch

    from . import _native as nat
    from . import hotpath

    hotpath.require_gpu()
    if planes.dim() != 3:
        raise ValueError(f"track_beads takes (time, y, x) planes, got {tuple(planes.shape)}")
    check_track("ncc", max_drift, half)
    n_t, h, w = planes.shape
    if not 0 <= t_ref < n_t:
        raise ValueError(f"t_ref must be in [0, {n_t}), got {t_ref}")
    if planes.stride(2) != 1 or planes.stride(1) != w:
        planes = planes.contiguous()
    dev = planes.device
    if isinstance(beads, torch.Tensor):
        table = beads.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    else:
        table = torch.from_numpy(np.ascontiguousarray(np.asarray(beads).reshape(-1, 3), dtype=np.int32)).to(dev)
    m, width = table.shape[0], 2 * max_drift + 1
    code = nat.dtype_code(planes.dtype)
    out = {"shift": torch.zeros((m, n_t, 2), dtype=torch.int32, device=dev),
           "score": torch.zeros((m, n_t), dtype=torch.float64, device=dev)}
    if want_sums:
        acc = torch.int64 if code in (nat.MG_U8, nat.MG_U16) else torch.float64
        out["sums"] = torch.zeros((m, n_t, width, width, 3), dtype=acc, device=dev)
        out["fixed"] = torch.zeros((m, 3), dtype=acc, device=dev)
    hotpath._call("mg_track_beads", planes.data_ptr(), code, n_t, planes.stride(0) if n_t > 1 else h * w, h, w, int(t_ref),
                  table.data_ptr(), m, int(half), int(max_drift), out["shift"].data_ptr(), out["score"].data_ptr(),
                  hotpath._ptr(out.get("sums")), hotpath._ptr(out.get("fixed")), hotpath._stream())
    return out


def tracked_tables(beads, shift, score, min_score: float, h: int, w: int):
    """The bead table of every timepoint: beads (M, 3) [row, col, r], shift (M, T, 2), score (M, T) ->
    (tables (T, M, 3) int32 -- (row + dy, col + dx, r) with the centre clamped into the image --, followed (M, T) bool).
    Where ``score < min_score`` the bead keeps its reference position and counts as not followed."""
    beads = np.asarray(beads).reshape(-1, 3).astype(np.int64)
    shift = np.asarray(shift).astype(np.int64)
    followed = np.asarray(score, dtype=np.float64) >= min_score
    m, n_t = followed.shape
    move = np.where(followed[..., None], shift, 0)
    tables = np.empty((n_t, m, 3), dtype=np.int32)
    tables[..., 0] = np.clip(beads[None, :, 0] + move[..., 0].T, 0, h - 1)
    tables[..., 1] = np.clip(beads[None, :, 1] + move[..., 1].T, 0, w - 1)
    tables[..., 2] = beads[None, :, 2]
    return tables, followed
