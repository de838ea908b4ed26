"""Following beads through a time series for ``find_beads(track="ncc")`` (not in the reference, which cuts every
timepoint's ROI at the bead's time-0 position -- find.py:564: "TODO: Don't assume beads don't move across timesteps";
DESIGN.md, "find_beads: following beads through time").

Per bead and timepoint the integer displacement in [-max_drift, max_drift]^2 at which the patch around the bead
correlates best (zero-mean normalised cross-correlation) with the patch at the reference timepoint.  The sums, the
scores and the pick are made on the device (``track_beads``: mg_track_beads, with the score and the tie-breaks of
``register.seam_scores`` / ``register.pick_displacements``); the per-timepoint bead tables are NumPy on (M, T) rows.

``stage_drift=D``: the stage itself moved by up to D pixels between time 0 and a timepoint, every bead with it
("find_beads: following a stage that moved").  The planes are binned by b = 2 / 4 / 8 (``bin_planes``:
mg_bin_planes), a grid of large anchor patches is tracked on the binned planes with mg_track_beads itself
(``stage_anchors``), the anchors' picks go to a median vote per timepoint (``stage_vote``) and the beads are then
searched around the voted offset (``track_beads(base=...)``: mg_track_beads_based).
"""
from __future__ import annotations

import numpy as np

from .utils import int_in

TRACK_MODES = (None, "ncc")
MAX_DRIFT_LIMIT = 16   # (2 * 16 + 1)^2 displacements per (bead, timepoint)
MAX_PATCH_SIDE = 95    # 2 * half + 1
MAX_WINDOW_SIDE = 127  # 2 * half + 1 + 2 * max_drift: the window mg_track_beads stages
MAX_STAGE_DRIFT = 128  # 8 * 16: the largest bin times the largest coarse search
MAX_ANCHOR_HALF = 47   # the largest patch of mg_track_beads
MIN_ANCHOR_HALF = 4


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


def stage_bin(stage_drift: int):
    """(b, mc): the bin of the coarse pass and its search range in binned pixels, ``mc = ceil(D / b) <= 16``."""
    b = 2 if stage_drift <= 32 else 4 if stage_drift <= 64 else 8
    return b, -(-int(stage_drift) // b)


def stage_anchors(hb: int, wb: int, mc: int):
    """The anchor patches of the coarse pass on (hb, wb) binned planes searched over ``[-mc, mc]^2``: (n, 3) int32
    [row, col, half_c] in raster order -- a grid of disjoint, unclipped patches of side ``2 half_c + 1``, as large as
    mg_track_beads takes them (``half_c <= 47``) and as four of them side by side fit."""
    inner = min(hb, wb) - 2 * mc
    half_c = min(MAX_ANCHOR_HALF, (inner - 2) // 4)
    if half_c < MIN_ANCHOR_HALF:
        raise ValueError(f"the image is too small for the anchors of stage_drift: {hb} x {wb} binned pixels with a coarse "
                         f"search of {mc} leave patches of half-width {half_c}; every binned side must be at least "
                         f"{4 * MIN_ANCHOR_HALF + 2 + 2 * mc}")
    side = 2 * half_c + 1
    rows = [mc + half_c + i * side for i in range((hb - 2 * mc) // side)]
    cols = [mc + half_c + i * side for i in range((wb - 2 * mc) // side)]
    return np.array([[r, c, half_c] for r in rows for c in cols], dtype=np.int32).reshape(-1, 3)


def check_stage_drift(stage_drift, track, max_drift=8, shape=None):
    """``stage_drift`` as ``find_beads`` takes it: None, or an integer D in [1, 128] with ``track="ncc"`` and
    ``max_drift >= b`` (the coarse offset is only known to b / 2: the fine search has to cover that and leave room for
    the bead's own motion).  With ``shape`` = (h, w) of the image also that the anchors fit.  Returns None or (b, mc)."""
    if stage_drift is None:
        return None
    if track is None:
        raise ValueError('stage_drift needs track="ncc": the stage offset is where the per-bead search starts')
    b, mc = stage_bin(int_in("stage_drift", stage_drift, 1, MAX_STAGE_DRIFT))
    if max_drift < b:
        raise ValueError(f"stage_drift {stage_drift} is searched on planes binned by {b}: max_drift must be at least {b}, "
                         f"got {max_drift}")
    if shape is not None:
        h, w = shape
        need = b * (4 * MIN_ANCHOR_HALF + 2 + 2 * mc)
        if min(h, w) < need:
            raise ValueError(f"the image ({h} x {w}) is too small for stage_drift {stage_drift}: every side must be at "
                             f"least {need}")
        stage_anchors(h // b, w // b, mc)
    return b, mc


def _row_contiguous(planes):
    n_t, h, w = planes.shape
    if planes.stride(2) != 1 or planes.stride(1) != w:
        planes = planes.contiguous()
    return planes, (planes.stride(0) if n_t > 1 else h * w)


def bin_planes(planes, b: int):
    """planes (T, H, W) on the device -- a view with any plane stride -- -> (T, H // b, W // b) float32: the sums of the
    b x b blocks (mg_bin_planes; exact for integer pixels); the trailing H % b rows and W % b columns are left out."""
    import torch

    from . import _native as nat
    from . import hotpath

    hotpath.require_gpu()
    if planes.dim() != 3:
        raise ValueError(f"bin_planes takes (time, y, x) planes, got {tuple(planes.shape)}")
    n_t, h, w = planes.shape
    if b not in (2, 4, 8) or h < b or w < b or n_t < 1:
        raise ValueError(f"bin_planes: bin must be 2, 4 or 8 and the planes at least one bin wide, got bin {b} on "
                         f"{tuple(planes.shape)}")
    planes, stride = _row_contiguous(planes)
    out = torch.empty((n_t, h // b, w // b), dtype=torch.float32, device=planes.device)
    hotpath._call("mg_bin_planes", planes.data_ptr(), nat.dtype_code(planes.dtype), n_t, stride, h, w, int(b),
                  out.data_ptr(), hotpath._stream())
    return out


def stage_vote(picks, scores, b: int, min_score: float, t_ref: int = 0):
    """The anchors' vote: picks (A, T, 2) in binned pixels, scores (A, T) -> (shift (T, 2) int32 in pixels, agree (T,)
    float64).  Per timepoint the voters are the anchors with ``score >= min_score``; the offset is their lower median
    per axis; ``agree`` counts the voters within one bin of it on both axes (a drift of 1.5 bins is picked as 1 by some
    anchors and as 2 by others) and the offset is trusted iff at least half the voters agree -- otherwise, and without
    voters, the base is (0, 0): the plain search.  ``agree`` is returned as a fraction of all anchors; row ``t_ref`` is
    (0, 0) and 1."""
    picks = np.asarray(picks).astype(np.int64)
    ok = np.asarray(scores, dtype=np.float64) >= min_score
    n_a, n_t = ok.shape
    shift = np.zeros((n_t, 2), dtype=np.int32)
    agree = np.zeros(n_t, dtype=np.float64)
    for t in range(n_t):
        if t == t_ref:
            agree[t] = 1.0
            continue
        votes = picks[ok[:, t], t]
        k = len(votes)
        if k == 0:
            continue
        med = np.sort(votes, axis=0)[(k - 1) // 2]
        n_agree = int((np.abs(votes - med) <= 1).all(axis=1).sum())
        agree[t] = n_agree / n_a
        if 2 * n_agree >= k:
            shift[t] = b * med
    return shift, agree


def stage_drift(planes, drift: int, min_score: float, t_ref: int = 0):
    """The offset every bead of a timepoint shares: planes (T, H, W) on the device, D = ``drift`` ->
    {"shift" (T, 2) int32 (pixels, a multiple of b), "agree" (T,) float64, "anchors" (A, 3), "picks" (A, T, 2),
    "scores" (A, T), "bin"}: the planes binned by b, the anchors tracked over ``[-mc, mc]^2`` by mg_track_beads, the
    vote of ``stage_vote``."""
    n_t, h, w = planes.shape
    b, mc = check_stage_drift(drift, "ncc", MAX_DRIFT_LIMIT, (h, w))
    anchors = stage_anchors(h // b, w // b, mc)
    res = track_beads(bin_planes(planes, b), anchors, int(anchors[0, 2]), mc, t_ref)
    picks, scores = res["shift"].cpu().numpy(), res["score"].cpu().numpy()
    shift, agree = stage_vote(picks, scores, b, min_score, t_ref)
    return {"shift": shift, "agree": agree, "anchors": anchors, "picks": picks, "scores": scores, "bin": b}


def track_beads(planes, beads, half: int, max_drift: int, t_ref: int = 0, want_sums: bool = False, base=None):
    """planes (T, H, W) on the device -- the timepoints of one channel, a view with any plane stride --, beads (M, 3)
    [row, col, r] (host or device) -> {"shift" (M, T, 2) int32 (dy, dx), "score" (M, T) float64} device tensors; row
    ``t_ref`` is (0, 0) with score 1.  ``want_sums``: also "sums" (M, T, 2 md + 1, 2 md + 1, 3) and "fixed" (M, 3), the
    correlation sums as ``register.seam_sums`` lays them out (int64 for integer pixels, float64 for float pixels).
    ``base`` (T, 2) [by, bx] (host or device): the search of timepoint t is centred on its base (mg_track_beads_based);
    "shift" is then the total displacement and "fixed" (M, T, 3), the patch being cut per timepoint."""
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
    planes, stride = _row_contiguous(planes)
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
        out["fixed"] = torch.zeros((m, 3) if base is None else (m, n_t, 3), dtype=acc, device=dev)
    tail = (out["shift"].data_ptr(), out["score"].data_ptr(), hotpath._ptr(out.get("sums")), hotpath._ptr(out.get("fixed")),
            hotpath._stream())
    head = (planes.data_ptr(), code, n_t, stride, h, w, int(t_ref), table.data_ptr(), m, int(half), int(max_drift))
    if base is None:
        hotpath._call("mg_track_beads", *head, *tail)
        return out
    if isinstance(base, torch.Tensor):
        d_base = base.to(device=dev, dtype=torch.int32).contiguous()
    else:
        d_base = torch.from_numpy(np.ascontiguousarray(np.asarray(base), dtype=np.int32)).to(dev)
    if tuple(d_base.shape) != (n_t, 2):
        raise ValueError(f"base must be (time, 2) = {(n_t, 2)}, got {tuple(d_base.shape)}")
    hotpath._call("mg_track_beads_based", *head, d_base.data_ptr(), *tail)
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
