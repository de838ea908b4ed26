"""Tile registration for ``stitch(register="ncc")`` (not in the reference; DESIGN.md, "stitch: registration by seam
cross-correlation"): the displacement of every pair of neighbouring tiles from the zero-mean normalised
cross-correlation of their overlap strips, and one integer shift per tile that explains those displacements.

The sums behind the correlation are made on the device (``seam_sums``: mg_seam_sums); the score, the pick and the
solve are NumPy on tables of a few hundred rows.

Notation: tiles (ty, tx) on an R x Cc grid, overlap v, ``m = max_shift``.  ``e[r, c] = (ey, ex)`` is the position error
of tile (r, c): its pixel q shows the scene point ``nominal origin + e + q``.  A seam (A | B) measures
``delta = e_B - e_A``.
"""
from __future__ import annotations

import numpy as np

REGISTER_MODES = (None, "ncc")
MAX_SHIFT_LIMIT = 32  # mg_seam_sums stages a tile and its halo of max_shift in LDS


def check_register(register, max_shift=8, overlap=None):
    """``register`` as ``stitch`` takes it: None or "ncc"; ``1 <= max_shift <= overlap // 4`` (the patch then keeps
    at least half the overlap) and at most ``MAX_SHIFT_LIMIT``."""
    if register not in REGISTER_MODES:
        raise ValueError(f"register must be one of {REGISTER_MODES}, got {register!r}")
    if isinstance(max_shift, bool) or int(max_shift) != max_shift:
        raise ValueError(f"max_shift must be an integer, got {max_shift!r}")
    if max_shift < 1 or (overlap is not None and max_shift > overlap // 4) or max_shift > MAX_SHIFT_LIMIT:
        raise ValueError(f"max_shift must be in [1, min(overlap // 4, {MAX_SHIFT_LIMIT})]: max_shift {max_shift}, "
                         f"overlap {overlap}")
    return register


def seam_list(R: int, Cc: int) -> np.ndarray:
    """(n_seams, 4) int: (row of A, column of A, row of B, column of B) -- the horizontal seams (r, c) | (r, c + 1) at
    index r (Cc - 1) + c, then the vertical ones (r, c) | (r + 1, c) at R (Cc - 1) + r Cc + c."""
    seams = [(r, c, r, c + 1) for r in range(R) for c in range(Cc - 1)]
    seams += [(r, c, r + 1, c) for r in range(R - 1) for c in range(Cc)]
    return np.asarray(seams, dtype=np.int64).reshape(-1, 4)


def seam_sums(planes, overlap: int, max_shift: int):
    """planes (P, R, Cc, ty, tx) on the device -> (sums (P, n_seams, 2m + 1, 2m + 1, 3), fixed (P, n_seams, 3)) device
    tensors: per displacement [sum A, sum A^2, sum A B], per seam [n, sum B, sum B^2]; int64 (exact) for integer
    pixels, float64 for float pixels, the same bits on every call."""
    import torch

    from . import _native as nat
    from . import hotpath

    hotpath.require_gpu()
    if planes.dim() != 5:
        raise ValueError(f"seam_sums takes (plane, tile_row, tile_col, tile_y, tile_x) tiles, got {tuple(planes.shape)}")
    p, nr, nc, ty, tx = planes.shape
    check_register("ncc", max_shift, overlap)
    if overlap > min(ty, tx):
        raise ValueError(f"Overlap ({overlap}) must not exceed the tile size ({ty}x{tx}).")
    planes = planes.contiguous()
    code = nat.dtype_code(planes.dtype)
    out_dtype = torch.int64 if code in (nat.MG_U8, nat.MG_U16) else torch.float64
    n_seams, w = nr * (nc - 1) + (nr - 1) * nc, 2 * max_shift + 1
    sums = torch.zeros((p, n_seams, w, w, 3), dtype=out_dtype, device=planes.device)
    fixed = torch.zeros((p, n_seams, 3), dtype=out_dtype, device=planes.device)
    if p == 0 or n_seams == 0:
        return sums, fixed
    nbytes = int(nat.lib().mg_seam_sums_scratch_bytes(p, nr, nc, ty, tx, overlap, max_shift))
    if nbytes < 0:
        raise ValueError("mg_seam_sums: invalid argument (MG_EINVAL)")
    scratch = torch.empty((max(nbytes // 8, 1),), dtype=torch.int64, device=planes.device)
    hotpath._call("mg_seam_sums", planes.data_ptr(), code, p, nr, nc, ty, tx, overlap, max_shift, sums.data_ptr(),
                  fixed.data_ptr(), scratch.data_ptr(), nbytes, hotpath._stream())
    return sums, fixed


def seam_scores(sums, fixed) -> np.ndarray:
    """z (..., 2m + 1, 2m + 1) float64 from sums (..., 2m + 1, 2m + 1, 3) and fixed (..., 3):
    z = (n sum AB - sum A sum B) / sqrt((n sum A^2 - (sum A)^2) (n sum B^2 - (sum B)^2)); 0 where a variance term
    is <= 0 or z is not finite (flat patches, NaN pixels)."""
    sums = np.asarray(sums).astype(np.float64)
    fixed = np.asarray(fixed).astype(np.float64)
    n, sb, sbb = (fixed[..., None, None, i] for i in range(3))
    sa, saa, sab = (sums[..., i] for i in range(3))
    with np.errstate(all="ignore"):
        va = n * saa - sa * sa
        vb = n * sbb - sb * sb
        z = (n * sab - sa * sb) / np.sqrt(va * vb)
        ok = (va > 0) & (vb > 0) & np.isfinite(z)
    return np.where(ok, z, 0.0)


def pick_displacements(scores):
    """scores (..., 2m + 1, 2m + 1) -> (delta (..., 2) int64, best score (...)): the displacement of the largest score;
    ties go to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx."""
    scores = np.asarray(scores, dtype=np.float64)
    w = scores.shape[-1]
    m = (w - 1) // 2
    dy, dx = (a.reshape(-1) for a in np.mgrid[-m:m + 1, -m:m + 1])
    order = np.lexsort((dx, dy, dy * dy + dx * dx))  # candidates in tie-break order: argmax keeps the first maximum
    flat = scores.reshape(scores.shape[:-2] + (w * w,))[..., order]
    first = np.argmax(flat, axis=-1)
    delta = np.stack([dy[order][first], dx[order][first]], axis=-1).astype(np.int64)
    return delta, np.take_along_axis(flat, first[..., None], axis=-1)[..., 0]


def _components(n, edges):
    """Label of every node: the smallest node index of its connected component."""
    label = np.arange(n)
    for _ in range(n):
        before = label.copy()
        for a, b in edges:
            label[a] = label[b] = min(label[a], label[b])
        if np.array_equal(before, label):
            break
    return label


def solve_shifts(R: int, Cc: int, best, min_score: float, clip: int):
    """One integer shift per tile from the seams' displacements.  ``best = (delta (n_seams, 2), score (n_seams,))`` in
    ``seam_list`` order.  Returns (shift (R, Cc, 2) int32, used (n_seams,) bool, number of clipped entries).

    A seam is used iff its score >= ``min_score``.  Per axis: the minimum-norm least-squares solution of
    ``e_B - e_A = delta`` over the used seams; per connected component of the used-seam graph the value at its first
    tile in raster order is subtracted and the rest rounded (np.rint), then g = (min + max) // 2 of the component is
    subtracted, so that the shifts are centred; a tile without a used seam keeps 0.  At last the table is clipped into
    [-clip, clip]."""
    delta, score = np.asarray(best[0], dtype=np.float64), np.asarray(best[1], dtype=np.float64)
    seams = seam_list(R, Cc)
    n = R * Cc
    used = score >= min_score if len(seams) else np.zeros(0, dtype=bool)
    ia, ib = seams[:, 0] * Cc + seams[:, 1], seams[:, 2] * Cc + seams[:, 3]
    shift = np.zeros((n, 2), dtype=np.int64)
    if used.any():
        rows = np.flatnonzero(used)
        a = np.zeros((len(rows), n), dtype=np.float64)
        a[np.arange(len(rows)), ib[rows]] = 1.0
        a[np.arange(len(rows)), ia[rows]] = -1.0
        label = _components(n, list(zip(ia[rows], ib[rows])))
        for axis in range(2):
            e = np.linalg.lstsq(a, delta[rows, axis], rcond=None)[0]
            e = np.rint(e - e[label]).astype(np.int64)  # (label: the component's first tile in raster order)
            for first in np.unique(label):
                mine = label == first
                e[mine] -= (e[mine].min() + e[mine].max()) // 2
            shift[:, axis] = e
    clipped = np.clip(shift, -clip, clip)
    n_clipped = int((clipped != shift).sum())
    return clipped.reshape(R, Cc, 2).astype(np.int32), used, n_clipped


def register_tiles(planes, overlap: int, max_shift: int = 8, min_score: float = 0.5):
    """planes (P, R, Cc, ty, tx) on the device, as the stitch would write the tiles -> one shift table per plane:
    {"tile_shift" (P, R, Cc, 2) int32, "seam_shift" (P, n_seams, 2) int32, "seam_score" (P, n_seams) float64,
    "seam_used" (P, n_seams) bool, "clipped": entries that had to be clipped into [-overlap // 2, overlap // 2]}.

    ``max_shift`` bounds the RELATIVE displacement of two neighbouring tiles (the search window of a seam), not a
    tile's absolute position error: a drift that grows by less than ``max_shift`` from tile to tile is followed across
    the grid, up to the ``overlap // 2`` a tile can be moved by."""
    p, nr, nc = planes.shape[:3]
    sums, fixed = seam_sums(planes, overlap, max_shift)
    delta, score = pick_displacements(seam_scores(sums.cpu().numpy(), fixed.cpu().numpy()))
    shifts = np.zeros((p, nr, nc, 2), dtype=np.int32)
    used = np.zeros(score.shape, dtype=bool)
    clipped = 0
    for i in range(p):
        shifts[i], used[i], n = solve_shifts(nr, nc, (delta[i], score[i]), min_score, overlap // 2)
        clipped += n
    return {"tile_shift": shifts, "seam_shift": delta.astype(np.int32), "seam_score": score, "seam_used": used,
            "clipped": clipped}
