"""NumPy restatement of ``find_beads(track="ncc", stage_drift=D)`` ("find_beads: following a stage that
moved"), independent of magnify_amd/track.py and of the kernels; the per-bead correlation is tests/track_ref.py's.

D = stage_drift: the stage moved by up to D pixels per axis between time 0 and a timepoint, every bead with it.
  * b = 2 (D <= 32), 4 (D <= 64), 8; mc = ceil(D / b).
  * binned[t, i, j] = the sum of the b x b block at (b i, b j) of plane t, in float64, rounded to float32 once
    (``bin_planes``); trailing rows and columns are left out.
  * anchors on the (hb, wb) binned planes (``anchors``): I = min(hb, wb) - 2 mc, half_c = min(47, (I - 2) // 4) >= 4,
    side = 2 half_c + 1, rows mc + half_c + i side for i < (hb - 2 mc) // side, columns alike; raster order.
  * the anchors are tracked on the binned planes over [-mc, mc]^2 (track_ref.track); per timepoint the anchors with
    score >= min_score vote: lower median per axis, agree = the voters within 1 of it on both axes, trusted iff
    2 agree >= k; base[t] = b * median if trusted, else (0, 0); base[t_ref] = (0, 0), agree[t_ref] = 1 (``vote``).
  * based tracking (``track_based``): the patch of (bead, t) is cut to 0 <= y < h, md <= y + by < h - md (x alike),
    A(y, x) = plane[t][y + by + dy, x + bx + dx], fixed per (bead, t), shift = base + pick; row t_ref ignores its base;
    an empty patch gives shift (0, 0), score 0.
"""
import numpy as np

import track_ref as tr
from synth import draw_beads, random_bead_positions


def stage_bin(D):
    b = 2 if D <= 32 else 4 if D <= 64 else 8
    return b, (D + b - 1) // b


def bin_planes(planes, b):
    """(T, h // b, w // b) float32; integer pixels summed exactly, float pixels in float64."""
    n_t, h, w = planes.shape
    hb, wb = h // b, w // b
    acc = np.int64 if planes.dtype.kind == "u" else np.float64
    blocks = planes[:, :hb * b, :wb * b].astype(acc).reshape(n_t, hb, b, wb, b)
    return blocks.sum(axis=(2, 4)).astype(np.float32)


def anchors(hb, wb, mc):
    """(n, 3) [row, col, half_c]; ValueError where half_c < 4."""
    inner = min(hb, wb) - 2 * mc
    half_c = min(47, (inner - 2) // 4)
    if half_c < 4:
        raise ValueError(f"half_c = {half_c}")
    side = 2 * half_c + 1
    out = []
    for i in range((hb - 2 * mc) // side):
        for j in range((wb - 2 * mc) // side):
            out.append((mc + half_c + i * side, mc + half_c + j * side, half_c))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def vote(picks, scores, b, min_score, t_ref=0):
    """picks (A, T, 2), scores (A, T) -> (shift (T, 2) int64 in pixels, agree (T,) as a fraction of A, trusted (T,))."""
    n_a, n_t = scores.shape
    shift, agree, trusted = np.zeros((n_t, 2), dtype=np.int64), np.zeros(n_t), np.zeros(n_t, dtype=bool)
    for t in range(n_t):
        if t == t_ref:
            agree[t], trusted[t] = 1.0, True
            continue
        voters = [a for a in range(n_a) if scores[a, t] >= min_score]
        k = len(voters)
        if k == 0:
            continue
        my = sorted(int(picks[a, t, 0]) for a in voters)[(k - 1) // 2]
        mx = sorted(int(picks[a, t, 1]) for a in voters)[(k - 1) // 2]
        n_agree = sum(1 for a in voters if abs(int(picks[a, t, 0]) - my) <= 1 and abs(int(picks[a, t, 1]) - mx) <= 1)
        agree[t] = n_agree / n_a
        if 2 * n_agree >= k:
            shift[t], trusted[t] = (b * my, b * mx), True
    return shift, agree, trusted


def stage_drift(planes, D, min_score, t_ref=0):
    """{"shift" (T, 2), "agree" (T,), "anchors", "picks", "scores", "bin"} of the coarse pass and its vote."""
    b, mc = stage_bin(D)
    binned = bin_planes(planes, b)
    table = anchors(binned.shape[1], binned.shape[2], mc)
    res = tr.track(binned, table, int(table[0, 2]), mc, t_ref)
    shift, agree, _ = vote(res["shift"], res["score"], b, min_score, t_ref)
    return {"shift": shift, "agree": agree, "anchors": table, "picks": res["shift"], "scores": res["score"], "bin": b}


def patch_based(row, col, half, md, h, w, by, bx):
    """((y0, y1), (x0, x1)) half-open, in the template's plane."""
    y0, y1 = max(row - half, 0, md - by), min(row + half + 1, h, h - md - by)
    x0, x1 = max(col - half, 0, md - bx), min(col + half + 1, w, w - md - bx)
    return (y0, max(y1, y0)), (x0, max(x1, x0))


def track_based(planes, beads, half, md, base, t_ref=0):
    """{"sums" (M, T, W, W, 3), "fixed" (M, T, 3), "z", "shift" (totals), "score", "gap"}."""
    n_t, h, w = planes.shape
    beads = np.asarray(beads).reshape(-1, 3)
    acc = np.int64 if planes.dtype.kind == "u" else np.float64
    width = 2 * md + 1
    sums = np.zeros((len(beads), n_t, width, width, 3), dtype=acc)
    fixed = np.zeros((len(beads), n_t, 3), dtype=acc)
    empty = np.zeros((len(beads), n_t), dtype=bool)
    for g, (row, col, _) in enumerate(beads):
        for t in range(n_t):
            by, bx = (0, 0) if t == t_ref else (int(base[t][0]), int(base[t][1]))
            (y0, y1), (x0, x1) = patch_based(int(row), int(col), half, md, h, w, by, bx)
            if y1 == y0 or x1 == x0:
                empty[g, t] = True
                continue
            B = planes[t_ref, y0:y1, x0:x1].astype(acc)
            fixed[g, t] = [B.size, B.sum(), (B * B).sum()]
            A = planes[t].astype(acc)
            for dy in range(-md, md + 1):
                for dx in range(-md, md + 1):
                    Ad = A[y0 + by + dy:y1 + by + dy, x0 + bx + dx:x1 + bx + dx]
                    assert Ad.shape == B.shape
                    sums[g, t, dy + md, dx + md] = [Ad.sum(), (Ad * Ad).sum(), (Ad * B).sum()]
    z = np.stack([tr.scores(sums[:, t:t + 1], fixed[:, t])[:, 0] for t in range(n_t)], axis=1)
    pick, best, gap = tr.pick(z, t_ref)
    shift = pick + np.asarray(base, dtype=np.int64)[None]
    shift[:, t_ref] = 0
    shift[empty & (np.arange(n_t) != t_ref)[None]] = 0
    return {"sums": sums, "fixed": fixed, "z": z, "shift": shift, "score": best, "gap": gap, "empty": empty}


def follow(planes, beads, half, md, D, min_score=0.5, t_ref=0):
    """The whole feature on one channel: (stage_drift's result, track_based's result around its shift)."""
    stage = stage_drift(planes, D, min_score, t_ref)
    return stage, track_based(planes, beads, half, md, stage["shift"], t_ref)


def scene(seed, shape, n, r_lo, r_hi, jitter, drifts, D=None, channels=None, background=100, poisson=20.0, read_noise=3.0):
    """track_ref.scene with a drift per timepoint on top of the per-bead offsets: (planes (T, h, w) uint16 -- or
    (channels, T, h, w) --, beads (n', 3) [row, col, r] at time 0, offsets (n', T, 2) = drifts[t] + an integer in
    [-jitter, jitter]^2 per bead; time 0 unmoved).  Beads lie at least r_hi + jitter + D + 2 from the border
    (D: the largest drift component unless given), so every moved bead is whole."""
    rng = np.random.default_rng(seed)
    drifts = np.asarray(drifts, dtype=np.int64).reshape(-1, 2)
    n_t = len(drifts)
    D = int(np.abs(drifts).max()) if D is None else D
    pos = random_bead_positions(rng, shape, n, r_hi + jitter + 2, border=r_hi + jitter + D + 2)
    radii = rng.integers(r_lo, r_hi + 1, size=len(pos))
    offsets = rng.integers(-jitter, jitter + 1, size=(len(pos), n_t, 2)) + drifts[None]
    offsets[:, 0] = 0
    planes = np.empty((channels or 1, n_t) + tuple(shape), dtype=np.uint16)
    for c in range(channels or 1):
        values = rng.integers(500, 4001, size=len(pos))
        for t in range(n_t):
            img = background + rng.poisson(poisson, size=shape).astype(np.float64)
            disks = draw_beads(shape, pos + offsets[:, t], 2 * radii, values).astype(np.float64)
            img = np.where(disks > 0, disks + img, img)
            img = np.rint(img + rng.normal(0, read_noise, size=shape))
            planes[c, t] = np.clip(img, 0, 65535).astype(np.uint16)
    return (planes if channels else planes[0]), np.column_stack([pos, radii]), offsets


# the scenes of tests/test_cpu_drift.py and tests/test_gpu_drift.py: (shape, drifts, D of the border, stage_drift)
SCENES = [((384, 352), ((0, 0), (37, -22), (-40, 40), (5, 3)), 40, 40),
          ((288, 320), ((0, 0), (-19, 20), (11, -7)), 20, 20)]
N_BEADS, R_LO, R_HI, JITTER, MAX_DRIFT, HALF = 12, 5, 12, 2, 8, 14
