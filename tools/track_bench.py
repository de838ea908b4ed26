"""Times bead tracking (``find_beads(track="ncc")``) on the MI355X with HIP events, inputs resident, every figure the
median of ``--calls`` timed calls after ``--warmup`` warm-up calls (one pair of events per call):

  * ``track_beads``: mg_track_beads alone, ``--beads`` beads x ``--time`` timepoints of one 4096 x 4096 uint16 channel,
    half = 27 (55 x 55 patches), max_drift = 8 (289 displacements); the planes are one random scene moved by a drawn
    offset per timepoint, so the shifts found are checked against what was drawn;
  * ``seam_sums``: mg_seam_sums with its reduce on the 8 x 8 grid of 1024 x 1024 tiles, overlap 102, max_shift 8 --
    the existing correlation kernel, as the yardstick;
  * ``roi_untracked`` / ``roi_tracked``: the ROI pass of the same stack with the time-0 table for every timepoint
    (what ``find_beads`` launches without ``track``) and with one table per timepoint (``find.tracked_roi_pass``: the
    pass over C T single-plane assays and the permuting copies of its outputs), roi_length ``--roi``.

Rates: ``pairs`` = (patch pixel, displacement) pairs, the unit of work both correlation kernels share; the seam kernel
spends three multiply-adds on a pair (sum A, sum A^2, sum A B in its inner loop), the tracking kernel one (sum A B; its
sums of A and A^2 are box sums).  Prints one JSON line.

    python tools/track_bench.py [--beads 2000] [--time 64] [--calls 20] [--warmup 5] [--roi 100]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import find, hotpath, register, track  # noqa: E402

SIDE, HALF, MAX_DRIFT = 4096, 27, 8
GRID, TILE, OVERLAP, MAX_SHIFT = 8, 1024, 102, 8


def timed(fn, calls, warmup):
    """(median, min, max) milliseconds of ``calls`` calls, each between two HIP events, after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beads", type=int, default=2000)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--roi", type=int, default=100)
    args = ap.parse_args()
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    n_t, m = args.time, args.beads
    # one random scene, moved as a whole by a drawn offset per timepoint (time 0 unmoved)
    scene = torch.from_numpy(rng.integers(0, 65536, size=(SIDE, SIDE), dtype=np.uint16)).cuda()
    moves = rng.integers(-MAX_DRIFT, MAX_DRIFT + 1, size=(n_t, 2))
    moves[0] = 0
    image = torch.empty((1, n_t, SIDE, SIDE), dtype=torch.uint16, device="cuda")
    for t in range(n_t):
        image[0, t].view(torch.int16).copy_(torch.roll(scene.view(torch.int16), (int(moves[t, 0]), int(moves[t, 1])), (0, 1)))
    margin = HALF + 2 * MAX_DRIFT + 2
    beads = np.column_stack([rng.integers(margin, SIDE - margin, size=(m, 2)), rng.integers(8, 26, size=m)]).astype(np.int32)
    d_beads = torch.from_numpy(beads).cuda()
    res = {"track": f"{m} beads x {n_t} timepoints, {SIDE}^2 u16, half {HALF}, max_drift {MAX_DRIFT}",
           "seams": f"{GRID}x{GRID} x {TILE}^2 u16, overlap {OVERLAP}, max_shift {MAX_SHIFT}", "calls": args.calls,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    found = track.track_beads(image[0], d_beads, HALF, MAX_DRIFT)
    shift, score = found["shift"].cpu().numpy(), found["score"].cpu().numpy()
    res["shifts_recovered"] = bool(np.array_equal(shift, np.broadcast_to(moves[None], shift.shape)))
    res["smallest_score"] = float(score.min())
    width = 2 * MAX_DRIFT + 1
    t_track = timed(lambda: track.track_beads(image[0], d_beads, HALF, MAX_DRIFT), args.calls, args.warmup)
    pairs = m * (n_t - 1) * width * width * (2 * HALF + 1) ** 2
    res["track_beads"] = dict(t_track, pairs=pairs, pairs_per_s=pairs / (t_track["ms"] * 1e-3),
                              multiply_adds_per_s=pairs / (t_track["ms"] * 1e-3))

    tiles = torch.from_numpy(rng.integers(0, 65536, size=(1, GRID, GRID, TILE, TILE), dtype=np.uint16)).cuda()
    t_seam = timed(lambda: register.seam_sums(tiles, OVERLAP, MAX_SHIFT), args.calls, args.warmup)
    n_seam = (TILE - 2 * MAX_SHIFT) * (OVERLAP - 2 * MAX_SHIFT)
    seam_pairs = 2 * GRID * (GRID - 1) * n_seam * (2 * MAX_SHIFT + 1) ** 2
    res["seam_sums"] = dict(t_seam, pairs=seam_pairs, pairs_per_s=seam_pairs / (t_seam["ms"] * 1e-3),
                            multiply_adds_per_s=3 * seam_pairs / (t_seam["ms"] * 1e-3))
    res["track_over_seam_pairs_per_s"] = res["track_beads"]["pairs_per_s"] / res["seam_sums"]["pairs_per_s"]
    del tiles

    tables, _ = track.tracked_tables(beads, shift, score, 0.5, SIDE, SIDE)
    L = args.roi
    res["roi"] = f"{m} markers x 1 channel x {n_t} timepoints, roi_length {L}"
    res["roi_untracked"] = timed(lambda: hotpath.roi_gather_reduce(image[None], [beads], L, None, disks=True), args.calls,
                                 args.warmup)
    res["roi_tracked"] = timed(lambda: find.tracked_roi_pass(image, tables, L), args.calls, args.warmup)
    res["roi_tracked_pass_only"] = timed(
        lambda: hotpath.roi_gather_reduce(image.view(n_t, 1, 1, SIDE, SIDE), [tables[t] for t in range(n_t)], L, None,
                                          disks=True), args.calls, args.warmup)
    res["roi_tracked_over_untracked"] = res["roi_tracked"]["ms"] / res["roi_untracked"]["ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
