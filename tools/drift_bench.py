"""Times ``find_beads(track="ncc", stage_drift=D)`` on the MI355X with HIP events, inputs resident, every figure the
median of ``--calls`` timed calls after ``--warmup`` warm-up calls (one pair of events per call), as
tools/track_bench.py does.  The stack: ``--beads`` beads x ``--time`` timepoints of one 4096 x 4096 uint16 channel,
half = 27, max_drift = 8; the planes are one scene -- 32-pixel blocks plus white noise: structure that survives binning,
and a sharp correlation peak at full resolution -- moved as a whole by a drawn stage offset within ``[-D, D]^2`` per
timepoint, so the offsets found are checked against what was drawn.  Per ``--drift`` D (default 100: b = 8, and 60:
b = 4):

  * ``plane_minmax``: mg_plane_minmax on the same planes -- the yardstick, it reads the same bytes once;
  * ``bin_planes``: mg_bin_planes, with its bytes (read + written) per second and its time over the yardstick's;
  * ``coarse``: mg_track_beads on the binned planes with the anchors as beads;
  * ``stage_drift``: binning, coarse pass, the copy of the picks to the host and the vote (``track.stage_drift``);
  * ``fine_based``: mg_track_beads_based around the voted offsets; ``fine_plain``: mg_track_beads on the same shape;
  * ``stack``: ``stage_drift`` + ``fine_based``.

Prints one JSON line.

    python tools/drift_bench.py [--beads 2000] [--time 64] [--calls 20] [--warmup 5] [--drift 100 60]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import hotpath, track  # noqa: E402

SIDE, HALF, MAX_DRIFT, BLOCK = 4096, 27, 8, 32


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
    ap.add_argument("--drift", type=int, nargs="+", default=[100, 60])
    args = ap.parse_args()
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    n_t, m = args.time, args.beads
    blocks = rng.integers(0, 40001, size=(SIDE // BLOCK, SIDE // BLOCK))
    scene = np.kron(blocks, np.ones((BLOCK, BLOCK), dtype=np.int64)) + rng.integers(0, 20001, size=(SIDE, SIDE))
    scene = torch.from_numpy(scene.astype(np.uint16)).cuda()
    image = torch.empty((n_t, SIDE, SIDE), dtype=torch.uint16, device="cuda")
    res = {"stack": f"{m} beads x {n_t} timepoints, {SIDE}^2 u16, half {HALF}, max_drift {MAX_DRIFT}", "calls": args.calls,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "drifts": {}}
    plane_bytes = n_t * SIDE * SIDE * 2
    for D in args.drift:
        b, mc = track.check_stage_drift(D, "ncc", MAX_DRIFT, (SIDE, SIDE))
        moves = rng.integers(-D, D + 1, size=(n_t, 2))
        moves[0] = 0
        for t in range(n_t):
            image[t].view(torch.int16).copy_(torch.roll(scene.view(torch.int16), (int(moves[t, 0]), int(moves[t, 1])), (0, 1)))
        margin = HALF + 2 * MAX_DRIFT + D + 2
        beads = np.column_stack([rng.integers(margin, SIDE - margin, size=(m, 2)), rng.integers(8, 26, size=m)]).astype(np.int32)
        d_beads = torch.from_numpy(beads).cuda()
        out = {"bin": b, "coarse_max_drift": mc}
        stage = track.stage_drift(image, D, 0.5)
        anchors = stage["anchors"]
        out["anchors"], out["anchor_half"] = int(len(anchors)), int(anchors[0, 2])
        out["stage_error_max"] = int(np.abs(stage["shift"] - moves).max())
        out["stage_agree_min"] = float(stage["agree"].min())
        d_base = torch.from_numpy(stage["shift"]).cuda()
        found = track.track_beads(image, d_beads, HALF, MAX_DRIFT, base=d_base)
        shift, score = found["shift"].cpu().numpy(), found["score"].cpu().numpy()
        out["shifts_recovered"] = bool(np.array_equal(shift, np.broadcast_to(moves[None], shift.shape)))
        out["smallest_score"] = float(score.min())

        t_mm = timed(lambda: hotpath.plane_minmax(image), args.calls, args.warmup)
        out["plane_minmax"] = dict(t_mm, bytes=plane_bytes, GB_per_s=plane_bytes / (t_mm["ms"] * 1e-3) / 1e9)
        t_bin = timed(lambda: track.bin_planes(image, b), args.calls, args.warmup)
        bin_bytes = plane_bytes + n_t * (SIDE // b) ** 2 * 4
        out["bin_planes"] = dict(t_bin, bytes=bin_bytes, GB_per_s=bin_bytes / (t_bin["ms"] * 1e-3) / 1e9,
                                 over_plane_minmax=t_bin["ms"] / t_mm["ms"])
        binned = track.bin_planes(image, b)
        d_anchors = torch.from_numpy(anchors).cuda()
        half_c = int(anchors[0, 2])
        out["coarse"] = timed(lambda: track.track_beads(binned, d_anchors, half_c, mc), args.calls, args.warmup)
        del binned
        out["stage_drift"] = timed(lambda: track.stage_drift(image, D, 0.5), args.calls, args.warmup)
        out["fine_based"] = timed(lambda: track.track_beads(image, d_beads, HALF, MAX_DRIFT, base=d_base), args.calls,
                                  args.warmup)
        out["fine_plain"] = timed(lambda: track.track_beads(image, d_beads, HALF, MAX_DRIFT), args.calls, args.warmup)
        out["fine_based_over_plain"] = out["fine_based"]["ms"] / out["fine_plain"]["ms"]

        def stack():
            s = track.stage_drift(image, D, 0.5)
            return track.track_beads(image, d_beads, HALF, MAX_DRIFT, base=s["shift"])

        out["stack"] = timed(stack, args.calls, args.warmup)
        res["drifts"][str(D)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
