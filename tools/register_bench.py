"""Times tile registration (``stitch(register="ncc")``) on the MI355X with HIP events: an 8 x 8 grid of 1024 x 1024
uint16 tiles, overlap 102 (a 7376 x 7376 chip), ``--planes`` planes, ``max_shift`` 8.  Reported, each the median of
``--windows`` windows of back-to-back calls after warm-up (the functions alternate window by window, so that drift of
the machine falls on all of them):

  * ``seam_sums``: mg_seam_sums with its reduce, on one registration plane;
  * ``solve``: score, pick and solve on the host (wall clock);
  * ``plain`` / ``linear``: the existing stitch passes of the same tiles, from this same build;
  * ``shift`` / ``shift+linear``: the registered stitch with the table already on the device -- the entry point's
    time, its read-back of the table and its wait for the stream included -- with its ratio to the pass it replaces;
  * ``shift (host table)``: the same call handed the NumPy table, as ``Stitcher`` makes it (check and upload included).

The tiles are cut from one random scene at positions jittered by up to +-4 pixels, so the tables are what a
registration finds.  Prints one JSON line.

    python tools/register_bench.py [--planes 4] [--windows 5] [--window-ms 300]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import hotpath, register  # noqa: E402

GRID, TILE, OVERLAP, MAX_SHIFT = 8, 1024, 102, 8


def timed(fns, windows, window_ms):
    """{name: (median, min, max, calls per window)} milliseconds per call: three warm-up calls each, a pilot to size the
    windows, then ``windows`` rounds of one window per function, each about ``window_ms`` of back-to-back calls between
    two HIP events."""
    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    calls = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(window_ms / max(window(fn, 3), 1e-3)))
    per_call = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            per_call[name].append(window(fn, calls[name]))
    return {name: (float(np.median(v)), float(min(v)), float(max(v)), calls[name]) for name, v in per_call.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    _, hy, hx = hotpath.stitch_geometry(TILE, TILE, OVERLAP)
    pad = 8
    scene = torch.from_numpy(rng.integers(0, 65536, size=(GRID * hy + OVERLAP + 2 * pad,) * 2, dtype=np.uint16)).cuda()
    e = rng.integers(-MAX_SHIFT // 2, MAX_SHIFT // 2 + 1, size=(GRID, GRID, 2))
    one = torch.stack([torch.stack([scene[pad + r * hy + e[r, c, 0]:, pad + c * hx + e[r, c, 1]:][:TILE, :TILE]
                                    for c in range(GRID)]) for r in range(GRID)])
    tiles = torch.stack([one] * args.planes)[:, None].contiguous()  # (planes, 1, R, Cc, ty, tx)
    found = register.register_tiles(tiles[0], OVERLAP, MAX_SHIFT)
    want = e - e[0, 0]
    want = want - (want.min(axis=(0, 1)) + want.max(axis=(0, 1))) // 2
    shifts = found["tile_shift"][0]
    h, w = GRID * hy, GRID * hx
    out = torch.empty((args.planes, 1, h, w), dtype=torch.uint16, device="cuda")
    minmax = torch.empty((args.planes, 2), dtype=torch.float64, device="cuda")
    res = {"tiles": f"{args.planes} x {GRID}x{GRID} x {TILE}^2 u16, overlap {OVERLAP}, max_shift {MAX_SHIFT}",
           "image": [h, w], "table_recovered": bool(np.array_equal(shifts, want)),
           "seams_used": int(found["seam_used"].sum()), "seams": int(found["seam_used"].size)}
    sums, fixed = register.seam_sums(tiles[0], OVERLAP, MAX_SHIFT)
    sums_host, fixed_host = sums.cpu().numpy(), fixed.cpu().numpy()
    solve = []
    for _ in range(9):
        t0 = time.perf_counter()
        delta, score = register.pick_displacements(register.seam_scores(sums_host, fixed_host))
        register.solve_shifts(GRID, GRID, (delta[0], score[0]), 0.5, OVERLAP // 2)
        solve.append((time.perf_counter() - t0) * 1e3)
    res["solve_ms"] = float(np.median(solve))
    kw = dict(apply_flatfield=False, out=out, minmax_out=minmax)
    table = hotpath.shift_tables(shifts, 1, GRID, GRID, OVERLAP, tiles.device)
    fns = {"seam_sums": lambda: register.seam_sums(tiles[0], OVERLAP, MAX_SHIFT),
           "plain": lambda: hotpath.flatfield_stitch(tiles, OVERLAP, **kw),
           "linear": lambda: hotpath.flatfield_stitch(tiles, OVERLAP, blend="linear", **kw),
           "shift": lambda: hotpath.flatfield_stitch(tiles, OVERLAP, shifts=table, **kw),
           "shift+linear": lambda: hotpath.flatfield_stitch(tiles, OVERLAP, blend="linear", shifts=table, **kw),
           "shift (host table)": lambda: hotpath.flatfield_stitch(tiles, OVERLAP, shifts=shifts, **kw)}
    res["ms"] = {name: {"ms": ms, "ms_min": lo, "ms_max": hi, "calls_per_window": n}
                 for name, (ms, lo, hi, n) in timed(fns, args.windows, args.window_ms).items()}
    res["shift_over_plain"] = res["ms"]["shift"]["ms"] / res["ms"]["plain"]["ms"]
    res["shift_linear_over_linear"] = res["ms"]["shift+linear"]["ms"] / res["ms"]["linear"]["ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
