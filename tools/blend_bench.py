"""Times the stitch pass (``hotpath.flatfield_stitch``, pass 2 only: the maxima are made once) with ``blend=None``
next to ``blend="linear"`` on the same tiles, on the MI355X with HIP events: an 8 x 8 grid of 1024 x 1024 uint16 tiles,
overlap 102 (a 7376 x 7376 chip), ``--planes`` planes, without a correction and with a float32 flat image.  The two
modes alternate window by window, so that drift of the machine falls on both.  GB/s are by compulsory bytes of the
plain pass: every kept pixel read once and written once.  Prints one JSON line.

    python tools/blend_bench.py [--planes 4] [--windows 5] [--window-ms 400] [--modes none,linear]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import hotpath  # noqa: E402

GRID, TILE, OVERLAP = 8, 1024, 102


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
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--modes", default="none,linear")
    args = ap.parse_args()
    modes = [None if m == "none" else m for m in args.modes.split(",")]
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    tiles = torch.from_numpy(rng.integers(0, 65536, size=(args.planes, 1, GRID, GRID, TILE, TILE), dtype=np.uint16)).cuda()
    yy, xx = np.mgrid[0:TILE, 0:TILE]
    flat = torch.from_numpy((1 - 0.15 * (((yy - 511.5) / 512) ** 2 + ((xx - 511.5) / 512) ** 2)).astype(np.float32)).cuda()
    _, hy, hx = hotpath.stitch_geometry(TILE, TILE, OVERLAP)
    h, w = GRID * hy, GRID * hx
    out = torch.empty((args.planes, 1, h, w), dtype=torch.uint16, device="cuda")
    minmax = torch.empty((args.planes, 2), dtype=torch.float64, device="cuda")
    gbytes = 2 * out.numel() * out.element_size() / 1e9
    bands = sum(b - a for a, b in hotpath.blend_bands(GRID, TILE, OVERLAP))
    res = {"tiles": f"{args.planes} x {GRID}x{GRID} x {TILE}^2 u16, overlap {OVERLAP}", "image": [h, w],
           "compulsory_GB": gbytes, "band_pixel_share": 1 - ((h - bands) / h) * ((w - bands) / w), "cases": {}}
    max2 = hotpath.flatfield_max(tiles, flat, 100.0)
    for case, kw in (("no correction", dict(apply_flatfield=False)),
                     ("float32 flat, dark 100", dict(flatfield=flat, darkfield=100.0, max2=max2))):
        fns = {str(m): (lambda m=m: hotpath.flatfield_stitch(tiles, OVERLAP, out=out, minmax_out=minmax, blend=m, **kw))
               for m in modes}
        res["cases"][case] = {name: {"ms": ms, "ms_min": lo, "ms_max": hi, "GB_per_s": gbytes / ms * 1e3, "calls_per_window": n}
                              for name, (ms, lo, hi, n) in timed(fns, args.windows, args.window_ms).items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
