"""Times the rotation kernel (mg_affine_bilinear) on the MI355X with HIP events, next to the project's streaming pass
over the same bytes: ``hotpath.flatfield_stitch(..., apply_flatfield=False)`` with overlap 0 on the same image (a
copy with the per-plane min/max).  Cases: one 7376^2 u16 plane (a stitched 8 x 8 chip) and a 4 x 4096^2 u16 assay, at
1 and at 45 degrees.  GB/s are by compulsory bytes: every pixel read once and written once.  Prints one JSON line.

    python tools/rotate_bench.py [--windows 5] [--window-ms 500]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import _native as nat  # noqa: E402
from magnify_amd import hotpath  # noqa: E402


def timed(fn, windows, window_ms):
    """(median, min, max) milliseconds per call of fn(): three warm-up calls, a pilot to size the windows, then
    ``windows`` windows of back-to-back calls between two HIP events, each about ``window_ms`` long."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    n = max(3, int(window_ms / max(window(3), 1e-3)))
    per_call = [window(n) for _ in range(windows)]
    return float(np.median(per_call)), float(min(per_call)), float(max(per_call)), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=500.0)
    args = ap.parse_args()
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    res = {"cases": []}
    for name, shape in (("1 x 7376^2 u16", (1, 1, 7376, 7376)), ("4 x 4096^2 u16", (4, 1, 4096, 4096))):
        c, t, h, w = shape
        image = torch.from_numpy(rng.integers(0, 65536, size=shape, dtype=np.uint16)).cuda()
        out = torch.empty_like(image)
        minmax = torch.empty((c * t, 2), dtype=torch.float64, device="cuda")
        init = hotpath._minmax_init(c * t, image.device)
        gbytes = 2 * image.numel() * image.element_size() / 1e9
        case = {"image": name, "compulsory_GB": gbytes}

        def copy_pass():
            hotpath.flatfield_stitch(image.view(c, t, 1, 1, h, w), 0, apply_flatfield=False, out=out, minmax_out=minmax)

        ms, lo, hi, n = timed(copy_pass, args.windows, args.window_ms)
        case["flatfield_stitch_copy"] = {"ms": ms, "ms_min": lo, "ms_max": hi, "GB_per_s": gbytes / ms * 1e3, "calls_per_window": n}
        for angle in (1.0, 45.0):
            m, off = hotpath.rotation_matrix_offset(angle, h, w)
            m, off = np.ascontiguousarray(m), np.ascontiguousarray(off)

            def rotate_pass():
                minmax.copy_(init)
                hotpath._call("mg_affine_bilinear", image.data_ptr(), out.data_ptr(), nat.dtype_code(image.dtype), c * t, h,
                              w, m.ctypes.data, off.ctypes.data, minmax.data_ptr(), hotpath._stream())

            ms, lo, hi, n = timed(rotate_pass, args.windows, args.window_ms)
            case[f"rotate_{angle:g}_deg"] = {"ms": ms, "ms_min": lo, "ms_max": hi, "GB_per_s": gbytes / ms * 1e3,
                                             "calls_per_window": n}
        res["cases"].append(case)
        del image, out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
