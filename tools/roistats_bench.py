"""Times the masked ROI statistics (``hotpath.masked_stats`` = mg_roi_masked_stats) on the MI355X with HIP events,
inputs resident, every figure the median of ``--calls`` timed calls after ``--warmup`` warm-up calls (one pair of
events per call), at the scale of tools/track_bench.py: ``--marks`` markers x 1 channel x ``--time`` timepoints of
``--roi`` x ``--roi`` pixels under one disk mask per marker (radii 8 .. 25), uint16 and float32:

  * ``stats_q0`` / ``stats_q1`` / ``stats_q7``: the kernel with q = (), (0.5,) and the seven-value list;
  * ``median``: mg_roi_masked_median on the same roi and mask -- the same kernel in its median mode (one double per
    window, no deviations; it was a kernel of its own, one read of the window per radix level, until DESIGN.md
    section 22); it should not be slower than q = (0.5,);
  * ``read_ceiling``: one streaming read of the same number of bytes by the library's own 16-byte-per-lane probe.

``bytes`` = what the kernel has to read: every pixel and every mask byte of every window once; the rates are those
bytes over the median time.  The results of both entry points are compared before anything is timed.  ``--roi 111``
puts the windows beyond the LDS budget: the path that selects from global memory.  Prints one JSON line.

    python tools/roistats_bench.py [--marks 2000] [--time 64] [--roi 100] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import _native as nat, hotpath, reduce  # noqa: E402

Q7 = (0, 0.01, 0.25, 0.5, 0.75, 0.998, 1)


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
    ap.add_argument("--marks", type=int, default=2000)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--roi", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    hotpath.require_gpu()
    m, n_t, L = args.marks, args.time, args.roi
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:L, :L]
    radii = rng.integers(8, 26, size=m)
    centre = (L - 1) / 2
    disks = ((yy - centre) ** 2 + (xx - centre) ** 2)[None] <= (radii ** 2)[:, None, None]
    mask = torch.from_numpy(disks.astype(np.uint8)).cuda()
    res = {"scale": f"{m} markers x 1 channel x {n_t} timepoints, roi {L} x {L}, one disk mask per marker (r 8..25)",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "mean_pixels_under_mask": float(disks.sum(axis=(1, 2)).mean())}
    for name in ("uint16", "float32"):
        if name == "uint16":
            roi = torch.randint(-32768, 32768, (m, 1, n_t, L, L), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint16)
        else:
            roi = torch.randn((m, 1, n_t, L, L), dtype=torch.float32, device="cuda", generator=gen)
        n_bytes = roi.numel() * (roi.element_size() + 1)
        # the same answers first: q = 0.5 interpolated the nanquantile way is the nanmedian for these types
        count, _, order = hotpath.masked_stats(roi, mask, (0.5,))
        median = hotpath.masked_median(roi, mask)
        case = {"bytes": n_bytes, "in_lds": hotpath.masked_stats_keys_in_lds(roi.dtype, L),
                "median_agrees": bool(torch.equal(reduce.interpolate_quantiles(count, order, (0.5,))[..., 0], median))}
        for key, q in (("stats_q0", ()), ("stats_q1", (0.5,)), ("stats_q7", Q7)):
            t = timed(lambda: hotpath.masked_stats(roi, mask, q), args.calls, args.warmup)
            case[key] = dict(t, bytes_per_s=n_bytes / (t["ms"] * 1e-3))
        t = timed(lambda: hotpath.masked_median(roi, mask), args.calls, args.warmup)
        case["median"] = dict(t, bytes_per_s=n_bytes / (t["ms"] * 1e-3))
        case["stats_q1_over_median_max"] = case["stats_q1"]["ms"] / case["median"]["ms_max"]
        case["stats_q1_over_median"] = case["stats_q1"]["ms"] / case["median"]["ms"]
        probe_bytes = n_bytes // 4096 * 4096
        src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda").random_(0, 256)
        sink = torch.zeros(4, dtype=torch.int32, device="cuda")
        t = timed(lambda: nat.check(nat.lib().mg_stream_probe(src.data_ptr(), None, probe_bytes, 1, sink.data_ptr(), 0,
                                                              hotpath._stream()), "mg_stream_probe"), args.calls, args.warmup)
        case["read_ceiling"] = dict(t, bytes=probe_bytes, bytes_per_s=probe_bytes / (t["ms"] * 1e-3))
        case["stats_q0_share_of_ceiling"] = case["stats_q0"]["bytes_per_s"] / case["read_ceiling"]["bytes_per_s"]
        res[name] = case
        del roi, src
    print(json.dumps(res))


if __name__ == "__main__":
    main()
