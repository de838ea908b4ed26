"""Times ``segment_rois``' kernel (mg_roi_threshold_masks) on the MI355X with HIP events, inputs resident, every figure
the median of ``--calls`` timed calls after ``--warmup`` warm-up calls (one pair of events per call):

  * ``beads``: ``--beads`` markers x ``--time`` timepoints of roi_length ``--roi`` uint16 windows (the C4 block),
    one drawn mask for all timepoints, ``allowed`` given;
  * ``chip``: 784 markers x 1 timepoint of roi_length 72, masks per timepoint, no ``allowed``;
  * beside each, mg_roi_masked_stats (no quantiles) under the drawn foreground of the same block: the sibling that
    reads the same window bytes.

Every window is ``100 + Poisson(20)`` with an 800-count ellipse (semi-axes 0.2 L x 0.07 L) under a drawn disk of radius
0.14 L; the drawn background is the annulus between 0.2 L and 0.42 L.  Settings: Otsu, open 1, grow 4, guard 2.
``bytes``: the window, the masks read and the two masks written, once each.  Prints one JSON line.

    python tools/segment_bench.py [--beads 2000] [--time 64] [--roi 100] [--calls 20] [--warmup 5]
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


def block(m, n_t, L, per_time, seed):
    """roi (m, 1, n_t, L, L) uint16 on the device and the drawn masks fg0, bg0 (m, n_t or 1, L, L) bool."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(L, device="cuda"), torch.arange(L, device="cuda"), indexing="ij")
    c = L // 2
    r2 = (yy - c) ** 2 + (xx - c) ** 2
    ellipse = ((yy - c) / (0.07 * L)) ** 2 + ((xx - c) / (0.2 * L)) ** 2 <= 1.0
    roi = torch.empty((m, 1, n_t, L, L), dtype=torch.uint16, device="cuda")
    step = max(1, (1 << 26) // (n_t * L * L))
    for g in range(0, m, step):
        part = roi[g:g + step]
        noise = torch.poisson(torch.full(part.shape, 20.0, device="cuda"), generator=gen) + 100.0 + 800.0 * ellipse
        part.view(torch.int16).copy_(noise.to(torch.int16))
    t_masks = n_t if per_time else 1
    fg0 = (r2 <= (0.14 * L) ** 2).expand(m, t_masks, L, L).contiguous()
    bg0 = ((r2 > (0.2 * L) ** 2) & (r2 <= (0.42 * L) ** 2)).expand(m, t_masks, L, L).contiguous()
    return roi, fg0, bg0


def case(m, n_t, L, per_time, with_allowed, calls, warmup):
    roi, fg0, bg0 = block(m, n_t, L, per_time, seed=m + L)
    allowed = (fg0 | bg0) if with_allowed else None
    fg, bg, thr, counts, seg = hotpath.threshold_masks(roi[:, 0], fg0, bg0, allowed)
    n = L * L
    moved = m * n_t * n * (2 + (3 if with_allowed else 2) + 2)
    t_seg = timed(lambda: hotpath.threshold_masks(roi[:, 0], fg0, bg0, allowed), calls, warmup)
    t_stats = timed(lambda: hotpath.masked_stats(roi, fg0), calls, warmup)
    stats_moved = m * n_t * n * 3
    return {"shape": f"{m} markers x {n_t} timepoints, roi_length {L}, uint16, masks per "
                     f"{'timepoint' if per_time else 'marker'}, allowed {'given' if with_allowed else 'NULL'}",
            "segmented_fraction": float(seg.to(torch.float64).mean().item()),
            "mean_fg_count": float(counts[..., 0].to(torch.float64).mean().item()),
            "threshold_masks": dict(t_seg, bytes=moved, gb_per_s=moved / (t_seg["ms"] * 1e-3) / 1e9,
                                    windows_per_s=m * n_t / (t_seg["ms"] * 1e-3)),
            "masked_stats": dict(t_stats, bytes=stats_moved, gb_per_s=stats_moved / (t_stats["ms"] * 1e-3) / 1e9),
            "threshold_masks_over_masked_stats": t_seg["ms"] / t_stats["ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beads", type=int, default=2000)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--roi", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    hotpath.require_gpu()
    res = {"calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "settings": "otsu, open_radius 1, max_grow 4, bg_guard 2, min_area 1"}
    res["beads"] = case(args.beads, args.time, args.roi, False, True, args.calls, args.warmup)
    torch.cuda.empty_cache()
    res["chip"] = case(784, 1, 72, True, False, args.calls, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
