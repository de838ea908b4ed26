"""Times the kernels of ``magnify_amd.plot`` on the MI355X with HIP events, inputs resident, every figure the median of
``--calls`` timed calls after ``--warmup`` warm-up calls (one pair of events per call), as tools/drift_bench.py does.
The stack: ``--channels`` x ``--time`` planes of 4096 x 4096 uint16 (4 x 64: 8 GiB), ``--marks`` markers per timepoint
with ``L = 100`` windows and a disk of radius 20 .. 40 as every mask, one mask per (marker, timepoint).

  * ``bin_planes``: mg_bin_planes with ``bin = 8`` over the same C T planes -- the yardstick of the level-3 render: the
    same bytes in the same read pattern;
  * ``plane_minmax``: mg_plane_minmax over the same planes -- what the level-0 render is reported next to;
  * ``render``: mg_render_overview at levels 3 and 0 with the "outline" overlay (``hotpath.render_overview``: the
    output allocation and the launch), its bytes (image + labels read, picture written) per second; level 3 also as a
    multiple of the yardstick's time, level 0 of ``plane_minmax``'s;
  * ``render_plain``: the same without an overlay;
  * ``labels``: mg_roi_image_labels at the same levels (``hotpath.image_labels``: the zero fill of the map and the
    launch), and ``labels_shared``: the same with one mask per marker for all timepoints (time stride 0).

Prints one JSON line.

    python tools/overview_bench.py [--channels 4] [--time 64] [--marks 2000] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import hotpath, plot, track, utils  # noqa: E402

SIDE, L = 4096, 100


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


def rate(t, n_bytes):
    return dict(t, bytes=int(n_bytes), GB_per_s=n_bytes / (t["ms"] * 1e-3) / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--marks", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    n_c, n_t, m = args.channels, args.time, args.marks
    image = torch.empty((n_c, n_t, SIDE, SIDE), dtype=torch.uint16, device="cuda")
    for c in range(n_c):  # white noise over the whole uint16 range
        image[c].view(torch.int16).copy_(torch.randint(0, 65536, (n_t, SIDE, SIDE), dtype=torch.int32, device="cuda") - 32768)
    yy, xx = np.mgrid[0:L, 0:L]
    radii = rng.integers(20, 41, size=m)
    disks = ((yy - L // 2) ** 2 + (xx - L // 2) ** 2)[None] <= (radii ** 2)[:, None, None]
    shared = torch.from_numpy(disks).cuda()[:, None].expand(m, n_t, L, L)  # one mask per marker: time stride 0
    fg = shared.contiguous()  # one per (marker, timepoint)
    centres = rng.integers(0, SIDE, size=(2, m, n_t))
    origin = torch.from_numpy(np.stack([utils.window_origin(centres[1], L, SIDE), utils.window_origin(centres[0], L, SIDE)], axis=-1).astype(np.int32)).cuda()
    table = torch.from_numpy(np.repeat(np.asarray(plot.MARK_COLORS, dtype=np.uint8)[np.arange(m) % 8][:, None], n_t,
                                       axis=1).copy()).cuda()
    limits, colors = [(1000.0, 60000.0)] * n_c, plot.default_colors(n_c)
    planes = image.view(n_c * n_t, SIDE, SIDE)
    plane_bytes = planes.numel() * 2
    res = {"stack": f"{n_c} channels x {n_t} timepoints, {SIDE}^2 u16, {m} markers per timepoint, L {L}", "calls": args.calls,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    t_bin = timed(lambda: track.bin_planes(planes, 8), args.calls, args.warmup)
    res["bin_planes"] = rate(t_bin, plane_bytes + n_c * n_t * (SIDE // 8) ** 2 * 4)
    t_mm = timed(lambda: hotpath.plane_minmax(planes), args.calls, args.warmup)
    res["plane_minmax"] = rate(t_mm, plane_bytes)
    for level, (yard_name, yard) in ((3, ("bin_planes", t_bin)), (0, ("plane_minmax", t_mm))):
        side = SIDE >> level
        out = {}
        labels = hotpath.image_labels(fg, origin, level, SIDE, SIDE)
        out["labelled_pixels"] = int((labels > 0).sum().item())
        moved = plane_bytes + n_t * side * side * (4 + 3)
        t = timed(lambda: hotpath.render_overview(image, level, limits, colors, labels, table, "outline"), args.calls,
                  args.warmup)
        out["render"] = dict(rate(t, moved), **{"over_" + yard_name: t["ms"] / yard["ms"]})
        t = timed(lambda: hotpath.render_overview(image, level, limits, colors), args.calls, args.warmup)
        out["render_plain"] = dict(rate(t, plane_bytes + n_t * side * side * 3), **{"over_" + yard_name: t["ms"] / yard["ms"]})
        t = timed(lambda: hotpath.image_labels(fg, origin, level, SIDE, SIDE), args.calls, args.warmup)
        out["labels"] = rate(t, fg.numel() + n_t * side * side * 4)
        t = timed(lambda: hotpath.image_labels(shared, origin, level, SIDE, SIDE), args.calls, args.warmup)
        out["labels_shared"] = t
        del labels
        res[f"level_{level}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
