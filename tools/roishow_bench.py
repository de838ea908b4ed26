"""Times the kernels of ``plot.percentile_limits`` and ``plot.roishow`` on the MI355X with HIP events, inputs resident,
every figure the median of ``--calls`` timed calls after ``--warmup`` warm-up calls (one pair of events per call), as
tools/overview_bench.py does.

Percentiles -- the stack of tools/overview_bench.py, ``--channels`` x ``--time`` planes of 4096 x 4096 uint16 (4 x 64:
8 GiB), once as white noise over the whole uint16 range and once as a narrow distribution, 100 + Poisson(20) with 0.1 %
bright pixels:

  * ``bin_planes``: mg_bin_planes with ``bin = 8`` over the same planes -- the yardstick: one read-once pass;
  * ``first_pass`` / ``refine_pass``: one mg_percentile_histogram launch over the whole stack (the 11 leading bits; the
    5 trailing bits inside the coarse bins of the 1 % and 99.8 % ranks of channel 0), as a multiple of the yardstick;
  * ``percentiles``: ``hotpath.percentiles(image[c], (1, 99.8))`` for every channel -- two read passes per channel and
    the host's look at the tables between them -- as a multiple of the yardstick (the target: passes x 1.5).

Montage -- ``--marks`` markers x ``--channels`` x ``--time`` windows of L = 100 uint16, a disk as every fg mask and a
ring as every bg mask (one per marker, time stride 0), at level 0 and at the default level:

  * ``render_overview``: mg_render_overview without overlay on an image with as many pixels per timepoint and channel
    as the windows have, at the same level -- the yardstick;
  * ``montage`` (overlay "fill") and ``montage_plain`` (no overlay): mg_render_roi_montage, as a multiple of it.

Prints one JSON line and writes it to ``--out`` (profiles/roishow_bench.json).

    python tools/roishow_bench.py [--channels 4] [--time 64] [--marks 2000] [--calls 20] [--warmup 5]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import _native as nat  # noqa: E402
from magnify_amd import hotpath, plot, track  # noqa: E402

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


def fill_noise(t16):
    """White noise over the whole uint16 range into a uint16 tensor, a leading slice at a time."""
    for part in t16:
        part.view(torch.int16).copy_(torch.randint(0, 65536, part.shape, dtype=torch.int32, device="cuda") - 32768)


def fill_narrow(t16):
    """100 + Poisson(20), 0.1 % of the pixels bright (uniform in 1000 .. 60000)."""
    for part in t16:
        for plane in part:
            v = 100.0 + torch.poisson(torch.full(plane.shape, 20.0, device="cuda"))
            bright = torch.rand(plane.shape, device="cuda") < 1e-3
            v = torch.where(bright, torch.randint(1000, 60001, plane.shape, device="cuda").float(), v)
            plane.view(torch.int16).copy_((v.to(torch.int32) + 32768) % 65536 - 32768)


def percentile_part(args, res):
    n_c, n_t = args.channels, args.time
    image = torch.empty((n_c, n_t, SIDE, SIDE), dtype=torch.uint16, device="cuda")
    planes = image.view(n_c * n_t, SIDE, SIDE)
    plane_bytes = planes.numel() * 2
    for name, fill in (("white_noise", fill_noise), ("narrow", fill_narrow)):
        fill(image)
        out = {}
        t_bin = timed(lambda: track.bin_planes(planes, 8), args.calls, args.warmup)
        out["bin_planes"] = rate(t_bin, plane_bytes + n_c * n_t * (SIDE // 8) ** 2 * 4)
        hist = torch.zeros((2, 2048), dtype=torch.int64, device="cuda")
        code = nat.dtype_code(image.dtype)

        def launch(shift, bits, prefixes):
            pre = np.asarray(prefixes, dtype=np.uint32)
            hotpath._call("mg_percentile_histogram", image.data_ptr(), code, 1, 0, n_c * n_t, SIDE * SIDE, SIDE * SIDE, shift,
                          bits, shift + bits if len(pre) else 0, pre.ctypes.data if len(pre) else 0, len(pre), hist.data_ptr(),
                          hotpath._stream())

        t = timed(lambda: launch(5, 11, []), args.calls, args.warmup)
        out["first_pass"] = dict(rate(t, plane_bytes), over_bin_planes=t["ms"] / t_bin["ms"])
        lim = hotpath.percentiles(image[0], (1.0, 99.8))
        prefixes = sorted({int(v) >> 5 for v in lim})
        t = timed(lambda: launch(0, 5, prefixes), args.calls, args.warmup)
        out["refine_pass"] = dict(rate(t, plane_bytes), over_bin_planes=t["ms"] / t_bin["ms"], prefixes=prefixes)
        t = timed(lambda: [hotpath.percentiles(image[c], (1.0, 99.8)) for c in range(n_c)], args.calls, args.warmup)
        out["percentiles"] = dict(rate(t, 2 * plane_bytes), over_bin_planes=t["ms"] / t_bin["ms"], read_passes=2,
                                  target=2 * 1.5, limits_channel_0=[float(v) for v in lim])
        res["percentiles_" + name] = out
    del image, planes


def montage_part(args, res):
    n_c, n_t, m = args.channels, args.time, args.marks
    rng = np.random.default_rng(0)
    roi = torch.empty((m, n_c, n_t, L, L), dtype=torch.uint16, device="cuda")
    fill_noise(roi.view(-1).chunk(32))
    yy, xx = np.mgrid[0:L, 0:L]
    d2 = ((yy - L // 2) ** 2 + (xx - L // 2) ** 2)[None]
    radii = rng.integers(20, 41, size=m)
    disks = d2 <= (radii ** 2)[:, None, None]
    rings = (d2 > ((radii + 2) ** 2)[:, None, None]) & (d2 <= ((radii + 8) ** 2)[:, None, None])
    fg = torch.from_numpy(disks).cuda()[:, None].expand(m, n_t, L, L)  # one mask per marker: time stride 0
    bg = torch.from_numpy(rings).cuda()[:, None].expand(m, n_t, L, L)
    side = math.isqrt(m * L * L - 1) + 1  # an image with as many pixels per plane as the m windows have
    image = torch.empty((n_c, n_t, side, side), dtype=torch.uint16, device="cuda")
    fill_noise(image)
    limits, colors = [(1000.0, 60000.0)] * n_c, plot.default_colors(n_c)
    layout = plot.montage_layout(None, m)
    rows, cols = layout.shape
    roi_bytes, image_bytes = roi.numel() * 2, image.numel() * 2
    res["montage_stack"] = f"{m} markers x {n_c} channels x {n_t} timepoints, L {L} u16; layout {rows} x {cols}; yardstick image {side}^2"
    for level in sorted({0, plot.montage_level(rows, cols, L)}):
        lk = -(L // -(1 << level))
        sk = -(side // -(1 << level))
        out = {"cell": lk, "picture": [rows * lk, cols * lk]}
        t_ov = timed(lambda: hotpath.render_overview(image, level, limits, colors), args.calls, args.warmup)
        out["render_overview"] = rate(t_ov, image_bytes + n_t * sk * sk * 3)
        pic = n_t * rows * lk * cols * lk * 3
        t = timed(lambda: hotpath.render_roi_montage(roi, layout, level, limits, colors, fg, bg, "fill"), args.calls, args.warmup)
        out["montage"] = dict(rate(t, roi_bytes + pic), over_render_overview=t["ms"] / t_ov["ms"])
        t = timed(lambda: hotpath.render_roi_montage(roi, layout, level, limits, colors), args.calls, args.warmup)
        out["montage_plain"] = dict(rate(t, roi_bytes + pic), over_render_overview=t["ms"] / t_ov["ms"])
        res[f"montage_level_{level}"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--marks", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roishow_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    res = {"stack": f"{args.channels} channels x {args.time} timepoints, {SIDE}^2 u16", "calls": args.calls,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    percentile_part(args, res)
    torch.cuda.empty_cache()
    montage_part(args, res)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
