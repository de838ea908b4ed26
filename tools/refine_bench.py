"""Times the circle fit (``hotpath.refine_circles`` = mg_roi_refine_circles) on the MI355X with HIP events, inputs
resident: ``--marks`` markers x 1 channel x ``--time`` timepoints (about 100 000 windows) of ``--roi`` x ``--roi`` uint16
pixels, every window a blurred bright disk (radius 8 .. 25 about a centre within a pixel of the window middle, contrast
3000 over 500, N(0, 40) noise of its own per timepoint), the start circle the rounded truth, ``--rays`` rays with a
reach of ``--reach`` pixels.  In the same process, one after the other in every round so that a drift of the clock or a
neighbour on the machine falls on both alike:

  * ``refine``: the kernel;
  * ``profile``: mg_roi_radial_profile of the same single-channel block without a mask, ``roi // 2`` rings of width 1
    about the same centres -- the neighbour that reads every pixel of every window, where the fit reads an annulus.

Every figure is the median of ``--calls`` timed calls after ``--warmup`` warm-up calls, one pair of events per call.
Before anything is timed two calls are compared bit for bit and the share of windows with status 0 is recorded (the
pictures are easy: all of them should fit).  ``taps`` = 4 rays (4 reach + 1) pixel reads per window, most of them cache
hits; ``window_bytes`` = what the profile kernel has to read.  Writes profiles/refine_bench.json and prints it as one
JSON line.

    python tools/refine_bench.py [--marks 1600] [--time 64] [--roi 100] [--rays 64] [--reach 3] [--calls 20] [--warmup 5]
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


def timed_together(fns, calls, warmup):
    """{name: (median, min, max) milliseconds} of ``calls`` rounds, every function once per round between two HIP
    events of its own, after ``warmup`` rounds."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))} for k, v in ms.items()}


def paint(m, n_t, L, gen):
    """(roi uint16 (m, 1, n_t, L, L), truth float64 (m, 3) = {cy, cx, r}) on the device, a group of markers at a time."""
    rng = np.random.default_rng(0)
    truth = np.concatenate([(L - 1) / 2 + rng.uniform(-1, 1, (m, 2)), rng.uniform(8, 25, (m, 1))], axis=1)
    roi = torch.empty((m, 1, n_t, L, L), dtype=torch.uint16, device="cuda")
    yy, xx = torch.meshgrid(torch.arange(L, device="cuda", dtype=torch.float32),
                            torch.arange(L, device="cuda", dtype=torch.float32), indexing="ij")
    d_truth = torch.from_numpy(truth.astype(np.float32)).cuda()
    for g0 in range(0, m, 100):
        c = d_truth[g0:g0 + 100]
        dist = torch.sqrt((yy[None] - c[:, 0, None, None]) ** 2 + (xx[None] - c[:, 1, None, None]) ** 2)
        clean = 500.0 + 3000.0 * torch.sigmoid((c[:, 2, None, None] - dist) / 0.5)  # (an edge about as wide as a blur of 0.8)
        noisy = clean[:, None] + 40.0 * torch.randn((len(c), n_t, L, L), device="cuda", generator=gen)
        roi[g0:g0 + 100, 0].view(torch.int16).copy_(((noisy.round().clamp(0, 65535).to(torch.int32) + 32768) % 65536 - 32768))
    return roi, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--marks", type=int, default=1600)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--roi", type=int, default=100)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--reach", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    m, n_t, L = args.marks, args.time, args.roi
    gen = torch.Generator(device="cuda").manual_seed(0)
    roi, truth = paint(m, n_t, L, gen)
    circle = torch.from_numpy((np.rint(truth) * 16).astype(np.int32)).cuda()  # (m, 3): one start circle for all timepoints
    centre = circle[:, None, :2].contiguous()
    edges = (np.arange(L // 2 + 1) * 16).astype(np.int32)
    plane = roi[:, 0]

    def refine():
        return hotpath.refine_circles(plane, circle, args.rays, args.reach)

    info, fit = refine()
    again = refine()
    ok = info[..., 0] == 0
    radius_error = (torch.sqrt(fit[..., 2]) - torch.from_numpy(truth[:, 2]).cuda()[:, None])[ok]
    res = {"scale": f"{m} markers x 1 channel x {n_t} timepoints = {m * n_t} windows, roi {L} x {L} uint16, "
                    f"{args.rays} rays, reach {args.reach}; profile: {L // 2} rings of width 1, no mask",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "windows": m * n_t, "window_bytes": roi.numel() * roi.element_size(),
           "taps": 4 * args.rays * (4 * args.reach + 1) * m * n_t,
           "same_bits_twice": bool(torch.equal(info, again[0])) and fit.view(torch.int64).equal(again[1].view(torch.int64)),
           "share_status_0": float(ok.double().mean()),
           "radius_error_px": {"mean": float(radius_error.mean()), "worst": float(radius_error.abs().max())}}
    t = timed_together({
        "refine": refine,
        "profile": lambda: hotpath.radial_profile(roi, None, centre, edges),
    }, args.calls, args.warmup)
    res["refine"] = dict(t["refine"], windows_per_s=m * n_t / (t["refine"]["ms"] * 1e-3))
    res["profile"] = dict(t["profile"], bytes_per_s=res["window_bytes"] / (t["profile"]["ms"] * 1e-3))
    res["refine_over_profile"] = t["refine"]["ms"] / t["profile"]["ms"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
