"""Times the two passes of ``skew.estimate_rotation`` on the MI355X with HIP events, next to ``mg_plane_minmax`` over the
same plane (one streaming read of it: what a pass that reads the plane once can be held against).  Two planes: the
1100^2 test chip (tests/synth.draw_chip((10, 10), 20), tilted by 4 degrees) and an 8192^2 uint16 plane with a grid of
disks of the same pitch at the same tilt, drawn on the device.  Per plane:

  * ``plane_minmax``: the yardstick;
  * ``coarse``: ``mg_bin_planes``, ``mg_plane_minmax`` of the binned plane and ``mg_skew_profiles`` over the coarse
    angle table on it, with the clearing of the profiles;
  * ``fine``: ``mg_skew_profiles`` over the 51 fine angles on the plane itself, with the clearing of the profiles.

The device work only: the scores (NumPy, on the profiles copied back) are not in the windows.  The variants are timed in
interleaved rounds in one process, each in a window of back-to-back calls of about ``--window-ms``; the result is the
median, minimum and maximum over the rounds and the ratio of every median to the yardstick's.  No pass mark.  Writes one
JSON document (default profiles/skew_bench.json) and prints it.

    python tools/skew_bench.py [--rounds 7] [--window-ms 200] [--feature 16] [--only PLANE:NAME]

``--only chip:fine`` (or ``large:coarse`` ...) runs one variant a few times and writes nothing: the run to put under a
kernel-stats profiler.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from magnify_amd import _native as nat  # noqa: E402
from magnify_amd import hotpath, skew, track  # noqa: E402

TILT = 4.0


def window(fn, n):
    """Milliseconds per call over n back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def test_chip():
    import rotate_ref as rr
    from synth import draw_chip

    return torch.from_numpy(rr.rotate(draw_chip((10, 10), 20), TILT)).cuda()


def large_plane(size=8192, pitch=100, radius=10):
    """uint16 (size, size): level 300 with disks of 1000 on a grid of ``pitch`` tilted by TILT degrees."""
    c, s = math.cos(math.radians(TILT)), math.sin(math.radians(TILT))
    y = torch.arange(size, device="cuda", dtype=torch.float32)[:, None] - (size - 1) / 2
    x = torch.arange(size, device="cuda", dtype=torch.float32)[None, :] - (size - 1) / 2
    u, v = y * c - x * s, x * c + y * s
    disk = (torch.remainder(u, pitch) - pitch / 2) ** 2 + (torch.remainder(v, pitch) - pitch / 2) ** 2 <= radius ** 2
    return (300 + 1000 * disk.to(torch.int32)).to(torch.uint16)


class Pass:
    """One launch sequence of mg_skew_profiles over ``angles`` on ``plane`` with buffers of its own."""

    def __init__(self, plane, angles):
        self.plane, self.table = plane, torch.from_numpy(skew.angle_table(angles)).cuda()
        nb = min(plane.shape) + 2
        self.sums = torch.zeros((len(self.table), 2, nb), dtype=torch.int64, device="cuda")
        self.counts = torch.zeros((len(self.table), 2, nb), dtype=torch.int32, device="cuda")

    def __call__(self, lo=0.0, scale=0.0):
        h, w = self.plane.shape
        self.sums.zero_()
        self.counts.zero_()
        for a in range(0, len(self.table), skew.MAX_ANGLES):
            hotpath._call("mg_skew_profiles", self.plane.data_ptr(), nat.dtype_code(self.plane.dtype), h, w,
                          self.plane.stride(0), lo, scale, self.table[a:].data_ptr(),
                          min(skew.MAX_ANGLES, len(self.table) - a), self.sums[a:].data_ptr(), self.counts[a:].data_ptr(),
                          hotpath._stream())


def variants_of(plane, feature, max_angle=10.0):
    b = skew.coarse_bin(feature)
    binned = track.bin_planes(plane[None], b)[0] if b > 1 else plane
    step, angles = skew.coarse_angles(feature, b, min(binned.shape), max_angle)
    lo, hi = hotpath.plane_minmax(binned[None])[0].tolist()
    coarse_pass = Pass(binned, angles)
    fine_pass = Pass(plane, TILT * -1.0 + np.arange(-skew.FINE_HALF, skew.FINE_HALF + 1) * (step / skew.FINE_HALF))

    def coarse():
        if b > 1:
            track.bin_planes(plane[None], b)
        hotpath.plane_minmax(binned[None])  # (the range is read back on the host in the product; here the launch only)
        coarse_pass(lo, 65535.0 / (hi - lo))

    info = {"h": int(plane.shape[0]), "w": int(plane.shape[1]), "dtype": str(plane.dtype).replace("torch.", ""),
            "input_bytes": plane.numel() * plane.element_size(), "bin": b, "coarse_angles": len(angles),
            "fine_angles": 2 * skew.FINE_HALF + 1, "coarse_step_degrees": step}
    return info, {"plane_minmax": lambda: hotpath.plane_minmax(plane[None]), "coarse": coarse, "fine": fine_pass}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--feature", type=float, default=16)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skew_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    planes = {"chip": test_chip(), "large": large_plane()}
    info, variants = {}, {}
    for pname, plane in planes.items():
        info[pname], vs = variants_of(plane, args.feature)
        variants.update({f"{pname}:{name}": fn for name, fn in vs.items()})
    if args.only:
        for _ in range(5):
            variants[args.only]()
        torch.cuda.synchronize()
        return
    calls = {}
    for name, fn in variants.items():  # warm-up of every shape, and a pilot that sizes the windows
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(args.window_ms / max(window(fn, 3), 1e-3)))
    per_call = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            per_call[name].append(window(fn, calls[name]))
    res = {"planes": info, "feature": args.feature, "tile": nat.DEFINES["MG_SKEW_TILE"], "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for name, ms in per_call.items():
        pname = name.split(":")[0]
        med, yard = float(np.median(ms)), float(np.median(per_call[f"{pname}:plane_minmax"]))
        res["variants"][name] = {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                                 "calls_per_window": calls[name], "input_GB_per_s": info[pname]["input_bytes"] / med / 1e6,
                                 "ratio_to_plane_minmax": med / yard}
    res["note"] = ("ratio_to_plane_minmax = median ms / the median ms of mg_plane_minmax over the same plane; a call "
                   "includes the clearing of the profiles (two memsets) and, for plane_minmax and bin_planes, the "
                   "allocation of the result (torch's caching allocator); the host's scores are not timed")
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
