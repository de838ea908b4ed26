"""Times the radial profile (``hotpath.radial_profile`` = mg_roi_radial_profile) on the MI355X with HIP events, inputs
resident, on the block of tools/roistats_bench.py: ``--marks`` markers x 1 channel x ``--time`` timepoints of ``--roi`` x
``--roi`` pixels under one disk mask per marker (radii 8 .. 25), uint16 and float32, ``--rings`` rings of width 1 about
the window middle.  In the same process, one after the other in every round so that a drift of the clock or a
neighbour on the machine falls on all three alike:

  * ``profile``: the kernel;
  * ``stats_q0``: mg_roi_masked_stats with q = () on the same roi and mask -- it reads the same bytes;
  * ``read_ceiling``: one streaming read of as many bytes by the library's own 16-byte-per-lane probe (mode 1).

Every figure is the median of ``--calls`` timed calls after ``--warmup`` warm-up calls, one pair of events per call.
``bytes`` = what the kernel has to read: every pixel and every mask byte of every window once; the rates are those bytes
over the median time.  The counts are compared with mg_roi_masked_stats' before anything is timed (under a mask that
lies inside the last ring the two count the same pixels), and two calls are compared bit for bit.  Writes
profiles/profile_bench.json and prints it as one JSON line.

    python tools/profile_bench.py [--marks 2000] [--time 64] [--roi 100] [--rings 50] [--calls 20] [--warmup 5] [--mask disk|all]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import _native as nat, hotpath  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--marks", type=int, default=2000)
    ap.add_argument("--time", type=int, default=64)
    ap.add_argument("--roi", type=int, default=100)
    ap.add_argument("--rings", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mask", choices=("disk", "all"), default="disk", help="all: a mask of ones, every pixel takes part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    m, n_t, L = args.marks, args.time, args.roi
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:L, :L]
    radii = rng.integers(8, 26, size=m)
    middle = (L - 1) / 2
    disks = ((yy - middle) ** 2 + (xx - middle) ** 2)[None] <= (radii ** 2)[:, None, None]
    if args.mask == "all":
        disks = np.ones_like(disks)
    mask = torch.from_numpy(disks.astype(np.uint8)).cuda()
    centre = torch.full((m, 1, 2), int(np.rint(middle * 16)), dtype=torch.int32, device="cuda")
    edges = (np.arange(args.rings + 1) * 16).astype(np.int32)
    what = "one disk mask per marker (r 8..25)" if args.mask == "disk" else "a mask of ones"
    res = {"scale": f"{m} markers x 1 channel x {n_t} timepoints, roi {L} x {L}, {what}, "
                    f"{args.rings} rings of width 1 about the window middle",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name in ("uint16", "float32"):
        if name == "uint16":
            roi = torch.randint(-32768, 32768, (m, 1, n_t, L, L), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint16)
        else:
            roi = torch.randn((m, 1, n_t, L, L), dtype=torch.float32, device="cuda", generator=gen)
        n_bytes = roi.numel() * (roi.element_size() + 1)
        count, moments = hotpath.radial_profile(roi, mask, centre, edges)
        again = hotpath.radial_profile(roi, mask, centre, edges)
        n_stats, stats, _ = hotpath.masked_stats(roi, mask, ())
        case = {"bytes": n_bytes, "same_bits_twice": bool(torch.equal(count, again[0])) and
                moments.view(torch.int64).equal(again[1].view(torch.int64))}
        if args.rings >= 26 and args.mask == "disk":  # every disk lies inside the last ring: the rings' counts add up to the mask's
            case["counts_agree"] = bool(torch.equal(count.sum(-1).to(torch.int32), n_stats))
            if name == "uint16":
                case["sums_agree"] = bool(torch.equal(moments[..., 0].sum(-1), stats[..., 0]))
        probe_bytes = n_bytes // 4096 * 4096
        src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda").random_(0, 256)
        sink = torch.zeros(4, dtype=torch.int32, device="cuda")
        t = timed_together({
            "profile": lambda: hotpath.radial_profile(roi, mask, centre, edges),
            "stats_q0": lambda: hotpath.masked_stats(roi, mask, ()),
            "read_ceiling": lambda: nat.check(nat.lib().mg_stream_probe(src.data_ptr(), None, probe_bytes, 1, sink.data_ptr(),
                                                                        0, hotpath._stream()), "mg_stream_probe"),
        }, args.calls, args.warmup)
        for key in ("profile", "stats_q0"):
            case[key] = dict(t[key], bytes_per_s=n_bytes / (t[key]["ms"] * 1e-3))
        case["read_ceiling"] = dict(t["read_ceiling"], bytes=probe_bytes, bytes_per_s=probe_bytes / (t["read_ceiling"]["ms"] * 1e-3))
        case["profile_over_stats_q0"] = case["profile"]["ms"] / case["stats_q0"]["ms"]
        case["profile_share_of_ceiling"] = case["profile"]["bytes_per_s"] / case["read_ceiling"]["bytes_per_s"]
        case["stats_q0_share_of_ceiling"] = case["stats_q0"]["bytes_per_s"] / case["read_ceiling"]["bytes_per_s"]
        res[name] = case
        del roi, src
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
