"""Times the four depth folds (``magnify_amd.depth``: project max, project mean, sharpest, fuse) on one block on the
MI355X with HIP events, next to a plain device copy of the same input bytes (``Tensor.copy_`` of the block: it reads
every input byte once, as the projections do, and writes as many, where a projection writes 1 / Z of them).  The block:
8 stacks x Z 9 x 2048^2 uint16 (604 MB) by default, random pixels.  The variants are timed in interleaved rounds in one
process: every round times each variant once, in a window of back-to-back calls of about ``--window-ms``; the result is
the median, minimum and maximum over the rounds, and for every fold the ratio of its median to the copy's.  No pass
mark: the ratio is the record.  Writes one JSON document (default profiles/depth_bench.json) and prints it.

    python tools/depth_bench.py [--stacks 8] [--z 9] [--size 2048] [--window 9] [--rounds 7] [--window-ms 300]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import depth, hotpath  # noqa: E402


def window(fn, n):
    """Milliseconds per call over n back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=8)
    ap.add_argument("--z", type=int, default=9)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--window", type=int, default=9, help="fuse window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    rng = np.random.default_rng(0)
    shape = (args.stacks, args.z, args.size, args.size)
    block = torch.from_numpy(rng.integers(0, 65536, size=shape, dtype=np.uint16)).cuda()
    spare = torch.empty_like(block)
    in_bytes = block.numel() * block.element_size()
    variants = {
        "copy": lambda: spare.copy_(block),
        "project_max": lambda: depth.project(block, "max"),
        "project_mean": lambda: depth.project(block, "mean"),
        "focus_totals": lambda: depth.focus_totals(block),
        "sharpest": lambda: depth.sharpest(block),  # focus_totals, the arg-max on the host (one sync), project pick
        "fuse": lambda: depth.fuse(block, args.window),
    }
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
    res = {"block": {"stacks": args.stacks, "z": args.z, "h": args.size, "w": args.size, "dtype": "uint16",
                     "input_bytes": in_bytes},
           "fuse_window": args.window, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "variants": {}}
    copy_ms = float(np.median(per_call["copy"]))
    for name, ms in per_call.items():
        med = float(np.median(ms))
        res["variants"][name] = {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                                 "calls_per_window": calls[name], "input_GB_per_s": in_bytes / med / 1e6,
                                 "ratio_to_copy": med / copy_ms}
    res["note"] = ("ratio_to_copy = median ms / the copy's median ms on the same input bytes; the copy also writes "
                   "input_bytes, a projection writes input_bytes / z; mg_depth_fuse was not profiled")
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
