"""Times the background kernels (``magnify_amd.background``: ``estimate`` and ``subtract`` at radius 4, 32 and 128, and
both with ``smooth=1`` at radius 32) on one block on the MI355X with HIP events, next to a plain device-to-device copy
of the same planes (``Tensor.copy_``: one read and one write of every pixel; the opening reads a block four times and
writes it three times) and next to ``despeckle.median`` of the same block (what ``smooth=1`` adds).  The block: 16
uint16 planes of 4096^2, noise around a level that rises across the plane, with bright disks.  The variants are timed in
interleaved rounds in one process: every round times each variant once, in a window of back-to-back calls of about
``--window-ms``; the result is the median, minimum and maximum over the rounds, and for every variant the ratio of its
median to the copy's.  No pass mark: the ratios are the record.  Writes one JSON document (default
profiles/background_bench.json) and prints it.

    python tools/background_bench.py [--planes 16] [--size 4096] [--rounds 7] [--window-ms 200] [--only NAME]

``--only NAME`` runs one variant a few times and writes nothing: the run to put under a kernel-stats profiler.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from magnify_amd import background, despeckle, hotpath  # noqa: E402

RADII = (4, 32, 128)


def window(fn, n):
    """Milliseconds per call over n back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def make_block(planes, size):
    gen = torch.Generator(device="cuda").manual_seed(0)
    noise = torch.randint(90, 131, (planes, size, size), dtype=torch.int32, device="cuda", generator=gen)
    yy = torch.arange(size, device="cuda", dtype=torch.int32)
    noise += (10 * yy)[None, None, :] + (3 * yy)[None, :, None]  # a level that rises across and down the plane
    disk = ((yy[:, None] % 128 - 64) ** 2 + (yy[None, :] % 128 - 64) ** 2) <= 20 ** 2  # a bead every 128 pixels
    noise += 2000 * disk[None].to(torch.int32)
    return noise.to(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    block = make_block(args.planes, args.size)
    spare = torch.empty_like(block)
    in_bytes = block.numel() * block.element_size()
    variants = {"copy": lambda: spare.copy_(block), "median_k1": lambda: despeckle.median(block, 1)}
    for radius in RADII:
        variants[f"estimate_r{radius}"] = lambda radius=radius: background.estimate(block, radius)
        variants[f"subtract_r{radius}"] = lambda radius=radius: background.subtract(block, radius)
    variants["estimate_r32_smooth1"] = lambda: background.estimate(block, 32, 1)
    variants["subtract_r32_smooth1"] = lambda: background.subtract(block, 32, 1)
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
    res = {"block": {"planes": args.planes, "h": args.size, "w": args.size, "dtype": "uint16", "input_bytes": in_bytes},
           "rows": background.ROWS, "cols": background.COLS, "span": background.SPAN,
           "scratch_limit_bytes": background.SCRATCH_LIMIT, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "variants": {}}
    copy = float(np.median(per_call["copy"]))
    for name, ms in per_call.items():
        med = float(np.median(ms))
        res["variants"][name] = {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                                 "calls_per_window": calls[name], "input_GB_per_s": in_bytes / med / 1e6,
                                 "ratio_to_copy": med / copy}
    v = res["variants"]
    res["ratio_r128_to_r4"] = {what: v[f"{what}_r128"]["ms_median"] / v[f"{what}_r4"]["ms_median"]
                               for what in ("estimate", "subtract")}
    res["note"] = ("ratio_to_copy = median ms / the median ms of the copy; a call includes the allocation of the result "
                   "and of the scratch (torch's caching allocator) and goes to the entry in groups of planes whose scratch "
                   "stays within scratch_limit_bytes; the smooth1 variants run despeckle's median of every group first")
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
