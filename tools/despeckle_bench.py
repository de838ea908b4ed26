"""Times the hot-pixel kernels (``magnify_amd.despeckle``: ``remove_outliers`` at radius 1 and 2, ``outlier_votes``) on
one block on the MI355X with HIP events, next to a plain device-to-device copy of the same planes (``Tensor.copy_``: one
read and one write of every pixel, the floor of a filter that reads every pixel once and writes it once).  The block: 4
planes of 4096^2 -- one timepoint of the bench -- as uint16 and as float32, noise with about 0.1 % hot pixels.  The
variants are timed in interleaved rounds in one process: every round times each variant once, in a window of
back-to-back calls of about ``--window-ms``; the result is the median, minimum and maximum over the rounds, and for
every kernel the ratio of its median to the copy's of the same dtype.  No pass mark: the ratio is the record.  Writes
one JSON document (default profiles/despeckle_bench.json) and prints it.

    python tools/despeckle_bench.py [--planes 4] [--size 4096] [--rounds 7] [--window-ms 200] [--only NAME]

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

from magnify_amd import despeckle, hotpath  # noqa: E402


def window(fn, n):
    """Milliseconds per call over n back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def make_block(dtype, planes, size):
    rng = np.random.default_rng(0)
    block = rng.integers(90, 131, size=(planes, size, size), dtype=np.uint16)
    block[rng.random(block.shape, dtype=np.float32) < 1e-3] = 60000
    return torch.from_numpy(block.astype(dtype)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--threshold", type=float, default=1000.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despeckle_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    variants, in_bytes = {}, {}
    for name, dtype in (("uint16", np.uint16), ("float32", np.float32)):
        block = make_block(dtype, args.planes, args.size)
        spare = torch.empty_like(block)
        in_bytes[name] = block.numel() * block.element_size()
        variants[f"copy_{name}"] = lambda block=block, spare=spare: spare.copy_(block)
        for k in (1, 2):
            variants[f"remove_outliers_k{k}_{name}"] = lambda block=block, k=k: despeckle.remove_outliers(block, args.threshold, k)
            variants[f"outlier_votes_k{k}_{name}"] = lambda block=block, k=k: despeckle.outlier_votes(block, args.threshold, k)
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
    res = {"block": {"planes": args.planes, "h": args.size, "w": args.size, "input_bytes": in_bytes, "hot_fraction": 1e-3},
           "threshold": args.threshold, "which": "bright", "tile": despeckle.TILE, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for name, ms in per_call.items():
        dtype = name.rsplit("_", 1)[1]
        med = float(np.median(ms))
        res["variants"][name] = {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                                 "calls_per_window": calls[name], "input_GB_per_s": in_bytes[dtype] / med / 1e6,
                                 "ratio_to_copy": med / float(np.median(per_call[f"copy_{dtype}"]))}
    res["note"] = ("ratio_to_copy = median ms / the median ms of the copy of the same dtype; remove_outliers writes every "
                   "pixel as the copy does and zeroes and fills its counts; outlier_votes writes only its int32 table")
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
