"""Times ``reduce.masked_sum`` and ``reduce.masked_mean`` of a Dataset without cached reductions on the MI355X, inputs
resident, masks that differ per timepoint: ``--marks`` markers x ``--channels`` x ``--time`` windows of ``--roi`` x
``--roi`` uint16 pixels, a random ``fg`` per (marker, timepoint).  Every figure is the median of ``--calls`` timed calls
after ``--warmup`` warm-up calls, each between two HIP events (the whole call: the views, every launch, the assembly of
the result).  The sums are compared with torch's before anything is timed.  Prints one JSON line.

    python tools/masked_sum_bench.py [--marks 2000] [--channels 4] [--time 8] [--roi 100] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import magnify_amd as mg  # noqa: E402
from magnify_amd import hotpath, reduce  # noqa: E402
from segment_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--marks", type=int, default=2000)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--time", type=int, default=8)
    ap.add_argument("--roi", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    hotpath.require_gpu()
    m, c, t, L = args.marks, args.channels, args.time, args.roi
    gen = torch.Generator(device="cuda").manual_seed(m + L)
    bits = torch.randint(-32768, 32768, (m, c, t, L, L), device="cuda", generator=gen, dtype=torch.int16)
    roi = bits.view(torch.uint16)
    fg = torch.rand((m, t, L, L), device="cuda", generator=gen) < 0.3
    ds = mg.Dataset({"roi": mg.DataArray(roi, ("mark", "channel", "time", "roi_y", "roi_x"))},
                    coords={"fg": (("mark", "time", "roi_y", "roi_x"), fg)})
    got = reduce.masked_sum(ds, "fg").data
    want = torch.stack([((bits[:, k].to(torch.int64) & 0xFFFF) * fg).sum(dim=(-1, -2)) for k in range(c)], dim=1)
    assert torch.equal(got, want.to(torch.float64)), "masked_sum disagrees with torch"
    res = {"calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "shape": f"{m} markers x {c} channels x {t} timepoints, roi_length {L}, uint16, a mask per timepoint",
           "masked_sum": timed(lambda: reduce.masked_sum(ds, "fg"), args.calls, args.warmup),
           "masked_mean": timed(lambda: reduce.masked_mean(ds, "fg"), args.calls, args.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
