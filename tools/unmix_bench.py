"""Times the per-pixel unmixing kernels on the MI355X with HIP events, inputs resident, at a C2-like block: ``--marks``
markers x 4 and 9 channels x 1 timepoint of ``--roi`` x ``--roi`` uint16 pixels under one disk mask per marker (radii
5 .. 25), 3 lanthanides for 4 channels and 5 for 9, q = (0.25, 0.5, 0.75), an offset per (marker, channel).  In the same
process, one after the other in every round so that a drift of the clock or a neighbour on the machine falls on all alike:

  * ``unmix_stats``: mg_roi_unmix_stats (``hotpath.unmix_stats``);
  * ``masked_stats``: mg_roi_masked_stats with the same q over the same channels and mask -- one order-statistics
    problem per channel where the unmixing has one per derived value (2 n_ln - 1 of them);
  * ``read_ceiling``: one streaming read of as many bytes as the block and its masks hold, by the library's own
    16-byte-per-lane probe (mode 1).

and for whole planes, ``--plane`` x ``--plane`` uint16 pixels per channel:

  * ``unmix_planes``: mg_unmix_planes with ratios (``hotpath.unmix_planes``);
  * ``copy``: a device-to-device copy of the same input bytes.

Every figure is the median of ``--calls`` timed calls after ``--warmup`` warm-up calls, one pair of events per call.
Two calls of the statistics are compared bit for bit before anything is timed.  Writes profiles/unmix_bench.json and
prints it as one JSON line.

    python tools/unmix_bench.py [--marks 2000] [--roi 100] [--plane 4096] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from magnify_amd import _native as nat, hotpath  # noqa: E402
from profile_bench import timed_together  # noqa: E402

Q = (0.25, 0.5, 0.75)
SHAPES = ((4, 3), (9, 5))  # (channels, lanthanides)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--marks", type=int, default=2000)
    ap.add_argument("--roi", type=int, default=100)
    ap.add_argument("--plane", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unmix_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    m, L, side = args.marks, args.roi, args.plane
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:L, :L]
    radii = rng.integers(5, 26, size=m)
    middle = (L - 1) / 2
    disks = ((yy - middle) ** 2 + (xx - middle) ** 2)[None] <= (radii ** 2)[:, None, None]
    mask = torch.from_numpy(disks.astype(np.uint8)).cuda()
    res = {"scale": f"{m} markers x C channels x 1 timepoint, roi {L} x {L} uint16, one disk mask per marker (r 5..25, "
                    f"{int(disks.sum(axis=(1, 2)).mean())} pixels on average), q = {Q}; planes {side} x {side} uint16",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "lds_key_bytes": hotpath.UNMIX_LDS_KEY_BYTES}
    for n_c, n_ln in SHAPES:
        w = rng.normal(0, 1, (n_ln, n_c))
        roi = torch.randint(-32768, 32768, (m, n_c, 1, L, L), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint16)
        off = torch.rand((m, n_c, 1), dtype=torch.float64, device="cuda", generator=gen) * 100
        n_bytes = roi.numel() * roi.element_size() + mask.numel()
        first = hotpath.unmix_stats(roi, mask, w, None, off, Q)
        again = hotpath.unmix_stats(roi, mask, w, None, off, Q)
        in_lds = [hotpath.unmix_keys_in_lds(n_ln, int(n)) for n in (disks.sum(axis=(1, 2)).max(), L * L)]
        case = {"channels": n_c, "lanthanides": n_ln, "derived": 2 * n_ln - 1, "bytes": n_bytes,
                "largest_mask_in_lds": in_lds[0], "whole_window_in_lds": in_lds[1],
                "same_bits_twice": all(a.view(torch.int32 if a.dtype == torch.int32 else torch.int64).equal(
                    b.view(torch.int32 if b.dtype == torch.int32 else torch.int64)) for a, b in zip(first, again))}
        probe_bytes = n_bytes // 4096 * 4096
        src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda").random_(0, 256)
        sink = torch.zeros(4, dtype=torch.int32, device="cuda")
        t = timed_together({
            "unmix_stats": lambda: hotpath.unmix_stats(roi, mask, w, None, off, Q),
            "masked_stats": lambda: hotpath.masked_stats(roi, mask, Q),
            "read_ceiling": lambda: nat.check(nat.lib().mg_stream_probe(src.data_ptr(), None, probe_bytes, 1, sink.data_ptr(),
                                                                        0, hotpath._stream()), "mg_stream_probe"),
        }, args.calls, args.warmup)
        for key in ("unmix_stats", "masked_stats"):
            case[key] = dict(t[key], bytes_per_s=n_bytes / (t[key]["ms"] * 1e-3))
        case["read_ceiling"] = dict(t["read_ceiling"], bytes=probe_bytes, bytes_per_s=probe_bytes / (t["read_ceiling"]["ms"] * 1e-3))
        case["unmix_over_masked_stats"] = case["unmix_stats"]["ms"] / case["masked_stats"]["ms"]
        case["unmix_us_per_window"] = case["unmix_stats"]["ms"] * 1e3 / m
        del roi, src
        # whole planes
        image = torch.randint(-32768, 32768, (n_c, 1, side, side), dtype=torch.int16, device="cuda", generator=gen).view(torch.uint16)
        spare = torch.empty_like(image)
        n_out = 2 * n_ln - 1
        read, written = image.numel() * image.element_size(), n_out * side * side * 4
        t = timed_together({"unmix_planes": lambda: hotpath.unmix_planes(image, w, None, None, True),
                            "copy": lambda: spare.copy_(image)}, args.calls, args.warmup)
        case["unmix_planes"] = dict(t["unmix_planes"], bytes_read=read, bytes_written=written,
                                    bytes_per_s=(read + written) / (t["unmix_planes"]["ms"] * 1e-3))
        case["copy"] = dict(t["copy"], bytes_read=read, bytes_written=read, bytes_per_s=2 * read / (t["copy"]["ms"] * 1e-3))
        res[f"c{n_c}"] = case
        del image, spare
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
