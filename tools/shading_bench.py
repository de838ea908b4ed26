"""Times the shading model on the MI355X with HIP events: the area downsample, the fit (ALM part and the rest, with
the iteration counts), and the fused apply-and-stitch next to flatfield_stitch with image operands on the same
stack; and the NumPy oracle's fit on the same input.  Input: 8 x 8 tiles of 1024^2, u16, 4 channels (C3's tile
geometry).  Prints one JSON line.

    python tools/shading_bench.py [--reps 5] [--skip-oracle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from magnify_amd import hotpath, shading  # noqa: E402


def timed(fn, reps):
    """Median milliseconds of fn() between HIP events on the current stream (after one warm-up call)."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()
    hotpath.require_gpu()
    import ref_shading as rs

    ch, grid, size = 4, 8, 1024
    stacks = [rs.synthetic_stack(n=grid * grid, size=size, seed=20 + c, strength=0.3 + 0.1 * c)[0] for c in range(ch)]
    host = np.stack(stacks).reshape(ch, 1, grid, grid, size, size)
    tiles = torch.from_numpy(host).cuda()
    train = tiles[0].reshape(-1, size, size)
    res = {"input": f"{ch} ch x {grid}x{grid} tiles of {size}^2 u16"}

    res["downsample_ms"] = timed(lambda: shading.working_stack(train, 128), args.reps)

    # fit: the whole call (after one warm-up fit), and its ALM part alone (passes replayed from the same weights)
    shading.fit(train)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = shading.fit(train)
    torch.cuda.synchronize()
    res["fit_wall_ms"] = (time.perf_counter() - t0) * 1e3
    res["iterations"] = model.iterations
    fitter = shading._Fitter(shading.working_stack(train, 128))
    alm = []
    for _ in range(len(model.iterations)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        it = fitter.run_pass()
        b.record()
        b.synchronize()
        alm.append((a.elapsed_time(b), it))
        _, _, mxa = fitter.fields()
        fitter.reweight(mxa, 0.1)
    res["alm_ms"] = sum(t for t, _ in alm)
    res["alm_iterations"] = [i for _, i in alm]
    res["alm_us_per_iteration"] = 1e3 * res["alm_ms"] / max(1, sum(i for _, i in alm))
    res["fit_rest_ms"] = res["fit_wall_ms"] - res["alm_ms"]
    # host time to enqueue one block of iterations (13 launches each with darkfield) against its device time
    fitter.begin()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    fitter.iterate(shading.BLOCK_ITERATIONS)
    res["enqueue_us_per_iteration"] = (time.perf_counter() - t0) * 1e6 / shading.BLOCK_ITERATIONS
    b.record()
    b.synchronize()
    res["block_device_us_per_iteration"] = a.elapsed_time(b) * 1e3 / shading.BLOCK_ITERATIONS

    flats = torch.stack([model.flatfield] * ch)
    darks = torch.stack([model.darkfield] * ch)
    res["shading_apply_stitch_ms"] = timed(lambda: shading.apply_stitch(tiles, 102, flats, darks), args.reps)
    res["flatfield_stitch_images_ms"] = timed(
        lambda: hotpath.flatfield_stitch(tiles, 102, model.flatfield, model.darkfield), args.reps)
    res["apply_vs_flatfield"] = res["shading_apply_stitch_ms"] / res["flatfield_stitch_images_ms"]

    if not args.skip_oracle:
        t0 = time.perf_counter()
        rs.fit(host[0].reshape(-1, size, size))
        res["oracle_fit_ms"] = (time.perf_counter() - t0) * 1e3
        res["fit_speedup_vs_oracle"] = res["oracle_fit_ms"] / res["fit_wall_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
