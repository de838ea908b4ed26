"""Times the blob finder on the MI355X with HIP events, next to ``mg_plane_minmax`` over the same plane (one streaming
read of it).  Two 4096^2 uint16 planes:

  * ``disks``: about 2000 disks of radius 6 .. 14, 1500 brighter than a background of 100 + Poisson(20) + N(0, 30),
    thresholded at 800: what ``find_blobs`` is for;
  * ``noise``: Bernoulli noise at p = 0.41 (value 1000 where on, threshold 500), 8-connected: just above the
    percolation point, a component through every tile and a few hundred thousand small ones: the labelling's hard case.

Per plane:

  * ``plane_minmax``: the yardstick;
  * ``label_device``: the seven launches of ``mg_blob_labels`` alone, into buffers allocated once;
  * ``label``: ``blobs.label`` as a caller sees it: allocation of the outputs, the launches, and the read-back of
    {K, status} (a host synchronisation);
  * ``select``: ``blobs.select(min_area=20)`` on a fresh copy of the map (the copy is inside the window);
  * ``find_blobs`` (``disks`` only: the noise plane has no windows worth cutting): the whole component on a one-plane
    dataset that is already on the device -- detection, selection, the label-map ROI pass, the dataset.

The variants are timed in interleaved rounds in one process, each in a window of back-to-back calls of about
``--window-ms``; the result is the median, minimum and maximum over the rounds and the ratio of every median to the
yardstick's.  No pass mark.  Writes one JSON document (default profiles/blob_bench.json) and prints it.

    python tools/blob_bench.py [--rounds 7] [--window-ms 300] [--size 4096] [--only PLANE:NAME]

``--only noise:label_device`` runs one variant a few times and writes nothing: the run to put under a kernel-stats
profiler.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import magnify_amd as mg  # noqa: E402
from magnify_amd import _native as nat  # noqa: E402
from magnify_amd import blobs, hotpath  # noqa: E402


def window(fn, n):
    """Milliseconds per call over n back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def disks_plane(size, n_disks=2000, seed=0):
    rng = np.random.default_rng(seed)
    img = 100.0 + rng.poisson(20, size=(size, size)) + rng.normal(0.0, 30.0, size=(size, size))
    cells = int(np.ceil(np.sqrt(n_disks)))
    pitch = size // cells
    yy, xx = np.mgrid[-16:17, -16:17]
    drawn = 0
    for i in range(cells):
        for j in range(cells):
            if drawn == n_disks or pitch < 40:
                break
            r = rng.uniform(6, 14)
            cy, cx = (int(v) for v in (i * pitch + pitch // 2 + rng.integers(-4, 5), j * pitch + pitch // 2 + rng.integers(-4, 5)))
            img[cy - 16:cy + 17, cx - 16:cx + 17][yy * yy + xx * xx <= r * r] += 1500.0
            drawn += 1
    return torch.from_numpy(np.clip(np.rint(img), 0, 65535).astype(np.uint16)).cuda(), drawn


def noise_plane(size, p=0.41, seed=1):
    on = torch.rand((size, size), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) < p
    return (on.to(torch.int32) * 1000).to(torch.uint16)


def variants_of(plane, threshold, cap, with_component):
    h, w = plane.shape
    labels = torch.empty((h, w), dtype=torch.int32, device="cuda")
    stats = torch.empty((cap, 8), dtype=torch.int64, device="cuda")
    head = torch.zeros(2, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(nat.lib().mg_blob_scratch_bytes(h, w, cap)), dtype=torch.uint8, device="cuda")

    def label_device():
        hotpath._call("mg_blob_labels", plane.data_ptr(), nat.dtype_code(plane.dtype), h, w, float(threshold), 0, 8,
                      labels.data_ptr(), head.data_ptr(), stats.data_ptr(), cap, head.data_ptr() + 4,
                      scratch.data_ptr(), scratch.numel(), hotpath._stream())

    found = blobs.label(plane, threshold, max_components=cap)
    kept = blobs.select(found["labels"].clone(), found["stats"], min_area=20)
    info = {"h": h, "w": w, "dtype": "uint16", "input_bytes": plane.numel() * 2, "threshold": threshold,
            "components": found["count"], "kept_min_area_20": kept["count"], "on_fraction": float((found["labels"] >= 0).float().mean())}
    try:  # what is timed is also right: the whole map and the areas against scipy, once
        import scipy.ndimage as ndi

        want, k = ndi.label(plane.cpu().numpy() > threshold, np.ones((3, 3), dtype=bool))
        info["equal_to_scipy"] = bool(k == found["count"] and np.array_equal(found["labels"].cpu().numpy(), want.astype(np.int32) - 1)
                                      and np.array_equal(found["stats"][:, 0].cpu().numpy(), np.bincount(want.reshape(-1))[1:]))
    except ImportError:
        info["equal_to_scipy"] = None
    vs = {"plane_minmax": lambda: hotpath.plane_minmax(plane[None]), "label_device": label_device,
          "label": lambda: blobs.label(plane, threshold, max_components=cap),
          "select": lambda: blobs.select(found["labels"].clone(), found["stats"], min_area=20)}
    if with_component:
        finder = mg.components.get("find_blobs")(threshold=threshold, max_components=cap)
        image = plane[None, None]

        def component():
            ds = mg.Dataset({"image": mg.DataArray(image, ("channel", "time", "im_y", "im_x"))})
            return finder(ds)

        info["marks"] = int(component().roi.sizes["mark"])
        info["roi_length"] = int(component().roi.sizes["roi_y"])
        vs["find_blobs"] = component
    return info, vs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_bench.json"))
    args = ap.parse_args()
    hotpath.require_gpu()
    disks, drawn = disks_plane(args.size)
    info, variants = {}, {}
    for pname, plane, threshold, cap, comp in (("disks", disks, 800, 1 << 20, True),
                                               ("noise", noise_plane(args.size), 500, 1 << 22, False)):
        info[pname], vs = variants_of(plane, threshold, cap, comp)
        variants.update({f"{pname}:{name}": fn for name, fn in vs.items()})
    info["disks"]["drawn"] = drawn
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
    res = {"planes": info, "tile": [blobs.TILE_H, blobs.TILE_W], "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for name, ms in per_call.items():
        pname = name.split(":")[0]
        med, yard = float(np.median(ms)), float(np.median(per_call[f"{pname}:plane_minmax"]))
        res["variants"][name] = {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                                 "calls_per_window": calls[name], "input_GB_per_s": info[pname]["input_bytes"] / med / 1e6,
                                 "ratio_to_plane_minmax": med / yard}
    res["note"] = ("ratio_to_plane_minmax = median ms / the median ms of mg_plane_minmax over the same plane; label and "
                   "find_blobs include host synchronisations (the component count, the kept statistics), select includes "
                   "the copy of the map it rewrites; plane_minmax, label and select include the allocation of their results")
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
