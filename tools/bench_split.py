"""Times the split stage's kernels (clx_label_basins, clx_basin_passes, clx_basin_relabel; 2-D) with HIP events, split_labels as a
user calls it on the host clock around a device synchronise, and for scale what a user does on the host today with the same
summits as markers: scipy.ndimage.watershed_ift of the inverted distance map (other semantics, a timing yardstick only).
Map: tools/bench_measure.py's jittered discs drawn so large that neighbours touch, two grid cells to an object: 2048^2 with
about 2 000 objects, most of them clumps of two cells.  Warm-up, then the median (min, max) of the repeats.  The algorithmic
bytes of every kernel are computed from the shape and set against the HBM peak.

    python tools/bench_split.py [--out FILE] [--repeats 20] [--size 2048]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_measure import dev, disc_map  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure import label_distance_sq  # noqa: E402
from cellulus_amd.split import basin_passes, basins, split_labels  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s (specification)
# the ascent reads a label and a distance and writes a link; a root launch reads a link and writes one (the links it follows are
# re-reads of words other threads read as their own, as the taps of the stencils are: not counted), and the usual map takes
# one; the passes read a label, a distance and a root; the relabelling zeroes the scratch map, reads a root and writes an id
BYTES = {"clx_label_basins": 8 + 4 + 4 + 4, "clx_basin_passes": 12, "clx_basin_relabel": 4 + 4 + 4}


def clump_map(size):
    """discs of radius 15 in grid cells of 32 pixels (clipped to their cell, so neighbours touch along its border), two cells
    side by side to an object"""
    lab, cells = disc_map(size, spacing=32, radius=15, jitter=7)
    n = math.isqrt(cells)
    iy, ix = (lab - 1) // n, (lab - 1) % n
    out = np.where(lab > 0, iy * ((n + 1) // 2) + ix // 2 + 1, 0).astype(np.int32)
    return out, len(np.unique(out)) - 1


def summary(ms):
    return f"{statistics.median(ms):9.4f} ({min(ms):9.4f} .. {max(ms):9.4f}) ms"


def bench(size, repeats, emit):
    labels_h, nobj = clump_map(size)
    npix = labels_h.size
    lab = torch.from_numpy(labels_h).to(dev)
    st, lib = _clx.stream_ptr(dev), _clx.load()
    dist = label_distance_sq(lab).reshape(-1).contiguous()
    root, summits = basins(lab)
    a, b, height = basin_passes(lab)
    pieces = split_labels(lab, 1)
    n0, n1 = len(summits), int(pieces.max())
    emit(f"clumps: {size} x {size}, {nobj} objects, {int((labels_h > 0).sum()) / npix:.0%} of the pixels in objects, {n0} summits, "
         f"{len(a)} passes, {n1} pieces at depth 1; {repeats} repeats: median (min .. max)")

    root = root.reshape(-1).contiguous()
    capacity = 1 << max(10, (8 * n0 - 1).bit_length())
    nbytes = int(lib.clx_label_basins_workspace(npix))
    work = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    root_out = torch.empty(npix, dtype=torch.int32, device=dev)
    summit_list = torch.empty(npix // 64, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    values = torch.empty(capacity, dtype=torch.int64, device=dev)
    summits_d = torch.from_numpy(summits.astype(np.uint32).view(np.int32)).to(dev)
    ids_d = torch.arange(1, n0 + 1, dtype=torch.int32, device=dev)
    out = torch.empty(npix, dtype=torch.int32, device=dev)
    flat = lab.reshape(-1)
    calls = {
        "clx_label_basins": lambda: _clx.call("clx_label_basins", _clx.ptr(flat), _clx.ptr(dist), 2, 1, size, size, summit_list.numel(),
                                              _clx.ptr(root_out), _clx.ptr(summit_list), _clx.ptr(info), _clx.ptr(work), nbytes, st),
        "clx_basin_passes": lambda: _clx.call("clx_basin_passes", _clx.ptr(flat), _clx.ptr(dist), _clx.ptr(root), 2, 1, size, size, capacity,
                                              _clx.ptr(keys), _clx.ptr(values), _clx.ptr(info), st),
        "clx_basin_relabel": lambda: _clx.call("clx_basin_relabel", _clx.ptr(root), npix, _clx.ptr(summits_d), _clx.ptr(ids_d), n0,
                                               _clx.ptr(out), _clx.ptr(info), _clx.ptr(work), nbytes, st),
    }
    for name, call in calls.items():
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        floor_ms = npix * BYTES[name] / HBM_PEAK * 1e3
        emit(f"  {name:18s} (HIP events)  {summary(ms)}: {BYTES[name]} algorithmic bytes a pixel are {floor_ms:.4f} ms at the HBM peak of "
             f"{HBM_PEAK / 1e12:.1f} TB/s, {floor_ms / statistics.median(ms):.1%} of the time")
    assert torch.equal(root_out, root), "the timed call's roots differ from basins()'s"

    for _ in range(3):
        split_labels(lab, 1)
    torch.cuda.synchronize()
    whole = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        split_labels(lab, 1)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    emit(f"  split_labels(depth=1), distance map and host merge included (host clock, synchronised)  {summary(whole)}")

    dist_h = dist.cpu().numpy().reshape(size, size)
    markers = np.where(labels_h > 0, 0, -1).astype(np.int32)
    markers.reshape(-1)[summits] = np.arange(1, n0 + 1)
    cost = (dist_h.max() - dist_h).astype(np.uint16)
    t0 = time.perf_counter()
    ndimage.watershed_ift(cost, markers, structure=np.ones((3, 3), dtype=bool))
    host_s = time.perf_counter() - t0
    emit(f"  scipy.ndimage.watershed_ift from the same summits (host, one run; it floods across labels)  {host_s * 1e3:9.1f} ms: "
         f"{host_s * 1e3 / statistics.median(whole):.0f}x split_labels")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_split needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    bench(args.size, args.repeats, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
