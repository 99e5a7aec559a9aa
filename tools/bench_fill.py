"""Times the fill stage's kernel (cellulus_amd.fill -> clx_label_holes, 2-D) on one workload: the territories of
tools/bench_propagate.py on 2048^2 (its 2 025 seeds grown inside its mask along its membrane image) with about 1 % of the object
pixels zeroed by a fixed seed -- pinholes inside the territories, and notches where a zeroed pixel lies on a territory's rim.
Warm-up, then the median (min .. max) of the repeats with HIP events around the whole call (five launches and the clearing of
info).  Two yardsticks beside the time: clx_cc_label_filter on the same map in the same run -- the nearest existing kernel, a
union-find over the other class of pixels, for scale and not a target -- and the time the call's algorithmic bytes would take at
the HBM peak.  Before anything is timed the device map, rows and info are compared with the restatement of tests/fill_ref.py on
a 512^2 crop.

    python tools/bench_fill.py [--out FILE] [--repeats 20] [--size 2048]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bench_measure import dev, disc_map  # noqa: E402
from bench_propagate import membrane  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.expand import expand_labels, nearest_object  # noqa: E402
from cellulus_amd.fill import fill_holes, hole_table  # noqa: E402
from cellulus_amd.propagate import geodesic_owner  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s (specification)
# per pixel: runs reads the map (4) and writes a parent (4); link reads the map (4; the row above is a re-read of what the wave
# above read as its own); flatten reads and, on zeros, rewrites the parents (4 + 4); reduce reads the parents (4); fill reads
# the map and the parents and writes out (12).  The root attributes and the neighbours of inner zeros are not counted
BYTES_PER_PIXEL = 8 + 4 + 8 + 4 + 12
KNOCKED = 0.01                          # share of the object pixels zeroed
SEED = 7


def summary(ms):
    return f"{statistics.median(ms):9.4f} ({min(ms):9.4f} .. {max(ms):9.4f}) ms"


def workload(size):
    labels_h, nobj = disc_map(size, spacing=46, radius=10, jitter=5)
    seeds = torch.from_numpy(labels_h).to(dev)
    mask = (expand_labels(seeds, 20) > 0).to(torch.uint8).contiguous()
    weight = membrane(nearest_object(seeds)[0]).contiguous()
    territories = geodesic_owner(seeds, mask, weight)[0].cpu().numpy()
    knocked = (np.random.default_rng(SEED).random(territories.shape) < KNOCKED) & (territories > 0)
    return np.where(knocked, 0, territories).astype(np.int32), nobj, int(knocked.sum())


def bench(size, repeats, emit):
    labels_h, nobj, knocked = workload(size)
    npix = labels_h.size
    labels = torch.from_numpy(labels_h).to(dev).reshape(-1)
    st, lib = _clx.stream_ptr(dev), _clx.load()

    from fill_ref import ref_hole_table, ref_holes

    crop = np.ascontiguousarray(labels_h[:512, :512])
    assert np.array_equal(fill_holes(crop, device=dev), ref_holes(crop)[0]), "fill_holes differs from the restatement on the crop"
    got, want = hole_table(crop, device=dev), ref_hole_table(crop)
    assert all(np.array_equal(got[k], want[k]) for k in want), "hole_table differs from the restatement on the crop"

    out = torch.empty(npix, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    capacity = max(1024, npix // 64)
    rows = torch.empty((capacity, 4), dtype=torch.int32, device=dev)
    nbytes = int(lib.clx_label_holes_workspace(2, 1, size, size))
    work = torch.empty(max(nbytes, int(lib.clx_cc_workspace(npix))) // 4 + 1, dtype=torch.int32, device=dev)

    def holes():
        _clx.call("clx_label_holes", _clx.ptr(labels), 2, 1, size, size, 0, -1, capacity, _clx.ptr(out), _clx.ptr(rows), _clx.ptr(info),
                  _clx.ptr(work), nbytes, st)

    def components():
        _clx.call("clx_cc_label_filter", _clx.ptr(labels), _clx.ptr(out), 1, size, size, 1, _clx.ptr(info), _clx.ptr(work), st)

    holes()
    found = info.tolist()
    assert found[0] <= capacity
    emit(f"territories: {size} x {size}, {nobj} objects, {int((labels_h > 0).sum()) / npix:.0%} of the pixels, {knocked} object pixels zeroed "
         f"(seed {SEED}); {found[2]} background components, {found[0]} holes, {found[1]} pixels filled; {repeats} repeats: median (min .. max)")
    times = {}
    for name, run in (("clx_label_holes, no cap", holes), ("clx_cc_label_filter, min_size 1", components)):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        times[name] = statistics.median(ms)
        emit(f"  {name:34s} (HIP events) {summary(ms)}")
    ours, theirs = times["clx_label_holes, no cap"], times["clx_cc_label_filter, min_size 1"]
    floor_ms = npix * BYTES_PER_PIXEL / HBM_PEAK * 1e3
    emit(f"  clx_label_holes takes {ours / theirs:.2f} times clx_cc_label_filter; {BYTES_PER_PIXEL} algorithmic bytes a pixel are "
         f"{npix * BYTES_PER_PIXEL / 1e6:.1f} MB, {floor_ms:.4f} ms at the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s, {floor_ms / ours:.1%} of the time")
    emit(f"  workspace {nbytes / npix:.0f} bytes a pixel; no counters were taken; 3-D was not timed")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fill needs a HIP device")
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
