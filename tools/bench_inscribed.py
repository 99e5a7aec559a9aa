"""Times the measure stage's label-aware distance map (clx_label_distance_sq, 2-D) and the reduction over it
(clx_region_inscribed) beside the existing binary transform (clx_edt_sq, cap = 0, on the mask `labels != 0` of the same map)
and beside what a user does on the host today: scipy.ndimage.distance_transform_edt of every object's mask on its
bounding-box crop.  clx_edt_sq is the yardstick: code of the same structure (a pass along x, a min-plus pass along y) that
reads one value where the label-aware passes read a label and a distance.  Maps: tools/bench_measure.py's discs of radius 12
on a jittered grid, 4096^2 (6 400 objects) and 512^2, and at 4096^2 the same discs grown until no background is left (every
pixel takes the id of the nearest disc: a sheet of touching cells about 51 pixels across).  On that map the mask has no
zero at all, so clx_edt_sq's searches run the whole length of every row and column: it is timed, with fewer repetitions,
but it measures that degenerate case and not the work of a distance map.  The yardstick there is clx_edt_sq on the mask of
the INTERIOR pixels (label-aware d2 > 1: the cells' rims are the zeros), whose searches are as long as the label-aware
ones less one step.
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  The host leg is one run on the
host clock.  Before anything is timed the kernel's map is compared with the host leg's, element by element.

    python tools/bench_inscribed.py [--out FILE] [--rounds 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_measure import dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402


def touching_map(labels):
    """every background pixel takes the id of the nearest object pixel"""
    idx = ndimage.distance_transform_edt(labels == 0, return_distances=False, return_indices=True)
    return np.ascontiguousarray(labels[tuple(idx)])


def host_distance_sq(labels):
    """scipy per object on the bounding box grown by one pixel (so that a box that is all object still has a candidate)
    -> (int64 map, seconds)"""
    t0 = time.perf_counter()
    out = np.zeros(labels.shape, dtype=np.int64)
    for i, box in enumerate(ndimage.find_objects(labels), 1):
        if box is None:
            continue
        grown = tuple(slice(max(0, s.start - 1), min(n, s.stop + 1)) for s, n in zip(box, labels.shape))
        mask = labels[grown] == i
        d = ndimage.distance_transform_edt(mask)
        out[grown][mask] = np.rint(d * d).astype(np.int64)[mask]
    return out, time.perf_counter() - t0


def bench(name, labels_h, nobj, rounds, emit):
    size = labels_h.shape[0]
    npix = labels_h.size
    nid = nobj + 1
    lab = torch.from_numpy(labels_h).to(dev)
    mask = (lab != 0).to(torch.uint8)
    st = _clx.stream_ptr(dev)
    lib = _clx.load()
    dist = torch.empty(npix, dtype=torch.int32, device=dev)
    work = torch.empty(int(lib.clx_label_distance_workspace(npix)) // 4, dtype=torch.int32, device=dev)
    out = torch.empty((nid, 3), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    edt = torch.empty(npix, dtype=torch.int32, device=dev)
    edt_work = torch.empty((int(lib.clx_edt_workspace(npix)) + 3) // 4, dtype=torch.int32, device=dev)

    def distance():
        _clx.call("clx_label_distance_sq", _clx.ptr(lab), 2, 1, size, size, 0, _clx.ptr(dist), _clx.ptr(work), work.numel() * 4, st)

    def inscribed():
        _clx.call("clx_region_inscribed", _clx.ptr(lab), _clx.ptr(dist), npix, nid, _clx.ptr(out), _clx.ptr(bad), st)

    def edt_sq(m=mask):
        _clx.call("clx_edt_sq", _clx.ptr(m), _clx.ptr(edt), 1, size, size, 0, _clx.ptr(edt_work), st)

    # faster and different is not faster: the kernel's map against the host leg's, the reduction against NumPy on that map
    want, host_s = host_distance_sq(labels_h)
    distance()
    inscribed()
    torch.cuda.synchronize()
    got = dist.cpu().numpy().reshape(labels_h.shape)
    assert np.array_equal(got, want), "clx_label_distance_sq differs from scipy per object"
    assert int(bad.item()) == 0
    rows = out.cpu().numpy()
    d2max = ndimage.maximum(want, labels_h, np.arange(1, nid))
    d2sum = ndimage.sum_labels(want, labels_h, np.arange(1, nid))
    assert np.array_equal(rows[1:, 0], d2max.astype(np.int64)) and np.array_equal(rows[1:, 2], np.rint(d2sum).astype(np.int64))
    background = int((labels_h == 0).sum())

    degenerate = background == 0
    legs = {"clx_label_distance_sq": distance, "clx_region_inscribed": inscribed, "clx_edt_sq (cap 0, mask of the map)": edt_sq}
    reps = {k: 10 for k in legs}
    yardstick = "clx_edt_sq (cap 0, mask of the map)"
    if degenerate:
        reps[yardstick] = 2
        interior = (dist > 1).to(torch.uint8)
        yardstick = "clx_edt_sq (cap 0, mask of d2 > 1)"
        legs[yardstick] = lambda: edt_sq(interior)
        reps[yardstick] = 10
    times = time_legs(legs, rounds, reps)
    emit(f"{name}: {size} x {size}, {nobj} objects, {background / npix:.0%} background, largest inscribed radius "
         f"{float(np.sqrt(rows[1:, 0].max())):.2f}; {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    best = {}
    for leg, ts in times.items():
        best[leg] = (min(ts), max(ts))
        emit(f"  {leg:44s} {min(ts):9.4f} ({max(ts):9.4f}) ms")
    emit(f"  {'scipy per object on crops (host, one run)':44s} {host_s * 1e3:9.1f} ms")
    d, e, r = best["clx_label_distance_sq"], best[yardstick], best["clx_region_inscribed"]
    if degenerate:
        emit("  (the mask of the map has no zero: clx_edt_sq searches every row and column end to end; the yardstick is the mask of d2 > 1)")
    emit(f"  clx_label_distance_sq / {yardstick}: {d[0] / e[0]:.2f}x (worst round against the yardstick's best: {d[1] / e[0]:.2f}x)")
    emit(f"  host / (clx_label_distance_sq + clx_region_inscribed): {host_s * 1e3 / (d[0] + r[0]):.0f}x")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--touching", type=int, nargs="*", default=[4096], help="sizes at which the grown map is timed too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inscribed needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for size in args.sizes:
        labels, nobj = disc_map(size)
        bench("discs", labels, nobj, args.rounds, emit)
    for size in args.touching:
        labels, nobj = disc_map(size)
        bench("touching (the discs grown until no background is left)", touching_map(labels), nobj, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
