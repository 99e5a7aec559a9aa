"""Times the measure stage's convex hull entry point (clx_region_hull: the row-span pass over the label map, then a wave
per object for the chains and the brute-force geometry) beside clx_region_moments on the same map.  The two share the
reading frame (4 pixels a lane, a ballot cutting the wave into runs), so clx_region_moments is the yardstick for the map
pass; what clx_region_hull takes beyond it is the per-object work.  The inference benchmark's geometry: discs of radius
12 on a jittered grid, 4096^2 (6 400 objects) and 512^2, as in tools/bench_topology.py.
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  Two more label maps of the
same size separate reading from the rest: an all-background map (loads, comparisons, ballots only; no row, no object)
and a map that is one object (one run a wave; one object of `size` rows, whose two chains are a lane each).
A kernel leg is 10 calls one after the other on the same 67 MB map, which fits in the 256 MB Infinity Cache: after the
first call the reads need not reach HBM.  The "of the HBM peak" column is algorithmic bytes over time, set against the
HBM peak as a yardstick; it is not measured HBM traffic (no counters are taken here).

    python tools/bench_hull.py [--out FILE] [--rounds 5]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_measure import PEAK_TBS, dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402


def bench(size, rounds, emit):
    labels_h, nobj = disc_map(size)
    nid = nobj + 1
    npix = size * size
    lab = torch.from_numpy(labels_h).to(dev)
    maps = {"discs": lab, "background": torch.zeros_like(lab), "one object": torch.ones_like(lab)}
    st = _clx.stream_ptr(dev)
    area = torch.empty(nid, dtype=torch.int64, device=dev)
    sum1 = torch.empty((nid, 3), dtype=torch.int64, device=dev)
    sum2 = torch.empty((nid, 6), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    hull = torch.empty((nid, 5), dtype=torch.int64, device=dev)
    state = {}

    def moments(name="discs", bbox=None):
        bbox = state[name]["bbox"] if bbox is None else bbox
        _clx.call("clx_region_moments", _clx.ptr(maps[name]), 1, size, size, nid, _clx.ptr(area), _clx.ptr(bbox), _clx.ptr(sum1),
                  _clx.ptr(sum2), _clx.ptr(bad), st)

    # per map: the bounding boxes of clx_region_moments, left on the device, and the prefix sum over their rows
    for name in maps:
        bbox = torch.empty((nid, 6), dtype=torch.int32, device=dev)
        moments(name, bbox)
        b = bbox.cpu().numpy().astype(np.int64)
        rows_of = np.where(b[:, 4] >= 0, b[:, 4] - b[:, 1] + 1, 0)
        rows_of[0] = 0
        rows = int(rows_of.sum())
        nbytes = int(_clx.load().clx_region_hull_workspace(rows))
        state[name] = dict(bbox=bbox, rows=rows, nbytes=nbytes, row_base=torch.from_numpy(np.cumsum(rows_of) - rows_of).to(dev),
                           work=torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev))

    def hull_call(name="discs"):
        s = state[name]
        _clx.call("clx_region_hull", _clx.ptr(maps[name]), 2, 1, size, size, nid, _clx.ptr(s["bbox"]), _clx.ptr(s["row_base"]),
                  s["rows"], _clx.ptr(s["work"]), s["nbytes"], _clx.ptr(hull), _clx.ptr(bad), st)

    for name, fn in (("clx_region_hull", hull_call), ("clx_region_moments", moments)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        emit(f"{size} x {size}: first call of {name}: {(time.perf_counter() - t0) * 1e3:.1f} ms (host clock, includes set-up)")
    # faster and wrong is not faster: a disc away from the image edge has the same hull wherever it lies
    hull_call()
    assert int(bad.item()) == 0
    h = hull.cpu().numpy()
    b = state["discs"]["bbox"].cpu().numpy()
    whole = np.flatnonzero((b[:, 4] - b[:, 1] == 24) & (b[:, 5] - b[:, 2] == 24))
    assert len(whole) > nobj // 2 and (h[whole] == h[whole[0]]).all(), "the discs' hulls differ"
    a2, nv, f2, c, l2 = (int(v) for v in h[whole[0]])
    hull_call("one object")
    assert hull[1].tolist() == [2 * npix, 4, 2 * size * size, npix, size * size] and int(bad.item()) == 0

    legs = {"clx_region_hull": hull_call, "clx_region_moments": moments}
    for name in maps:
        if name != "discs":
            legs[f"clx_region_hull, {name}"] = lambda name=name: hull_call(name)
            legs[f"clx_region_moments, {name}"] = lambda name=name: moments(name)
    reps = {k: 10 for k in legs}
    times = time_legs(legs, rounds, reps)

    emit(f"{size} x {size}, {nobj} objects, {state['discs']['rows']} rows in their boxes; a whole disc: area_convex {a2 / 2:g}, "
         f"{nv} vertices, Feret max {f2 ** 0.5:.3f}, min {c / l2 ** 0.5:.3f}; {rounds} rounds, legs alternating; ms per call: "
         "min (max) of the rounds")
    best = {}
    for name, ts in times.items():
        lo, hi = min(ts), max(ts)
        best[name] = (lo, hi)
        # the label map once; the calls also clear their outputs (moments: 108 bytes an id; hull: 8 bytes a row) and the
        # hull writes 40 bytes an id
        which = name.split(", ")[1] if ", " in name else "discs"
        nbytes = npix * 4 + (nid * 40 + state[which]["rows"] * 8 if "hull" in name else nid * 108)
        tbs = nbytes / (lo * 1e-3) / 1e12
        emit(f"  {name:48s} {lo:9.4f} ({hi:9.4f}) ms   {nbytes / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {tbs / PEAK_TBS:4.2f} of the "
             f"{PEAK_TBS:.0f} TB/s HBM peak")
    for name in maps:
        suffix = "" if name == "discs" else f", {name}"
        t, m = best["clx_region_hull" + suffix], best["clx_region_moments" + suffix]
        emit(f"  clx_region_hull / clx_region_moments, {name}: {t[0] / m[0]:.2f}x (worst round of the hull against the best of the "
             f"moments: {t[1] / m[0]:.2f}x)")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 512])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hull needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for size in args.sizes:
        bench(size, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
