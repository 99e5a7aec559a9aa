"""Times the relate stage's two kernels (clx_label_overlaps: the sparse joint histogram of two label maps; clx_region_clearance:
per child the smallest value of its parent's distance map) beside the one other kernel that reads two label maps at once,
clx_joint_histogram (csrc/evaluate.hip), on the same maps in the same run.  Both histograms read two int32 maps: 8 bytes a
pixel, which is what "TB/s of map bytes" divides by; the clearance kernel reads the distance map too, 12 bytes a pixel.
clx_joint_histogram fills a dense #a x #b table that its caller zeroes before every call, which is timed as a leg of its own
and as part of "dense, with its zero fill"; clx_label_overlaps clears its own table of `capacity` slots inside the call.
Ids stay below 2^16 so that the dense kernel can run.
Maps at 4096^2, three object densities: cells are discs on a jittered grid grown until no background is left
(tools/bench_inscribed.py's "touching" map), nuclei smaller discs around the same grid points moved by up to a third of
the spacing, so that some straddle two cells.  Before anything is timed the sparse set is compared with the dense table
and the clearance rows with a restatement (one mask per child) on a sample of the children.
The two maps are 128 MiB and fit the 256 MiB Infinity Cache, from which back-to-back calls on the same maps read them; the
"from HBM" legs take their maps from four copies in rotation, so that every call reads maps that 384 MiB (576 MiB with
the distance maps) of other traffic have displaced.
HIP events, warm-up, the legs alternating inside every round; median, min and max over the rounds.

    python tools/bench_relate.py [--out FILE] [--rounds 7]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_inscribed import touching_map  # noqa: E402
from bench_measure import dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure import _pair_capacity, label_distance_sq  # noqa: E402
from cellulus_amd.relate import assign_parents  # noqa: E402

OVERLAPS, CLEARANCE = "clx_label_overlaps", "clx_region_clearance"
DENSE, ZERO, DENSE_ZERO = "clx_joint_histogram (dense yardstick)", "zero fill of the dense table", "dense, with its zero fill"
HBM = ", maps from HBM"
COPIES = 4
NOTES = """hipcc (gfx950, -O3) reports: overlaps_kernel 42 VGPRs, 8192 bytes of LDS; clearance_kernel 61 VGPRs, 7168 bytes of LDS; neither
spills, 8 waves a SIMD for both (a grid of 1024 blocks is 4 waves a SIMD).
Neither kernel is bound by reading its maps: maps from HBM cost 3 - 14 % over maps from the Infinity Cache, and
clx_label_overlaps takes 2.7 times as long on the dense map as on the sparse one for the same bytes.  Its time grows with the
number of runs a wave holds (every run's head and every lane on an edge makes a chain of LDS atomics: load, compare-and-swap,
add) and with the pairs every block flushes into the global table.  Two things were tried.  Loading the next trip's pixels
before the current trip's are counted, which both kernels now do: the first version, without it, took 0.0485 / 0.0856 / 0.1256 ms
(overlaps) and 0.0566 / 0.0621 / 0.0659 ms (clearance) on the three maps from the cache.  A grid of 2048 blocks for
clx_label_overlaps (8 waves a SIMD, twice the flushes): 0.0508 / 0.0758 / 0.1201 ms, better on one map and worse on two; not kept.
No counters were taken."""


def maps(size, spacing, seed=1):
    """(nuclei, cells, objects): the same grid, the nuclei's centres moved by up to spacing / 3"""
    discs, nobj = disc_map(size, spacing, spacing // 4, spacing // 8, seed)
    cells = touching_map(discs)
    nuclei, _ = disc_map(size, spacing, spacing // 5, spacing // 3, seed + 1)
    return nuclei, cells, nobj


def bench(name, nuclei_h, cells_h, nobj, rounds, emit):
    size = nuclei_h.shape[0]
    npix = nuclei_h.size
    nid = nobj + 1
    a, b = (torch.from_numpy(v).to(dev).reshape(-1) for v in (nuclei_h, cells_h))
    st = _clx.stream_ptr(dev)
    capacity = _pair_capacity(2 * nobj)                      # what relate() starts with
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    counts = torch.empty(capacity, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    identity = torch.arange(nid, dtype=torch.int32, device=dev)           # id -> row / column of the dense table
    joint = torch.zeros((nid, nid), dtype=torch.int64, device=dev)
    out = torch.empty((nid, 3), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    turn = [0]

    def rotate(copies):
        turn[0] = (turn[0] + 1) % COPIES
        return copies[turn[0]]

    def overlaps(a=a, b=b):
        _clx.call(OVERLAPS, _clx.ptr(a), _clx.ptr(b), npix, nid, nid, capacity, _clx.ptr(keys), _clx.ptr(counts), _clx.ptr(info), st)

    def dense(a=a, b=b):
        _clx.call("clx_joint_histogram", _clx.ptr(a), _clx.ptr(b), npix, _clx.ptr(identity), _clx.ptr(identity), nid, _clx.ptr(joint), st)

    def zero():
        joint.zero_()

    def dense_zero():
        zero()
        dense()

    # faster and different is not faster: the sparse set against the dense table
    overlaps()
    dense_zero()
    torch.cuda.synchronize()
    flags, used = info.tolist()
    assert flags == 0, f"clx_label_overlaps reported {flags}"
    slot = torch.nonzero(keys).reshape(-1)
    k = keys[slot]
    want = torch.nonzero(joint)
    want = want[(want[:, 0] > 0) | (want[:, 1] > 0)]
    order = torch.argsort(k)
    assert used == len(want) and torch.equal(k[order], (want[:, 0] << 32) | want[:, 1]), "the sparse set differs from the dense table"
    assert torch.equal(counts[slot][order], joint[want[:, 0], want[:, 1]]), "the sparse counts differ from the dense table"
    k_h = k[order].cpu().numpy()
    label, parent, _ = assign_parents(k_h >> 32, k_h & 0xFFFFFFFF, counts[slot][order].cpu().numpy())
    table = np.zeros(nid, dtype=np.int32)
    table[label] = parent
    parent_d = torch.from_numpy(table).to(dev)
    dist = label_distance_sq(b.reshape(size, size)).reshape(-1)

    def clearance(a=a, b=b, dist=dist):
        _clx.call(CLEARANCE, _clx.ptr(a), _clx.ptr(b), _clx.ptr(dist), _clx.ptr(parent_d), npix, nid, _clx.ptr(out), _clx.ptr(bad), st)

    clearance()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    out_h, dist_h = out.cpu().numpy(), dist.cpu().numpy().astype(np.int64)
    fa, fb = nuclei_h.reshape(-1), cells_h.reshape(-1)
    for i in label[:: max(1, len(label) // 64)]:             # a sample of the children, one mask each
        p = np.flatnonzero((fa == i) & (fb == table[i]))
        row = [len(p), min((int(dist_h[q]) << 32) | int(q) for q in p), int(dist_h[p].sum())] if len(p) else [0, -1, 0]
        assert out_h[i].tolist() == row, f"clx_region_clearance differs from the restatement for child {i}"

    copies = [(a.clone(), b.clone(), dist.clone()) for _ in range(COPIES)]
    legs = {OVERLAPS: overlaps, CLEARANCE: clearance, DENSE: dense, ZERO: zero, DENSE_ZERO: dense_zero,
            OVERLAPS + HBM: lambda: overlaps(*rotate(copies)[:2]), CLEARANCE + HBM: lambda: clearance(*rotate(copies)),
            DENSE + HBM: lambda: dense(*rotate(copies)[:2])}
    times = time_legs(legs, rounds, {k: 10 for k in legs})
    emit(f"{name}: {size} x {size}, {nobj} cells without background between them, {len(label)} nuclei over "
         f"{int((nuclei_h > 0).sum()) / npix:.0%} of the pixels, {used} pairs in a table of {capacity} slots; dense table "
         f"{nid} x {nid} x 8 bytes = {nid * nid * 8 / 2 ** 20:.0f} MiB; {rounds} rounds, legs alternating; ms per call: median (min - max)")
    med = {k: float(np.median(v)) for k, v in times.items()}
    for leg, ts in times.items():
        line = f"  {leg:54s} {med[leg]:9.4f} ({min(ts):9.4f} - {max(ts):9.4f}) ms"
        if leg != ZERO:
            line += f"  {npix * 8 / (med[leg] * 1e-3) / 1e12:5.2f} TB/s of map bytes"
        if leg in (OVERLAPS, CLEARANCE):
            line += f"  {med[leg] / med[DENSE]:5.2f}x the dense kernel alone, {med[leg] / med[DENSE_ZERO]:5.2f}x with its zero fill"
        if leg in (OVERLAPS + HBM, CLEARANCE + HBM):
            line += f"  {med[leg] / med[DENSE + HBM]:5.2f}x the dense kernel alone on such maps"
        emit(line)
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", type=int, default=4096)
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    if not torch.cuda.is_available():
        raise SystemExit("bench_relate needs a HIP device")
    emit(f"device: {torch.cuda.get_device_name(0)}")
    for name, spacing in (("sparse", 102), ("medium", 51), ("dense", 32)):
        bench(f"{name} (grid spacing {spacing})", *maps(args.size, spacing), args.rounds, emit)
    emit(NOTES)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
