"""Times the measure stage's radial distribution (clx_region_radial: count and sum per object, ring and wedge) beside
clx_region_intensity on the same map and channel, the yardstick: code of the same reading frame that streams two 4-byte maps
where clx_region_radial streams three (labels, the distance map, the float32 channel), so 1.5x is the floor by bytes.  Maps at
4096^2: tools/bench_measure.py's discs of radius 12 on a jittered grid (6 400 objects), tools/bench_inscribed.py's "touching"
map (the discs grown until no background is left), and ONE object that fills the map, the contention case: every pixel of a
block lands in a handful of cells.  The distance map and the inscribed rows are the device's own (clx_label_distance_sq,
clx_region_inscribed); the one-object map is measured with `edge` (without it every distance is CLX_DIST_INF).
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  Before anything is timed every
leg's tables are compared with the NumPy restatement of tests/radial_ref.py, which is also timed, once, on the host clock.

    python tools/bench_radial.py [--out FILE] [--rounds 5]
    python tools/bench_radial.py --cells [--out FILE]      # no device: what the block tables see, counted from the restatement
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_inscribed import touching_map  # noqa: E402
from bench_measure import dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure_columns import intensity_shift  # noqa: E402
from radial_ref import ref_radial  # noqa: E402

_RAW_F32 = 0
# (name, rings, width, wedges)
SETTINGS = (("4 rings x 1 wedge, relative", 4, 0, 1), ("4 rings x 8 wedges, relative", 4, 0, 8),
            ("32 rings x 8 wedges, relative", 32, 0, 8), ("4 rings x 1 wedge, absolute, width 2", 4, 2, 1))


def bench(name, labels_h, nobj, edge, rounds, emit):
    size = labels_h.shape[0]
    npix = labels_h.size
    nid = nobj + 1
    lab = torch.from_numpy(labels_h).to(dev)
    raw_h = (np.random.default_rng(0).random((size, size), dtype=np.float32) * 1000.0).astype(np.float32)
    raw = torch.from_numpy(raw_h).to(dev)
    shift = intensity_shift(float(raw_h.max()), npix)
    st = _clx.stream_ptr(dev)
    lib = _clx.load()
    dist = torch.empty(npix, dtype=torch.int32, device=dev)
    work = torch.empty(int(lib.clx_label_distance_workspace(npix)) // 4, dtype=torch.int32, device=dev)
    ins = torch.empty((nid, 3), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    _clx.call("clx_label_distance_sq", _clx.ptr(lab), 2, 1, size, size, int(edge), _clx.ptr(dist), _clx.ptr(work), work.numel() * 4, st)
    _clx.call("clx_region_inscribed", _clx.ptr(lab), _clx.ptr(dist), npix, nid, _clx.ptr(ins), _clx.ptr(bad), st)
    assert int(bad.item()) == 0
    row_h = np.arange(-1, nid - 1, dtype=np.int32)          # row[id] = id - 1
    row = torch.from_numpy(row_h).to(dev)
    nrows = nid - 1
    cells = nrows * 32 * 8
    count = torch.empty(cells, dtype=torch.int64, device=dev)
    isum = torch.empty(cells, dtype=torch.int64, device=dev)
    whole = torch.empty(nid, dtype=torch.int64, device=dev)
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)

    def radial(rings, width, wedges):
        _clx.call("clx_region_radial", _clx.ptr(lab), _clx.ptr(dist), _clx.ptr(raw), _RAW_F32, 2, 1, size, size, nid, _clx.ptr(ins),
                  _clx.ptr(row), nrows, rings, width, wedges, shift, _clx.ptr(count), _clx.ptr(isum), _clx.ptr(bad), st)

    def intensity():
        _clx.call("clx_region_intensity", _clx.ptr(lab), _clx.ptr(raw), _RAW_F32, npix, nid, shift, _clx.ptr(whole), _clx.ptr(vkey),
                  _clx.ptr(bad), st)

    # faster and different is not faster: every setting against the restatement, and its sums against the yardstick's
    dist_h, ins_h = dist.cpu().numpy(), ins.cpu().numpy()
    intensity()
    whole_h = whole.cpu().numpy()
    host_s = {}
    for leg, rings, width, wedges in SETTINGS:
        radial(rings, width, wedges)
        torch.cuda.synchronize()
        n = nrows * rings * wedges
        got_count, got_isum = (t[:n].cpu().numpy().reshape(nrows, rings, wedges) for t in (count, isum))
        assert int(bad.item()) == 0
        t0 = time.perf_counter()
        want_count, want_isum, want_bad = ref_radial(labels_h, dist_h, raw_h, nid, ins_h, row_h, nrows, rings, width, wedges, shift)
        host_s[leg] = time.perf_counter() - t0
        assert want_bad == 0 and np.array_equal(got_count, want_count) and np.array_equal(got_isum, want_isum), f"{leg} differs"
        assert np.array_equal(got_isum.sum(axis=(1, 2)), whole_h[1:]), f"{leg}: the sums differ from clx_region_intensity's"

    legs = {f"clx_region_radial, {leg}": (lambda r=rings, w=width, o=wedges: radial(r, w, o)) for leg, rings, width, wedges in SETTINGS}
    legs["clx_region_intensity"] = intensity
    times = time_legs(legs, rounds, {k: 10 for k in legs})
    emit(f"{name}: {size} x {size}, {nobj} object{'s' if nobj > 1 else ''}, {int((labels_h == 0).sum()) / npix:.0%} background, "
         f"edge = {int(edge)}, float32 raw; {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    y = (min(times["clx_region_intensity"]), max(times["clx_region_intensity"]))
    for leg, ts in times.items():
        lo, hi = min(ts), max(ts)
        nbytes = npix * 4 * (2 if leg == "clx_region_intensity" else 3)
        line = f"  {leg:58s} {lo:9.4f} ({hi:9.4f}) ms  {nbytes / (lo * 1e-3) / 1e12:5.2f} TB/s of map bytes"
        if leg != "clx_region_intensity":
            line += f"  {lo / y[0]:5.2f}x clx_region_intensity (worst round against its best: {hi / y[0]:.2f}x)"
            line += f", host / device {host_s[leg[len('clx_region_radial, '):]] * 1e3 / lo:.0f}x"
        emit(line)
    emit("  NumPy restatement (host, one run each): " + ", ".join(f"{s * 1e3:.0f} ms" for s in host_s.values()))
    emit("")


def count_cells(size, emit):
    """What the kernel's tables see on the two object maps, counted on the host from the restatement (no device): the adds to a
    block's table (one per run of uniform lanes inside a wave, one per group of equal cell in another lane) and the distinct
    cells of a block (MAX_GRID = 1024 blocks of consecutive tiles) against its 1024 slots"""
    from radial_ref import ref_distance_sq, ref_inscribed, ref_rings, ref_wedge

    discs, nobj = disc_map(size)
    emit(f"host count, {size} x {size}, {nobj} objects: what the block tables of clx_region_radial see (relative rings)")
    for name, lab in (("discs", discs), ("touching", touching_map(discs))):
        dist = ref_distance_sq(lab, 0)
        ins, _ = ref_inscribed(lab, dist, nobj + 1)
        flat, d = lab.reshape(-1).astype(np.int64), dist.reshape(-1)
        keep = np.flatnonzero(flat > 0)
        for rings, wedges in ((4, 1), (4, 8), (32, 8)):
            ring = ref_rings(d[keep], ins[flat[keep], 0], rings, 0)
            c = ins[flat[keep], 1]
            wedge = ref_wedge(keep // size - c // size, keep % size - c % size) if wedges == 8 else 0
            cell = np.full(flat.size, -1, dtype=np.int64)
            cell[keep] = ((flat[keep] - 1) * rings + ring) * wedges + wedge
            lanes = cell.reshape(-1, 4)
            first = lanes[:, 0]
            uni = (first >= 0) & (lanes == lanes[:, :1]).all(axis=1)
            continues = np.r_[False, (first[1:] == first[:-1]) & uni[:-1]] & uni & (np.arange(len(first)) % 64 != 0)
            other = lanes[~uni]
            groups = (other[:, 0] >= 0).astype(np.int64) + ((other[:, 1:] != other[:, :-1]) & (other[:, 1:] >= 0)).sum(axis=1)
            adds = int((uni & ~continues).sum()) + int(groups.sum())
            distinct = np.array([len(np.unique(b[b >= 0])) for b in cell.reshape(1024, -1)])
            emit(f"  {name:9s} {rings:2d} rings x {wedges} wedges: {len(keep)} object pixels, {adds} adds ({len(keep) / adds:.2f} pixels an add), "
                 f"{uni.mean():.1%} uniform lanes, distinct cells a block: mean {distinct.mean():.0f}, max {distinct.max()}, "
                 f"{int((distinct > 1024).sum())} of 1024 blocks above 1024 slots")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--cells", action="store_true", help="count on the host what the block tables see (no device, no timing); appends to --out")
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    if args.cells:
        assert args.size * args.size % (1024 * 1024) == 0, "the count cuts the map into 1024 blocks of whole tiles"
        count_cells(args.size, emit)
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        raise SystemExit(0)
    if not torch.cuda.is_available():
        raise SystemExit("bench_radial needs a HIP device")
    emit(f"device: {torch.cuda.get_device_name(0)}")
    labels, nobj = disc_map(args.size)
    bench("discs", labels, nobj, False, args.rounds, emit)
    bench("touching (the discs grown until no background is left)", touching_map(labels), nobj, False, args.rounds, emit)
    bench("one object", np.ones((args.size, args.size), np.int32), 1, True, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
