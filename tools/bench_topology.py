"""Times the measure stage's topology kernel (clx_region_topology) beside clx_region_contacts (the same reads in the same
frame: own pixels, the row below, a ballot; its table of pairs instead of the table of ids) and against the same five
counts written with torch ops on the device (what a user can do today without it), on the inference benchmark's
geometry: discs of radius 12 on a jittered grid, 4096^2 (6 400 objects) and 512^2, as in tools/bench_contacts.py.
  torch topology   the map padded with a ring of zeros and its four shifted views (the voxels of every 2 x 2 window); a
                   voxel pair with different values adds to both values' ids (torch.bincount); a cell through the vertex
                   adds to every distinct id among its voxels (E_hi: torch.sort along the voxels) or to the one id all
                   its voxels carry (E_lo)
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  Two more label maps of the
same size separate reading from accumulating: an all-background map (loads, comparisons, ballots only) and a map that is
one object (windows along the image edge only).
A kernel leg is 10 calls one after the other on the same 67 MB map, which fits in the 256 MB Infinity Cache: after the
first call the reads need not reach HBM.  The "of the HBM peak" column is algorithmic bytes over time, set against the
HBM peak as a yardstick; it is not measured HBM traffic (no counters are taken here).

    python tools/bench_topology.py [--out FILE] [--rounds 5]
"""
import argparse
import itertools
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_measure import PEAK_TBS, dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure import _pair_capacity  # noqa: E402


def bench(size, rounds, emit):
    labels_h, nobj = disc_map(size)
    nid = nobj + 1
    npix = size * size
    lab = torch.from_numpy(labels_h).to(dev)
    maps = {"discs": lab, "background": torch.zeros_like(lab), "one object": torch.ones_like(lab)}
    st = _clx.stream_ptr(dev)
    capacity = _pair_capacity(nobj)
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    pair_counts = torch.empty(capacity, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    counts = torch.empty((nid, 5), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    t_out = {}

    def topology(m=lab):
        _clx.call("clx_region_topology", _clx.ptr(m), 2, 1, size, size, nid, _clx.ptr(counts), _clx.ptr(bad), st)

    def contacts(m=lab):
        _clx.call("clx_region_contacts", _clx.ptr(m), 2, 1, size, size, nid, capacity, _clx.ptr(keys), _clx.ptr(pair_counts),
                  _clx.ptr(info), st)

    def torch_topology():
        p = torch.nn.functional.pad(lab.long(), (1, 1, 1, 1))
        v = [p[dy:dy + size + 1, dx:dx + size + 1] for dy, dx in itertools.product((0, 1), repeat=2)]
        out = torch.zeros((nid, 5), dtype=torch.int64, device=dev)

        def add(column, ids, weight=1):
            out[:, column] += weight * torch.bincount(ids[ids > 0], minlength=nid)

        for a, b in itertools.combinations(range(4), 2):
            differ = v[a] != v[b]
            k = 2 if a ^ b == 3 else 1                   # the diagonal pairs are (0, 3) and (1, 2)
            add(k - 1, v[a][differ])
            add(k - 1, v[b][differ])
        cells = [(0, [0, 1, 2, 3]), (1, [0, 1]), (1, [2, 3]), (1, [0, 2]), (1, [1, 3]), (2, [0]), (2, [1]), (2, [2]), (2, [3])]
        for d, members in cells:
            w = 1 << (2 - d)
            s = torch.sort(torch.stack([v[n] for n in members], dim=-1), dim=-1).values
            add(3, s[..., 0].reshape(-1), (-1) ** d * w)
            for j in range(1, len(members)):
                add(3, s[..., j][s[..., j] != s[..., j - 1]], (-1) ** d * w)
            add(4, s[..., 0][s[..., 0] == s[..., -1]], (-1) ** (2 - d) * w)
        t_out["counts"] = out

    for name, fn in (("clx_region_topology", topology), ("clx_region_contacts", contacts), ("torch topology", torch_topology)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        emit(f"{size} x {size}: first call of {name}: {(time.perf_counter() - t0) * 1e3:.1f} ms (host clock, includes set-up)")
    # faster and different is not faster: the same counts as the torch formulation
    assert int(bad.item()) == 0 and info.tolist()[0] == 0
    assert torch.equal(counts[1:], t_out["counts"][1:])
    faces = int(counts[1:, 0].sum()) // 2
    holes = int((counts[1:, 3] != 4).sum())

    legs = {"clx_region_topology": topology, "clx_region_contacts": contacts, "torch topology": torch_topology}
    for name, m in maps.items():
        if name != "discs":
            legs[f"clx_region_topology, {name}"] = lambda m=m: topology(m)
            legs[f"clx_region_contacts, {name}"] = lambda m=m: contacts(m)
    reps = {k: (1 if k.startswith("torch") else 10) for k in legs}
    times = time_legs(legs, rounds, reps)

    emit(f"{size} x {size}, {nobj} objects, {faces} boundary faces, {holes} objects with an Euler number other than 1; {rounds} "
         "rounds, legs alternating; ms per call: min (max) of the rounds")
    best = {}
    for name, ts in times.items():
        lo, hi = min(ts), max(ts)
        best[name] = (lo, hi)
        line = f"  {name:48s} {lo:9.4f} ({hi:9.4f}) ms"
        if name.startswith("clx"):
            # the label map once; the calls also clear their outputs (40 bytes an id; keys and counts, 16 bytes a slot)
            nbytes = npix * 4 + (capacity * 16 if "contacts" in name else nid * 40)
            tbs = nbytes / (lo * 1e-3) / 1e12
            line += f"   {nbytes / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {tbs / PEAK_TBS:4.2f} of the {PEAK_TBS:.0f} TB/s HBM peak"
        emit(line)
    (klo, khi), (tlo, thi) = best["clx_region_topology"], best["torch topology"]
    emit(f"  torch topology / clx_region_topology: {tlo / klo:.1f}x (worst round of the kernel against the best of torch: {tlo / khi:.1f}x)")
    for name in maps:
        suffix = "" if name == "discs" else f", {name}"
        t, c = best["clx_region_topology" + suffix][0], best["clx_region_contacts" + suffix][0]
        emit(f"  clx_region_topology / clx_region_contacts, {name}: {t / c:.2f}x")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 512])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topology needs a HIP device")
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
