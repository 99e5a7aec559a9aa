"""Times the measure stage's boundary kernels (clx_region_contacts, clx_region_perimeter) against the same counts
written with torch ops on the device (what a user can do today without them), on the inference benchmark's geometry:
discs of radius 12 on a jittered grid, 4096^2 (6 400 objects) and 512^2, as in tools/bench_measure.py.
  torch contacts   the map padded with a ring of zeros, compared with itself shifted along y and along x, the differing
                   pairs as (min << 32) | max, torch.unique with counts
  torch perimeter  border = object pixel with a 4-neighbour of another id; the eight neighbour comparisons on the border
                   map; class by code; torch.bincount per class over the ids of the border pixels
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  Two more label maps of the
same size separate reading from emitting: an all-background map (nothing to emit: loads, comparisons, ballots only) and
a map that is one object (faces along the image edge only).
A kernel leg is 10 calls one after the other on the same 67 MB map, which fits in the 256 MB Infinity Cache: after the
first call the reads need not reach HBM.  The "of the HBM peak" column is algorithmic bytes over time, set against the
HBM peak as a yardstick; it is not measured HBM traffic (no counters are taken here).  tools/bench_measure.py does the same.

    python tools/bench_contacts.py [--out FILE] [--rounds 5]
"""
import argparse
import os
import sys

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
    capacity = _pair_capacity(nobj)                      # what contact_pairs picks
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    counts = torch.empty(capacity, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    classes = torch.empty((nid, 4), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    t_out = {}
    groups = [torch.tensor(g, device=dev) for g in ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))]      # codes of a weight

    def contacts(m=lab):
        _clx.call("clx_region_contacts", _clx.ptr(m), 2, 1, size, size, nid, capacity, _clx.ptr(keys), _clx.ptr(counts),
                  _clx.ptr(info), st)

    def perimeter(m=lab):
        _clx.call("clx_region_perimeter", _clx.ptr(m), size, size, nid, _clx.ptr(classes), _clx.ptr(bad), st)

    def torch_contacts():
        p = torch.nn.functional.pad(lab.long(), (1, 1, 1, 1))
        found = []
        for lo, hi in ((p[:-1], p[1:]), (p[:, :-1], p[:, 1:])):
            differ = lo != hi
            a, b = lo[differ], hi[differ]
            found.append((torch.minimum(a, b) << 32) | torch.maximum(a, b))
        t_out["keys"], t_out["counts"] = torch.unique(torch.cat(found), return_counts=True)

    def torch_perimeter():
        p = torch.nn.functional.pad(lab, (1, 1, 1, 1))
        c = p[1:-1, 1:-1]
        border = (c > 0) & ((p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c))
        q = torch.nn.functional.pad(torch.where(border, c, torch.zeros_like(c)), (1, 1, 1, 1))
        c = q[1:-1, 1:-1]
        n4 = ((q[:-2, 1:-1] == c).int() + (q[2:, 1:-1] == c).int() + (q[1:-1, :-2] == c).int() + (q[1:-1, 2:] == c).int())
        nd = ((q[:-2, :-2] == c).int() + (q[:-2, 2:] == c).int() + (q[2:, :-2] == c).int() + (q[2:, 2:] == c).int())
        code = 1 + 2 * n4 + 10 * nd
        ids = c[border].long()
        code = code[border]
        cols = [torch.bincount(ids, minlength=nid)]
        for group in groups:
            cols.append(torch.bincount(ids[torch.isin(code, group)], minlength=nid))
        t_out["classes"] = torch.stack(cols, dim=1)

    import time
    for name, fn in (("clx_region_contacts", contacts), ("clx_region_perimeter", perimeter), ("torch contacts", torch_contacts),
                     ("torch perimeter", torch_perimeter)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        emit(f"{size} x {size}: first call of {name}: {(time.perf_counter() - t0) * 1e3:.1f} ms (host clock, includes set-up)")
    # faster and different is not faster: the same pairs, counts and classes as the torch formulation
    flags, used = info.tolist()
    assert flags == 0 and int(bad.item()) == 0
    slot = torch.nonzero(keys).reshape(-1)
    order = torch.argsort(keys[slot])
    assert used == len(t_out["keys"]) and torch.equal(keys[slot][order], t_out["keys"])
    assert torch.equal(counts[slot][order], t_out["counts"])
    assert torch.equal(classes[1:], t_out["classes"][1:])
    faces = int(t_out["counts"].sum())

    legs = {"clx_region_contacts": contacts, "clx_region_perimeter": perimeter, "torch contacts": torch_contacts,
            "torch perimeter": torch_perimeter}
    for name, m in maps.items():
        if name != "discs":
            legs[f"clx_region_contacts, {name}"] = lambda m=m: contacts(m)
            legs[f"clx_region_perimeter, {name}"] = lambda m=m: perimeter(m)
    reps = {k: (1 if k.startswith("torch") else 10) for k in legs}
    times = time_legs(legs, rounds, reps)

    emit(f"{size} x {size}, {nobj} objects, {used} pairs, {faces} faces, table of {capacity} slots; {rounds} rounds, legs "
         "alternating; ms per call: min (max) of the rounds")
    best = {}
    for name, ts in times.items():
        lo, hi = min(ts), max(ts)
        best[name] = (lo, hi)
        line = f"  {name:48s} {lo:9.4f} ({hi:9.4f}) ms"
        if name.startswith("clx"):
            # the label map once; the contacts call also clears its table (keys and counts, 16 bytes a slot)
            nbytes = npix * 4 + (capacity * 16 if "contacts" in name else nid * 32)
            tbs = nbytes / (lo * 1e-3) / 1e12
            line += f"   {nbytes / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {tbs / PEAK_TBS:4.2f} of the {PEAK_TBS:.0f} TB/s HBM peak"
        emit(line)
    for kernel, formulation in (("clx_region_contacts", "torch contacts"), ("clx_region_perimeter", "torch perimeter")):
        (klo, khi), (tlo, thi) = best[kernel], best[formulation]
        emit(f"  {formulation} / {kernel}: {tlo / klo:.1f}x (worst round of the kernel against the best of torch: {tlo / khi:.1f}x)")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 512])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contacts needs a HIP device")
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
