"""Times the measure stage's co-occurrence counts (clx_region_cooccurrence: the four 2-D direction matrices of every object at
pixel distance 1) beside clx_region_intensity on the same arrays, the device yardstick (one pass over labels and raw that keeps
sums and extrema), and beside the NumPy restatement of the same counts on the host (tests/texture_ref.py: shifted views and
np.add.at).  Maps at the inference benchmark's geometry: tools/bench_measure.py's discs of radius 12 on a jittered grid at
4096^2 (6 400 objects of about 450 pixels, one work item each), and the map that is one object everywhere (one box cut into
thousands of slabs that add into one row: the shared-object path).  Raw: float32 noise (the pairs spread over the whole
matrix) and a smooth image (nearly every pair falls on a diagonal cell: the LDS atomics of a wave collide).  8 and 32 levels.
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  The host leg is one run on the
host clock.  Before anything is timed the counts are compared with the restatement's.

    python tools/bench_texture.py [--out FILE] [--rounds 5]
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
from bench_measure import dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure_columns import intensity_shift  # noqa: E402
from cellulus_amd.segment import _RAW_F32  # noqa: E402
from texture_ref import ref_cooccurrence  # noqa: E402


def bench(name, labels_h, nobj, raw_name, raw_h, levels_list, rounds, emit):
    size = labels_h.shape[0]
    npix = labels_h.size
    nid = nobj + 1
    lib = _clx.load()
    st = _clx.stream_ptr(dev)
    lab = torch.from_numpy(labels_h).to(dev)
    raw = torch.from_numpy(raw_h).to(dev)
    area = torch.empty(nid, dtype=torch.int64, device=dev)
    bbox = torch.empty((nid, 6), dtype=torch.int32, device=dev)
    sum1 = torch.empty((nid, 3), dtype=torch.int64, device=dev)
    sum2 = torch.empty((nid, 6), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    _clx.call("clx_region_moments", _clx.ptr(lab), 1, size, size, nid, _clx.ptr(area), _clx.ptr(bbox), _clx.ptr(sum1), _clx.ptr(sum2),
              _clx.ptr(bad), st)
    area_h = area.cpu().numpy()
    area_h[0] = 0
    ids_h = np.flatnonzero(area_h).astype(np.int32)
    nrows = len(ids_h)
    ids = torch.from_numpy(ids_h).to(dev)
    lo, hi = float(raw_h[labels_h > 0].min()), float(raw_h[labels_h > 0].max())
    nbytes = int(lib.clx_region_cooccurrence_workspace(npix, nrows))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    seen = torch.empty(nrows, dtype=torch.int64, device=dev)
    isum = torch.empty(nid, dtype=torch.int64, device=dev)
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)
    shift = intensity_shift(float(np.abs(raw_h).max()), npix)
    counts = {L: torch.empty((nrows, 4, L, L), dtype=torch.int32, device=dev) for L in levels_list}

    def cooccurrence(L):
        _clx.call("clx_region_cooccurrence", _clx.ptr(lab), _clx.ptr(raw), _RAW_F32, 2, 1, size, size, nid, _clx.ptr(bbox), _clx.ptr(ids),
                  nrows, lo, hi, L, 1, _clx.ptr(counts[L]), _clx.ptr(seen), _clx.ptr(bad), _clx.ptr(work), nbytes, st)

    def intensity():
        _clx.call("clx_region_intensity", _clx.ptr(lab), _clx.ptr(raw), _RAW_F32, npix, nid, shift, _clx.ptr(isum), _clx.ptr(vkey),
                  _clx.ptr(bad), st)

    # faster and different is not faster: the counts against the restatement, whose run is the host leg
    host_s, diagonal = {}, {}
    for L in levels_list:
        t0 = time.perf_counter()
        want = ref_cooccurrence(labels_h, raw_h, nid, ids_h, lo, hi, L, 1)
        host_s[L] = time.perf_counter() - t0
        cooccurrence(L)
        torch.cuda.synchronize()
        got = counts[L].cpu().numpy()
        assert int(bad.item()) == 0 and np.array_equal(seen.cpu().numpy(), area_h[ids_h])
        assert np.array_equal(got, want["counts"]), "clx_region_cooccurrence differs from the restatement"
        total = int(got.sum())
        diagonal[L] = (int(np.trace(got.sum(axis=(0, 1)))) / total, total)

    legs = {f"clx_region_cooccurrence, {L} levels": (lambda L=L: cooccurrence(L)) for L in levels_list}
    legs["clx_region_intensity"] = intensity
    times = time_legs(legs, rounds, {k: 10 for k in legs})
    best = {leg: (min(ts), max(ts)) for leg, ts in times.items()}
    a = area_h[ids_h]
    emit(f"{name}, {raw_name}: {size} x {size}, {nrows} objects, {int(a.sum()) / npix:.0%} object pixels, largest object {int(a.max())} "
         f"pixels; 4 directions at distance 1; {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    for leg, (lo_ms, hi_ms) in best.items():
        emit(f"  {leg:44s} {lo_ms:9.4f} ({hi_ms:9.4f}) ms")
    y = best["clx_region_intensity"]
    for L in levels_list:
        w = best[f"clx_region_cooccurrence, {L} levels"]
        share, total = diagonal[L]
        emit(f"  {L:2d} levels: {total} pairs, {share:.1%} of them on the diagonal; the counts table is {nrows * 4 * L * L * 4 / 1e6:.1f} MB; "
             f"restatement on the host (one run) {host_s[L] * 1e3:.0f} ms")
        emit(f"             clx_region_cooccurrence / clx_region_intensity: {w[0] / y[0]:.2f}x (worst round against the yardstick's "
             f"best: {w[1] / y[0]:.2f}x); host / clx_region_cooccurrence: {host_s[L] * 1e3 / w[0]:.0f}x")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--levels", type=int, nargs="+", default=[8, 32])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    size = args.size
    rng = np.random.default_rng(0)
    noise = (rng.random((size, size), dtype=np.float32) * 1000.0).astype(np.float32)
    yy, xx = np.indices((size, size), dtype=np.float32)
    smooth = (np.float32(1000.0 / (2 * size)) * (yy + xx)).astype(np.float32)      # a ramp: neighbours differ by 1/8 of a level at 32
    emit(f"device: {torch.cuda.get_device_name(0)}")
    labels, nobj = disc_map(size)
    one = np.ones((size, size), np.int32)
    bench("discs", labels, nobj, "float32 noise", noise, args.levels, args.rounds, emit)
    bench("discs", labels, nobj, "float32 smooth ramp", smooth, args.levels, args.rounds, emit)
    bench("one object everywhere", one, 1, "float32 noise", noise, args.levels, args.rounds, emit)
    bench("one object everywhere", one, 1, "float32 smooth ramp", smooth, args.levels, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
