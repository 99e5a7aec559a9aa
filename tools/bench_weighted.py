"""Times the measure stage's weighted moments (clx_region_weighted: the 21 words per object behind the weighted centroid, the
weighted covariance, the mass displacement and the peak position) and its border intensity (clx_region_border_intensity: the
seven words per object over the rim) beside two yardsticks of the same reading frame on the same map in the same run:
clx_region_intensity (one 64-bit sum and two keys per id) and clx_region_products with a == b and no thresholds (three 128-bit
sums through the wave where clx_region_weighted carries two and a 64-bit one).  All four read the label map and one float32
channel: 8 bytes a pixel, which is what "TB/s of map bytes" divides by (the border kernel reads the label map up to three
times, from the caches, and the channel along the rims only).
Maps at 4096^2: tools/bench_measure.py's discs of radius 12 on a jittered grid (6 400 objects), tools/bench_inscribed.py's
"touching" map (the discs grown until no background is left), and ONE object that fills the map, the contention case: every
run of every block lands in the same slot.  clx_region_weighted is also timed on the same bytes taken as 16 slices of 256
rows: the same runs, summed in the 21-word table of a 3-D map.  The channel is float32 holding integers below 256 at shift 0,
so that the int64 restatement of tests/weighted_ref.py is exact; the kernels do the same work whatever the values are.
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  Before anything is timed both
tables are compared with the restatement.  For the border kernel the share of waves (256 consecutive pixels) without a border
pixel is counted on the host from the restatement's mask: those are the waves that read no raw value.

    python tools/bench_weighted.py [--out FILE] [--rounds 5]
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
from weighted_ref import NB, NW, border_words, ref_border, ref_border_mask, ref_weighted, weighted_words  # noqa: E402

_RAW_F32 = 0
WEIGHTED, BORDER = "clx_region_weighted", "clx_region_border_intensity (2-D)"
WEIGHTED_3D = "clx_region_weighted, the map as 16 slices (3-D table)"
INTENSITY, PRODUCTS = "clx_region_intensity (yardstick)", "clx_region_products, a == b, no thresholds (yardstick)"
NOTES = """hipcc (gfx950, -O3) reports for the float32 kernels, none of which spills:
  weighted_kernel, 2-D   91 VGPRs, 27648 bytes of LDS (13 words an id): __launch_bounds__(256, 4), 4 blocks a CU in a grid of 1024
  weighted_kernel, 3-D  115 VGPRs, 44032 bytes of LDS (21 words an id): __launch_bounds__(256, 3), 3 blocks a CU, grid of 768
  border_kernel          58 VGPRs, 15360 bytes of LDS: 8 waves a SIMD
  products_kernel (no thresholds) 98 VGPRs, 19456 bytes of LDS: 4 waves a SIMD
clx_region_weighted's first version (one add128 after the other, a call of its own for every piece of a lane on an edge, the
21-word table for 2-D maps too) took 0.193 / 0.222 / 0.131 ms on the three maps, 1.30x / 1.31x / 0.87x the products yardstick;
csrc/region_weighted.hip's header says what was changed.  The peak (the gather of the largest key per id and the atomicMin)
was 5 - 9 % of that version's time, measured by passing peak_keys = NULL.
On the one-object map every block's flush adds to the same words of global memory.  We believe that both new kernels, like
the yardsticks, pay for that contention there and not for their pixels: the border kernel skips 87.5 % of the waves on that
map and is slower than on the other two."""


def bench(name, labels_h, nobj, rounds, emit):
    size = labels_h.shape[0]
    npix = labels_h.size
    nid = nobj + 1
    rng = np.random.default_rng(0)
    a_h = rng.integers(0, 256, size=(size, size)).astype(np.float32)
    lab, a = (torch.from_numpy(v).to(dev) for v in (labels_h, a_h))
    st = _clx.stream_ptr(dev)
    out_w = torch.empty((nid, NW), dtype=torch.int64, device=dev)
    out_b = torch.empty((nid, NB), dtype=torch.int64, device=dev)
    out_p = torch.empty((nid, 20), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    isum = torch.empty(nid, dtype=torch.int64, device=dev)
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)
    keys = torch.empty(nid, dtype=torch.int64, device=dev)

    def intensity():
        _clx.call("clx_region_intensity", _clx.ptr(lab), _clx.ptr(a), _RAW_F32, npix, nid, 0, _clx.ptr(isum), _clx.ptr(vkey), _clx.ptr(bad), st)

    def products():
        _clx.call("clx_region_products", _clx.ptr(lab), _clx.ptr(a), _clx.ptr(a), _RAW_F32, npix, nid, 0, 0, _clx.ptr(None), _clx.ptr(None),
                  _clx.ptr(out_p), _clx.ptr(bad), st)

    def weighted():
        _clx.call("clx_region_weighted", _clx.ptr(lab), _clx.ptr(a), _RAW_F32, 1, size, size, nid, 0, _clx.ptr(keys), _clx.ptr(out_w),
                  _clx.ptr(bad), st)

    def weighted_3d():
        _clx.call("clx_region_weighted", _clx.ptr(lab), _clx.ptr(a), _RAW_F32, 16, size // 16, size, nid, 0, _clx.ptr(keys), _clx.ptr(out_w),
                  _clx.ptr(bad), st)

    def border():
        _clx.call("clx_region_border_intensity", _clx.ptr(lab), _clx.ptr(a), _RAW_F32, 2, 1, size, size, nid, 0, _clx.ptr(out_b),
                  _clx.ptr(bad), st)

    # faster and different is not faster: both tables against the restatement, with the yardstick's largest keys as peak keys
    intensity()
    keys.copy_(vkey[:, 1])
    torch.cuda.synchronize()
    keys_h = keys.cpu().numpy().view(np.uint64)
    weighted()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    t0 = time.perf_counter()
    rows, want_bad = ref_weighted(labels_h, a_h, nid, 0, keys_h, small=True)
    host_s = time.perf_counter() - t0
    got = out_w.cpu().numpy().view(np.uint64)
    assert want_bad == 0 and np.array_equal(got[1:], weighted_words(rows)[1:]), "clx_region_weighted differs from the restatement"
    assert np.array_equal(got[1:, 1].view(np.int64), isum.cpu().numpy()[1:]), "Σq differs from clx_region_intensity's"
    weighted_3d()
    torch.cuda.synchronize()
    rows, want_bad = ref_weighted(labels_h.reshape(16, size // 16, size), a_h, nid, 0, keys_h, small=True)
    assert int(bad.item()) == 0 and want_bad == 0 and np.array_equal(out_w.cpu().numpy().view(np.uint64)[1:], weighted_words(rows)[1:]), \
        "clx_region_weighted differs from the restatement on the 3-D view"
    border()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    rows, want_bad = ref_border(labels_h, a_h, nid, 2, 0, small=True)
    assert want_bad == 0 and np.array_equal(out_b.cpu().numpy().view(np.uint64)[1:], border_words(rows)[1:]), \
        "clx_region_border_intensity differs from the restatement"
    mask = ref_border_mask(labels_h, nid, 2).reshape(-1)
    waves = -(-npix // 256)
    busy = np.zeros(waves * 256, bool)
    busy[:npix] = mask
    skipped = 1.0 - busy.reshape(waves, 256).any(axis=1).mean()

    legs = {WEIGHTED: weighted, WEIGHTED_3D: weighted_3d, BORDER: border, INTENSITY: intensity, PRODUCTS: products}
    times = time_legs(legs, rounds, {k: 10 for k in legs})
    emit(f"{name}: {size} x {size}, {nobj} object{'s' if nobj > 1 else ''}, {int((labels_h == 0).sum()) / npix:.0%} background, "
         f"one float32 channel; {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    yard = {k: min(times[k]) for k in (INTENSITY, PRODUCTS)}
    for leg, ts in times.items():
        lo, hi = min(ts), max(ts)
        line = f"  {leg:56s} {lo:9.4f} ({hi:9.4f}) ms  {npix * 8 / (lo * 1e-3) / 1e12:5.2f} TB/s of map bytes"
        if leg in (WEIGHTED, WEIGHTED_3D, BORDER):
            line += f"  {lo / yard[PRODUCTS]:5.2f}x the products yardstick, {lo / yard[INTENSITY]:5.2f}x the intensity yardstick"
        emit(line)
    emit(f"  border pixels: {int(mask.sum())} of {npix} pixels; waves of 256 pixels that take the interior skip: {skipped:.1%} of {waves}")
    emit(f"  int64 NumPy restatement of the weighted sums (host, one run): {host_s * 1e3:.0f} ms")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    if not torch.cuda.is_available():
        raise SystemExit("bench_weighted needs a HIP device")
    emit(f"device: {torch.cuda.get_device_name(0)}")
    labels, nobj = disc_map(args.size)
    bench("discs", labels, nobj, args.rounds, emit)
    bench("touching (the discs grown until no background is left)", touching_map(labels), nobj, args.rounds, emit)
    bench("one object", np.ones((args.size, args.size), np.int32), 1, args.rounds, emit)
    emit(NOTES)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
