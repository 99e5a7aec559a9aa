"""Times the measure stage's sums of products (clx_region_products: the twenty words per object behind the intensity standard
deviation and the colocalization columns) beside the yardstick: clx_region_intensity called once per channel on the same map,
code of the same reading frame that streams 16 bytes a pixel (labels and one float32 channel, twice) where clx_region_products
streams 12 (labels and both channels, once), and keeps one 64-bit sum and two keys per id where this keeps twenty words.
Maps at 4096^2: tools/bench_measure.py's discs of radius 12 on a jittered grid (6 400 objects), tools/bench_inscribed.py's
"touching" map (the discs grown until no background is left), and ONE object that fills the map, the contention case: every
run of every block lands in the same slot.  The channels are float32 holding integers below 256 at shift 0, so that the int64
restatement of tests/coloc_ref.py is exact; the kernel does the same work whatever the values are.
HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  Before anything is timed every
leg's table is compared with the restatement, and its sums with the yardstick's.

    python tools/bench_coloc.py [--out FILE] [--rounds 5]
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
from coloc_ref import NW, ref_products, words_of  # noqa: E402

_RAW_F32 = 0
YARDSTICK = "clx_region_intensity, once per channel"


def bench(name, labels_h, nobj, rounds, emit):
    size = labels_h.shape[0]
    npix = labels_h.size
    nid = nobj + 1
    rng = np.random.default_rng(0)
    a_h = rng.integers(0, 256, size=(size, size)).astype(np.float32)
    b_h = np.clip(a_h * 0.5 + rng.integers(0, 128, size=(size, size)), 0, 255).astype(np.float32)
    thr_a_h = rng.integers(20, 60, size=nid).astype(np.int64)
    thr_b_h = rng.integers(20, 60, size=nid).astype(np.int64)
    lab, a, b = (torch.from_numpy(v).to(dev) for v in (labels_h, a_h, b_h))
    thr_a, thr_b = (torch.from_numpy(v).to(dev) for v in (thr_a_h, thr_b_h))
    st = _clx.stream_ptr(dev)
    out = torch.empty((nid, NW), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    whole = [torch.empty(nid, dtype=torch.int64, device=dev) for _ in range(2)]
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)

    def products(x, y, ta, tb):
        _clx.call("clx_region_products", _clx.ptr(lab), _clx.ptr(x), _clx.ptr(y), _RAW_F32, npix, nid, 0, 0, _clx.ptr(ta), _clx.ptr(tb),
                  _clx.ptr(out), _clx.ptr(bad), st)

    def intensity():
        for raw, isum in zip((a, b), whole):
            _clx.call("clx_region_intensity", _clx.ptr(lab), _clx.ptr(raw), _RAW_F32, npix, nid, 0, _clx.ptr(isum), _clx.ptr(vkey),
                      _clx.ptr(bad), st)

    settings = (("channels a, b, no thresholds", a, b, None, None, a_h, b_h, None, None),
                ("channels a, b, per-object thresholds", a, b, thr_a, thr_b, a_h, b_h, thr_a_h, thr_b_h),
                ("a == b, no thresholds (the std alone)", a, a, None, None, a_h, a_h, None, None))
    # faster and different is not faster: every leg against the restatement, and its sums against the yardstick's
    intensity()
    whole_h = [w.cpu().numpy() for w in whole]
    host_s = 0.0
    for leg, x, y, ta, tb, xh, yh, tah, tbh in settings:
        products(x, y, ta, tb)
        torch.cuda.synchronize()
        assert int(bad.item()) == 0
        got = out.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        rows, want_bad = ref_products(labels_h, xh, yh, nid, 0, 0, tah, tbh, small=True)
        host_s = time.perf_counter() - t0
        assert want_bad == 0 and np.array_equal(got[1:], words_of(rows)[1:]), f"{leg} differs from the restatement"
        assert np.array_equal(got[1:, 1].view(np.int64), whole_h[0][1:]), f"{leg}: Σa differs from clx_region_intensity's"
        if y is b:
            assert np.array_equal(got[1:, 2].view(np.int64), whole_h[1][1:]), f"{leg}: Σb differs from clx_region_intensity's"

    legs = {f"clx_region_products, {s[0]}": (lambda s=s: products(s[1], s[2], s[3], s[4])) for s in settings}
    legs[YARDSTICK] = intensity
    times = time_legs(legs, rounds, {k: 10 for k in legs})
    emit(f"{name}: {size} x {size}, {nobj} object{'s' if nobj > 1 else ''}, {int((labels_h == 0).sum()) / npix:.0%} background, "
         f"float32 channels; {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    y0 = min(times[YARDSTICK])
    for leg, ts in times.items():
        lo, hi = min(ts), max(ts)
        nbytes = npix * 4 * (4 if leg == YARDSTICK else 3)
        line = f"  {leg:62s} {lo:9.4f} ({hi:9.4f}) ms  {nbytes / (lo * 1e-3) / 1e12:5.2f} TB/s of map bytes"
        if leg != YARDSTICK:
            line += f"  {lo / y0:5.2f}x the yardstick (worst round against its best: {hi / y0:.2f}x)"
        emit(line)
    emit(f"  int64 NumPy restatement (host, one run): {host_s * 1e3:.0f} ms")
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
        raise SystemExit("bench_coloc needs a HIP device")
    emit(f"device: {torch.cuda.get_device_name(0)}")
    labels, nobj = disc_map(args.size)
    bench("discs", labels, nobj, args.rounds, emit)
    bench("touching (the discs grown until no background is left)", touching_map(labels), nobj, args.rounds, emit)
    bench("one object", np.ones((args.size, args.size), np.int32), 1, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
