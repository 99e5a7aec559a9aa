"""Times the expand stage's nearest-object map (cellulus_amd.expand.nearest_object -> clx_label_nearest, 2-D) without a limit
and with limit = 8, beside what a user does on the host today: scipy.ndimage.distance_transform_edt(labels == 0,
return_indices=True) of the same map.  Map: tools/bench_measure.py's jittered discs, 2048^2 with about 2 000 of them.
nearest_object is timed as a user calls it, on a device tensor and on the host clock around a device synchronise (its range
check of the labels and its allocations included); the library call alone with HIP events.  Warm-up, then the median (min,
max) of the repeats.  Before anything is timed the device maps are compared with scipy's distances everywhere and with its
indices wherever one object is nearest.  The algorithmic bytes of the three passes are computed from the shape.

    python tools/bench_nearest.py [--out FILE] [--repeats 20] [--size 2048]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_measure import dev, disc_map  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.expand import nearest_object  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s (specification)
# pass X reads the labels (4) and writes a key (8); pass Y reads every pixel's own key (8) and writes one (8); the taps of the
# outward search are re-reads of keys other threads read as their own: they are not counted
BYTES_PER_PIXEL_2D = 4 + 8 + 8 + 8


def summary(ms):
    return f"{statistics.median(ms):9.4f} ({min(ms):9.4f} .. {max(ms):9.4f}) ms"


def bench(size, repeats, emit):
    labels_h, nobj = disc_map(size, spacing=46, radius=10, jitter=5)
    npix, nid = labels_h.size, nobj + 1
    lab = torch.from_numpy(labels_h).to(dev)
    st, lib = _clx.stream_ptr(dev), _clx.load()
    nearest = torch.empty(npix, dtype=torch.int32, device=dev)
    dist = torch.empty(npix, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = int(lib.clx_label_nearest_workspace(npix))
    work = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)

    t0 = time.perf_counter()
    edt, indices = ndimage.distance_transform_edt(labels_h == 0, return_indices=True)
    host_s = time.perf_counter() - t0
    want_d2 = np.rint(edt * edt).astype(np.int64)
    theirs = labels_h[tuple(indices)]
    got, got_d2 = (t.cpu().numpy() for t in nearest_object(lab))
    assert np.array_equal(got_d2, want_d2), "nearest_object's distances differ from scipy's"
    differ = got != theirs
    assert (got[differ] < theirs[differ]).all() and differ.mean() < 0.01, "nearest_object's ids differ from scipy's beyond ties"
    limited, limited_d2 = (t.cpu().numpy() for t in nearest_object(lab, 8))
    inside = want_d2 <= 64
    assert np.array_equal(limited[inside], got[inside]) and np.array_equal(limited_d2[inside], got_d2[inside]) and not limited[~inside].any()

    emit(f"discs: {size} x {size}, {nobj} objects, {int((labels_h == 0).sum()) / npix:.0%} background, farthest pixel "
         f"{float(np.sqrt(got_d2.max())):.1f} from an object, ties {differ.mean():.2%} of the pixels differ from scipy's choice; "
         f"{repeats} repeats: median (min .. max)")
    for name, limit, limit_sq in (("no limit", None, -1), ("limit = 8", 8, 64)):
        def call():
            _clx.call("clx_label_nearest", _clx.ptr(lab), 2, 1, size, size, nid, limit_sq, _clx.ptr(nearest), _clx.ptr(dist), _clx.ptr(bad),
                      _clx.ptr(work), nbytes, st)

        for _ in range(3):
            nearest_object(lab, limit)
            call()
        torch.cuda.synchronize()
        whole, kernel = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            nearest_object(lab, limit)
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1))
        floor_ms = npix * BYTES_PER_PIXEL_2D / HBM_PEAK * 1e3
        emit(f"  nearest_object, {name:10s} (host clock, synchronised)   {summary(whole)}")
        emit(f"  clx_label_nearest, {name:10s} (HIP events)              {summary(kernel)}: {BYTES_PER_PIXEL_2D} algorithmic bytes a pixel "
             f"are {floor_ms:.4f} ms at the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s, {floor_ms / statistics.median(kernel):.1%} of the time")
        emit(f"  scipy distance_transform_edt(return_indices=True) (host, one run) {host_s * 1e3:9.1f} ms: "
             f"{host_s * 1e3 / statistics.median(whole):.0f}x nearest_object")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nearest needs a HIP device")
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
