"""Times the skeleton stage's thinning kernel (cellulus_amd.skeleton -> clx_label_thin, 2-D) on one workload: the territories of
tools/bench_propagate.py on 2048^2 (its 2 025 seeds grown inside its mask along its membrane image), objects some 40 pixels
wide.  Warm-up, then the median (min .. max) of the repeats with HIP events.  Timed: thin_labels() to the fixed point as a user
calls it (the host reads info between the calls); the same iterations queued through the C ABI without a host read, with 64
iterations a call (launches of 8 iterations, 16 sub-iterations on chip) and with ONE iteration a call (launches of one
iteration: what a kernel without the on-chip steps would do, plus the call's clearing, finish and output pass, which a call
that runs nothing measures).  Two yardsticks beside the times: the time a sub-iteration would take at the HBM peak if it read
the nine bit planes and wrote one, and clx_label_distance_sq on the same map in the same run, for scale and not a target.
Before anything is timed the device map is compared with the restatement of tests/skeleton_ref.py on a 512^2 crop.

    python tools/bench_skeleton.py [--out FILE] [--repeats 20] [--size 2048]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bench_measure import dev, disc_map  # noqa: E402
from bench_propagate import membrane  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.expand import expand_labels, nearest_object  # noqa: E402
from cellulus_amd.propagate import geodesic_owner  # noqa: E402
from cellulus_amd.skeleton import thin_labels  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s (specification)
PLANES = 10                             # bit planes a sub-iteration would move: nine read, one written


def summary(ms):
    return f"{statistics.median(ms):9.4f} ({min(ms):9.4f} .. {max(ms):9.4f}) ms"


def workload(size):
    labels_h, nobj = disc_map(size, spacing=46, radius=10, jitter=5)
    seeds = torch.from_numpy(labels_h).to(dev)
    mask = (expand_labels(seeds, 20) > 0).to(torch.uint8).contiguous()
    weight = membrane(nearest_object(seeds)[0]).contiguous()
    return geodesic_owner(seeds, mask, weight)[0].cpu().numpy().astype(np.int32), nobj


def timed(run, repeats):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def bench(size, repeats, emit):
    labels_h, nobj = workload(size)
    npix = labels_h.size
    labels = torch.from_numpy(labels_h).to(dev).reshape(-1)
    st, lib = _clx.stream_ptr(dev), _clx.load()

    from skeleton_ref import skeleton

    crop = np.ascontiguousarray(labels_h[:512, :512])
    assert np.array_equal(thin_labels(crop, device=dev), skeleton(crop)), "thin_labels differs from the restatement on the crop"

    out = torch.empty(npix, dtype=torch.int32, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    nbytes = int(lib.clx_label_thin_workspace(2, 1, size, size))
    work = torch.empty(max(nbytes, int(lib.clx_label_distance_workspace(npix))) // 4 + 2, dtype=torch.int32, device=dev)

    def call(iterations, resume):
        _clx.call("clx_label_thin", _clx.ptr(labels), 2, 1, size, size, iterations, resume, _clx.ptr(out), _clx.ptr(info), _clx.ptr(work),
                  nbytes, st)

    # the iterations to the fixed point, the last of which deletes nothing: one iteration a call, info read after each
    total, deleted = 0, 0
    while True:
        call(1, int(total > 0))
        total += 1
        found = info.tolist()
        deleted += found[2]
        if found[1] == 0:
            break
    skeleton_pixels = int((out != 0).sum().item())
    assert deleted == int((labels_h != 0).sum()) - skeleton_pixels
    launches = -(-total // 8)

    def queued(per_call):
        done = 0
        while done < total:
            n = min(per_call, total - done)
            call(n, int(done > 0))
            done += n

    def distance():
        _clx.call("clx_label_distance_sq", _clx.ptr(labels), 2, 1, size, size, 0, _clx.ptr(out), _clx.ptr(work),
                  int(lib.clx_label_distance_workspace(npix)), st)

    def idle():                         # a call after the fixed point: its launch returns at once; clearing, finish, output pass
        call(1, 1)

    emit(f"territories: {size} x {size}, {nobj} objects, {int((labels_h > 0).sum()) / npix:.0%} of the pixels; the fixed point after {total} "
         f"iterations = {2 * total} sub-iterations (the last iteration deletes nothing), {deleted} pixels deleted, {skeleton_pixels} left; "
         f"{repeats} repeats: median (min .. max)")
    rows = (("thin_labels() to the fixed point, host loop", lambda: thin_labels(labels.reshape(size, size))),
            (f"clx_label_thin, 64 iterations a call: {launches} launches", lambda: queued(64)),
            (f"clx_label_thin, 1 iteration a call: {total} launches", lambda: queued(1)),
            ("clx_label_thin, a call that runs nothing", lambda: (queued(64), [idle() for _ in range(10)])),
            ("clx_label_distance_sq", distance))
    times = {}
    for name, run in rows:
        ms = timed(run, repeats)
        times[name] = statistics.median(ms)
        emit(f"  {name:52s} (HIP events) {summary(ms)}")
    multi, single, idle10 = (times[rows[k][0]] for k in (1, 2, 3))
    idle_ms = (idle10 - multi) / 10
    floor_ms = npix / 8 * PLANES / HBM_PEAK * 1e3
    sub = 2 * total
    emit(f"  a call that runs nothing takes {idle_ms:.4f} ms (ten of them after the 64-iteration schedule, less that schedule)")
    emit(f"  per sub-iteration: {multi / sub * 1e3:.2f} us with 16 sub-iterations a launch (init and output pass included), "
         f"{single / sub * 1e3:.2f} us with 2 a launch, {(single - total * idle_ms) / sub * 1e3:.2f} us with 2 a launch less the calls' fixed cost: "
         f"{(single - total * idle_ms) / max(multi - idle_ms, 1e-9):.2f} times the on-chip schedule")
    emit(f"  ten bit planes are {npix / 8 * PLANES / 1e6:.2f} MB: {floor_ms * 1e3:.2f} us a sub-iteration at the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s, "
         f"{floor_ms / (multi / sub):.1%} of the time a sub-iteration takes on chip")
    emit(f"  thinning to the fixed point takes {multi / times['clx_label_distance_sq']:.2f} times clx_label_distance_sq; workspace "
         f"{nbytes / npix:.2f} bytes a pixel; no counters were taken; 3-D stacks were not timed")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton needs a HIP device")
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
