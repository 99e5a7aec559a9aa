"""Times the propagate stage's kernel (cellulus_amd.propagate.geodesic_owner -> clx_label_propagate, 2-D) on one workload: the
2 025 jittered discs of tools/bench_nearest.py on 2048^2 as seeds, the mask expand_labels(seeds, 20) > 0, and as weight a
synthetic membrane along the borders of the seeds' zones in 256 levels (255 on a border pixel, 128 beside one).  Warm-up, then
the median (min .. max) of the repeats with HIP events around the whole converged sequence of calls: as geodesic_owner makes
them, 8 rounds a call and a look at info[1] after each, and with the same rounds queued 64 a call without a look between.  The
rounds and the active tile-rounds are counted in a run of one round a call that reads the tiles' changed flags from the
workspace after every round.  Yardstick: clx_label_nearest on the same seeds in the same run -- the unconstrained single-pass
answer, a floor for scale and not a target.  Before anything is timed the device maps are compared with the Jacobi
restatement of tests/propagate_ref.py on a 256^2 crop, whose heap Dijkstra is timed once as a host yardstick.

    python tools/bench_propagate.py [--out FILE] [--repeats 20] [--size 2048]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bench_measure import dev, disc_map  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.expand import expand_labels, nearest_object  # noqa: E402
from cellulus_amd.propagate import ROUNDS_PER_CALL, geodesic_owner  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s (specification)
TILE_Y, TILE_X, HEAD_BYTES = 16, 64, 4 * (16 + 64)                  # csrc/label_propagate.hip: TileShape<2>, the head and the counters
# an active tile reads, per pixel, its key (8), weight (4), seed (4) and mask byte (1) and writes a key (8); the halo is a
# re-read of what the neighbour tiles read as their own and is not counted
BYTES_PER_ACTIVE_PIXEL = 8 + 4 + 4 + 1 + 8


def summary(ms):
    return f"{statistics.median(ms):9.4f} ({min(ms):9.4f} .. {max(ms):9.4f}) ms"


def membrane(zones):
    """int32 levels: 255 where a zone meets another (4-neighbours), 128 beside such a pixel, else 0"""
    border = torch.zeros_like(zones, dtype=torch.bool)
    border[:, :-1] |= zones[:, :-1] != zones[:, 1:]
    border[:-1, :] |= zones[:-1, :] != zones[1:, :]
    near = torch.nn.functional.max_pool2d(border[None, None].float(), 3, 1, 1)[0, 0] > 0
    return torch.where(border, 255, torch.where(near, 128, 0)).to(torch.int32)


def bench(size, repeats, emit):
    labels_h, nobj = disc_map(size, spacing=46, radius=10, jitter=5)
    npix, nid = labels_h.size, nobj + 1
    seeds = torch.from_numpy(labels_h).to(dev)
    mask = (expand_labels(seeds, 20) > 0).to(torch.uint8).contiguous()
    weight = membrane(nearest_object(seeds)[0]).contiguous()
    st, lib = _clx.stream_ptr(dev), _clx.load()
    owner, cost = (torch.empty(npix, dtype=torch.int32, device=dev) for _ in range(2))
    info = torch.empty(3, dtype=torch.int32, device=dev)
    nbytes = int(lib.clx_label_propagate_workspace(2, 1, size, size))
    work = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    nty, ntx = -(-size // TILE_Y), -(-size // TILE_X)

    def call(rounds, resume):
        _clx.call("clx_label_propagate", _clx.ptr(seeds), _clx.ptr(mask), _clx.ptr(weight), 2, 1, size, size, nid, 1, -1, rounds, resume,
                  _clx.ptr(owner), _clx.ptr(cost), _clx.ptr(info), _clx.ptr(work), nbytes, st)

    # correctness on a crop, and the host yardstick
    from propagate_ref import ref_propagate, ref_propagate_sweeps

    crop = tuple(t[:256, :256].contiguous() for t in (seeds, mask, weight))
    got = [t.cpu().numpy() for t in geodesic_owner(*crop)]
    crop_h = [t.cpu().numpy() for t in crop]
    want = ref_propagate_sweeps(*crop_h, nid=nid)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "geodesic_owner differs from the restatement on the crop"
    t0 = time.perf_counter()
    ref_propagate(*crop_h, nid=nid)
    host_s = time.perf_counter() - t0

    # one round a call: the rounds, and from the changed flags the tiles active in each
    flags = work.view(torch.uint8)[HEAD_BYTES + 8 * npix:]
    pad = (nty * ntx + 3) // 4 * 4
    rounds, active, changed_tiles = 0, nty * ntx, 0
    while True:
        call(1, int(rounds > 0))
        if info.tolist()[1] == 0:
            break
        changed = flags[(rounds & 1) * pad:(rounds & 1) * pad + nty * ntx].reshape(nty, ntx)
        changed_tiles += int(changed.sum())
        rounds += 1
        active += int((torch.nn.functional.max_pool2d(changed[None, None].float(), 3, 1, 1) > 0).sum())
    rounds += 1                                               # the round that changed nothing ran on its active tiles too
    reached = int((owner > 0).sum())

    def looked():
        resume = 0
        while True:
            call(ROUNDS_PER_CALL, resume)
            if info.tolist()[1] == 0:
                return
            resume = 1

    def queued():
        for k in range(-(-rounds // 64)):
            call(64, int(k > 0))

    def nearest():
        _clx.call("clx_label_nearest", _clx.ptr(seeds), 2, 1, size, size, nid, -1, _clx.ptr(owner), _clx.ptr(cost), _clx.ptr(info), _clx.ptr(work),
                  int(lib.clx_label_nearest_workspace(npix)), st)

    emit(f"discs: {size} x {size}, {nobj} seeds, mask {int(mask.sum()) / npix:.0%} of the pixels, {reached} pixels reached; {rounds} rounds "
         f"({rounds - 1} changed a tile), {active} active tile-rounds of {rounds * nty * ntx} ({changed_tiles} changed); "
         f"{repeats} repeats: median (min .. max)")
    times = {}
    for name, run in (("8 rounds a call, info read after each", looked), ("64 rounds a call, no look between", queued),
                      ("clx_label_nearest, no limit", nearest)):
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
        times[name] = ms
        emit(f"  {name:42s} (HIP events) {summary(ms)}")
    best = min(statistics.median(times[name]) for name in list(times)[:2])
    nbytes_active = active * TILE_Y * TILE_X * BYTES_PER_ACTIVE_PIXEL
    floor_ms = nbytes_active / HBM_PEAK * 1e3
    emit(f"  {best / rounds:.4f} ms a round; {BYTES_PER_ACTIVE_PIXEL} algorithmic bytes a pixel of an active tile are {nbytes_active / 1e6:.1f} MB, "
         f"{floor_ms:.4f} ms at the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s, {floor_ms / best:.1%} of the time")
    emit(f"  heap Dijkstra of tests/propagate_ref.py on the 256 x 256 crop (host, one run) {host_s * 1e3:9.1f} ms")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_propagate needs a HIP device")
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
