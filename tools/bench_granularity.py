"""Times the granularity stage's kernels (cellulus_amd.granularity -> clx_grey_morph, clx_grey_reconstruct, 2-D) on one workload:
the territories of tools/bench_propagate.py on 2048^2 and an image of Gaussian blobs of widths 2, 4 and 8 pixels on a flat floor,
in 256 grey levels, 16 scales.  Warm-up, then the median (min .. max) of the repeats with HIP events.  Per scale: the rounds in
which a tile changed, the time of the reconstruction with its rounds queued through the C ABI without a host read (64 rounds a
call), and the time with ONE round a call and info read after each, so that launch-plus-sync cost stands beside the queued
form.  The sweeps a tile makes inside a round are not counted: the kernel keeps no counter for them.  Then the total as a user
calls it (granular_spectrum(), the host reads info every 8 rounds and the sums after every scale), and clx_grey_morph's bytes
per second -- it reads and writes an int32 map -- against the HBM figures.  Before anything is timed the device sums are
compared with the restatement of tests/granularity_ref.py on a 256^2 crop.

    python tools/bench_granularity.py [--out FILE] [--repeats 10] [--size 2048] [--scales 16]
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
from bench_measure import dev  # noqa: E402
from bench_skeleton import summary, timed, workload  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.granularity import granular_spectrum  # noqa: E402
from cellulus_amd.propagate import image_levels  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12    # bytes / s: the specification, and what a float4 copy reaches


def blob_levels(size, seed=3):
    """256 grey levels of a flat floor with one Gaussian blob per 32 x 32 cell, widths 2, 4 and 8 in turn"""
    rs = np.random.RandomState(seed)
    image = torch.full((size, size), 10.0, dtype=torch.float32, device=dev)
    yy = torch.arange(size, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(size, device=dev, dtype=torch.float32)[None, :]
    cells = size // 32
    for sigma in (2.0, 4.0, 8.0):
        acc = torch.zeros_like(image)
        picks = [(cy, cx) for cy in range(cells) for cx in range(cells) if (cy * 7 + cx * 3) % 3 == int(np.log2(sigma)) - 1]
        reach = int(4 * sigma)
        for cy, cx in picks:
            y, x = cy * 32 + int(rs.randint(8, 24)), cx * 32 + int(rs.randint(8, 24))
            ys, xs = slice(max(0, y - reach), y + reach + 1), slice(max(0, x - reach), x + reach + 1)
            acc[ys, xs] += 200.0 * torch.exp(-((yy[ys] - y) ** 2 + (xx[:, xs] - x) ** 2) / (2.0 * sigma * sigma))
        image += acc
    return image_levels(image.cpu().numpy(), 256)


def bench(size, repeats, scales, emit):
    labels_h, nobj = workload(size)
    levels_h = blob_levels(size)
    npix = labels_h.size
    st, lib = _clx.stream_ptr(dev), _clx.load()

    from granularity_ref import ref_spectrum

    crop = np.s_[:256, :256]
    ids, sums = granular_spectrum(np.ascontiguousarray(labels_h[crop]), np.ascontiguousarray(levels_h[crop]), scales=4, device=dev)
    want = ref_spectrum(labels_h[crop], levels_h[crop], 4)
    assert np.array_equal(ids, want[0]) and sums.tolist() == want[1], "granular_spectrum differs from the restatement on the crop"

    g = torch.from_numpy(levels_h).to(dev).reshape(-1)
    out = torch.empty(npix, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    nbytes = int(lib.clx_grey_reconstruct_workspace(2, 1, size, size))
    work = torch.empty(nbytes // 4 + 2, dtype=torch.int32, device=dev)

    def morph(src, dst, op, steps):
        _clx.call("clx_grey_morph", _clx.ptr(src), None, 2, 1, size, size, op, steps, _clx.ptr(dst), _clx.ptr(bad), st)

    def call(marker, rounds, resume):
        _clx.call("clx_grey_reconstruct", _clx.ptr(marker), _clx.ptr(g), None, 2, 1, size, size, rounds, resume, _clx.ptr(out), _clx.ptr(info),
                  _clx.ptr(work), nbytes, st)

    def by_one(marker):
        """one round a call, info read after each -> the rounds in which a tile changed"""
        busy, calls = 0, 0
        while True:
            call(marker, 1, int(calls > 0))
            calls += 1
            found = info.tolist()
            busy += found[2]
            if found[1] == 0:
                return busy

    def queued(marker, rounds):
        done = 0
        while done < rounds:
            n = min(64, rounds - done)
            call(marker, n, int(done > 0))
            done += n

    emit(f"territories: {size} x {size}, {nobj} objects, {int((labels_h > 0).sum()) / npix:.0%} of the pixels; blobs of widths 2, 4 and 8 in 256 grey "
         f"levels; {scales} scales; {repeats} repeats: median (min .. max)")
    emit("  scale  rounds  queued, 64 rounds a call (HIP events)          one round a call, info read after each")
    e, totals = g, [0, 0.0, 0.0]
    for i in range(1, scales + 1):
        nxt = torch.empty_like(g)
        morph(e, nxt, 0, 1)
        e = nxt
        busy = by_one(e)
        rounds = busy + 1                                   # the round that changes nothing is run too
        fast, slow = timed(lambda: queued(e, rounds), repeats), timed(lambda: by_one(e), repeats)
        emit(f"  {i:5d}  {busy:6d}  {summary(fast)}   {summary(slow)}")
        totals = [totals[0] + busy, totals[1] + statistics.median(fast), totals[2] + statistics.median(slow)]
    emit(f"  all    {totals[0]:6d}  {totals[1]:9.4f} ms queued, {totals[2]:9.4f} ms one round a call: {totals[2] / max(totals[1], 1e-9):.2f} times; "
         f"{totals[1] / max(totals[0] + scales, 1) * 1e3:.2f} us a round queued")
    labels = torch.from_numpy(labels_h).to(dev)
    whole = timed(lambda: granular_spectrum(labels, g.reshape(size, size), scales=scales), max(3, repeats // 3))
    emit(f"  granular_spectrum(), {scales} scales, host loop: {summary(whole)}")
    for steps in (1, 16):
        ms = timed(lambda: morph(g, out, 0, steps), repeats)
        rate = 8.0 * npix / (statistics.median(ms) * 1e-3)
        emit(f"  clx_grey_morph, erode, {steps:2d} steps: {summary(ms)}: {rate / 1e12:.3f} TB/s of the {8 * npix / 1e6:.1f} MB it reads and writes, "
             f"{rate / HBM_COPY:.1%} of a copy's {HBM_COPY / 1e12:.2f} TB/s, {rate / HBM_PEAK:.1%} of the {HBM_PEAK / 1e12:.1f} TB/s peak")
    emit(f"  workspace {nbytes / npix:.2f} bytes a pixel; no counters were taken; 3-D stacks were not timed")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--scales", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_granularity needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    bench(args.size, args.repeats, args.scales, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
