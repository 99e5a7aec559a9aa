"""Times the measure stage's order statistics (clx_region_order_stats: the quartiles (0.25, 0.5, 0.75) of one raw channel per
object) phase by phase -- the gather that buckets the pixels' keys by object, the select that picks the keys of the six ranks
-- beside clx_region_intensity on the same inputs, the device yardstick (one pass over the same two arrays that keeps sums
and extrema instead of the keys), and beside what a user does on the host today: np.quantile per object on bounding-box crops.
Maps: tools/bench_measure.py's discs of radius 12 on a jittered grid, 4096^2 (6 400 objects of about 450 pixels: the LDS sort)
and 512^2, and at 4096^2 the map that is one object everywhere (one segment of 2^24 keys: the radix select by many blocks).
Raw: 16-bit counts as int32 and float32 (4 radix passes where a segment is too long to sort; float64 and the MAD's second
call take 8).  HIP events, warm-up, the legs alternating inside every round; min and max over the rounds.  The host leg is
one run on the host clock.  Before anything is timed the selected keys are compared with a sort of every object's values.

    python tools/bench_order_stats.py [--out FILE] [--rounds 5]
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_measure import dev, disc_map, time_legs  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure_columns import intensity_shift, quantile_ranks  # noqa: E402
from cellulus_amd.segment import _RAW_F32, _RAW_I32, _decode_keys  # noqa: E402

QS = (0.25, 0.5, 0.75)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def select_constants():
    """SORT_MAX, BLOCK_MAX of csrc/region_order.hip"""
    text = open(os.path.join(ROOT, "cellulus_amd", "csrc", "region_order.hip")).read()
    return tuple(int(re.search(r"constexpr \w[\w ]* %s = (\d+);" % name, text).group(1)) for name in ("SORT_MAX", "BLOCK_MAX"))


def host_quantiles(labels, raw, ranks):
    """np.quantile per object on bounding-box crops, timed; then (not timed) the order statistics at `ranks` from a sort
    -> (seconds, values (objects, nq))"""
    boxes = ndimage.find_objects(labels)
    t0 = time.perf_counter()
    for i, box in enumerate(boxes, 1):
        if box is not None:
            np.quantile(raw[box][labels[box] == i], QS)
    seconds = time.perf_counter() - t0
    want = np.zeros((len(boxes), ranks.shape[1]), dtype=raw.dtype)
    for i, box in enumerate(boxes, 1):
        if box is not None:
            want[i - 1] = np.sort(raw[box][labels[box] == i])[ranks[i]]
    return seconds, want


def bench(name, labels_h, nobj, raw_name, raw_h, raw_type, rounds, emit):
    size = labels_h.shape[0]
    npix = labels_h.size
    nid = nobj + 1
    lib = _clx.load()
    st = _clx.stream_ptr(dev)
    area = np.bincount(labels_h.reshape(-1), minlength=nid).astype(np.int64)
    area[0] = 0
    present = np.flatnonzero(area)
    ranks = np.zeros((nid, 2 * len(QS)), dtype=np.int64)
    for j, q in enumerate(QS):
        lo, hi, _ = quantile_ranks(area[present], q)
        ranks[present, 2 * j], ranks[present, 2 * j + 1] = lo, hi
    total = int(area.sum())
    nbytes = int(lib.clx_region_order_workspace(total, nid))
    lab = torch.from_numpy(labels_h).to(dev).reshape(-1)
    raw = torch.from_numpy(raw_h).to(dev).reshape(-1)
    area_d, base_d, rank_d = (torch.from_numpy(v).to(dev) for v in (area, np.cumsum(area) - area, ranks))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty((nid, ranks.shape[1]), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    isum = torch.empty(nid, dtype=torch.int64, device=dev)
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)
    shift = 0 if raw_type == _RAW_I32 else intensity_shift(float(np.abs(raw_h).max()), npix)
    args = (_clx.ptr(lab), _clx.ptr(raw), raw_type, npix, nid, _clx.ptr(area_d), _clx.ptr(base_d), total, _clx.ptr(None),
            _clx.ptr(rank_d), ranks.shape[1], _clx.ptr(out), _clx.ptr(work), nbytes, _clx.ptr(bad))

    def gather():
        _clx.call("clx_region_order_phase", *args, 1, st)

    def select():
        _clx.call("clx_region_order_phase", *args, 2, st)

    def whole():
        _clx.call("clx_region_order_stats", *args, st)

    def intensity():
        _clx.call("clx_region_intensity", _clx.ptr(lab), _clx.ptr(raw), raw_type, npix, nid, shift, _clx.ptr(isum), _clx.ptr(vkey),
                  _clx.ptr(bad), st)

    # faster and different is not faster: the selected keys against a sort of every object's values
    host_s, want = host_quantiles(labels_h, raw_h, ranks)
    whole()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    got = _decode_keys(out.cpu().numpy().view(np.uint64)[1:], raw_type)
    assert np.array_equal(got[present - 1], want[present - 1]), "clx_region_order_stats differs from a sort per object"
    gather()
    select()
    torch.cuda.synchronize()
    assert np.array_equal(_decode_keys(out.cpu().numpy().view(np.uint64)[1:], raw_type), got) and int(bad.item()) == 0

    sort_max, block_max = select_constants()
    passes = 4                                               # float32 / int32 keys without a centre
    a = area[present]
    read = int(8 * a[a <= sort_max].sum() + 8 * passes * a[a > sort_max].sum())
    legs = {"gather (phase 1)": gather, "select (phase 2)": select, "clx_region_order_stats": whole, "clx_region_intensity": intensity}
    times = time_legs(legs, rounds, {k: 10 for k in legs})
    emit(f"{name}, {raw_name}: {size} x {size}, {len(present)} objects, {total / npix:.0%} object pixels, largest object {int(a.max())} "
         f"pixels ({int((a <= sort_max).sum())} sorted in LDS, {int(((a > sort_max) & (a <= block_max)).sum())} selected by one block, "
         f"{int((a > block_max).sum())} by many); {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    best = {leg: (min(ts), max(ts)) for leg, ts in times.items()}
    for leg, (lo, hi) in best.items():
        emit(f"  {leg:44s} {lo:9.4f} ({hi:9.4f}) ms")
    emit(f"  {'np.quantile per object on crops (host, one run)':44s} {host_s * 1e3:9.1f} ms")
    g, s, w, y = (best[k] for k in legs)
    emit(f"  the select phase reads {read / total:.1f} bytes per key ({read / 1e6:.1f} MB: {read / s[0] / 1e6:.1f} GB/s); "
         f"the gather reads {8 * npix / 1e6:.1f} MB and writes {8 * total / 1e6:.1f} MB")
    emit(f"  clx_region_order_stats / clx_region_intensity: {w[0] / y[0]:.2f}x (worst round against the yardstick's best: {w[1] / y[0]:.2f}x); "
         f"gather alone {g[0] / y[0]:.2f}x, select alone {s[0] / y[0]:.2f}x")
    emit(f"  host / clx_region_order_stats: {host_s * 1e3 / w[0]:.0f}x")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 512])
    ap.add_argument("--one-object", type=int, nargs="*", default=[4096], help="sizes at which the one-object map is timed too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_order_stats needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    def raws(size):
        rng = np.random.default_rng(0)
        return (("uint16 counts as int32", rng.integers(0, 65536, (size, size)).astype(np.int32), _RAW_I32),
                ("float32", (rng.random((size, size), dtype=np.float32) * 1000.0).astype(np.float32), _RAW_F32))

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for size in args.sizes:
        labels, nobj = disc_map(size)
        for raw_name, raw, raw_type in raws(size):
            bench("discs", labels, nobj, raw_name, raw, raw_type, args.rounds, emit)
    for size in args.one_object:
        for raw_name, raw, raw_type in raws(size):
            bench("one object everywhere", np.ones((size, size), np.int32), 1, raw_name, raw, raw_type, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
