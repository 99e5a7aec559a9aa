"""Times clx_cc_label_filter on a 3-D volume, where it takes the run pipeline (cc_init_runs, cc_merge_runs, cc_flatten_count and
the numbering passes; tools/bench_fill.py times the 2-D label-list pipeline): 64 x 512 x 512 pixels, cubes of 12^3 pixels in
five values on a lattice of 24, an eighth of the volume.  Warm-up, then the median (min .. max) of the repeats with HIP events
around the call; the number of components and a checksum of the output are printed to compare two libraries' results.

    python tools/bench_cc_volume.py [--repeats 20]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellulus_amd import _clx  # noqa: E402

Z, Y, X = 64, 512, 512

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cc_volume needs a HIP device")
    dev = torch.device("cuda:0")
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    vol = ((zz // 12) % 2) * ((yy // 12) % 2) * ((xx // 12) % 2) * (1 + (zz // 24 + yy // 24 + xx // 24) % 5)
    seg = torch.from_numpy(vol.astype(np.int32)).to(dev).reshape(-1)
    npix = seg.numel()
    lib, st = _clx.load(), _clx.stream_ptr(dev)
    out = torch.empty(npix, dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(int(lib.clx_cc_workspace(npix)) // 4 + 1, dtype=torch.int32, device=dev)

    def run():
        _clx.call("clx_cc_label_filter", _clx.ptr(seg), _clx.ptr(out), Z, Y, X, 1, _clx.ptr(n), _clx.ptr(work), st)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"cubes: {Z} x {Y} x {X}, {int(n.item())} components, checksum {int(out.to(torch.int64).sum().item())}; "
          f"{args.repeats} repeats: median (min .. max)")
    print(f"  clx_cc_label_filter, min_size 1, run pipeline (HIP events) {statistics.median(ms):9.4f} ({min(ms):9.4f} .. {max(ms):9.4f}) ms")
