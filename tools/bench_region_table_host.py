"""Wall time of region_table with every flag on, which is mostly HOST time (the columns are formed in Python integers): a
2048 x 2048 map tiled with 4096 squares of 24 x 24 pixels, one per 32 x 32 cell, so they do not touch, and two float32
channels.  One warm-up, then five timed runs, each ending in torch.cuda.synchronize().

    python tools/bench_region_table_host.py [--other PATH/measure.py]

--other times another version of cellulus_amd/measure.py first (loaded as a module of this package beside the tree's own, so
it runs on the same library) and checks that both give the same table: how profiles/measure_refactor.txt compared the stage
before and after its host code was restructured.
"""

import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellulus_amd import measure  # noqa: E402

FLAGS = dict(boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.25, 0.5), mad=True, texture=True, radial=True,
             radial_wedges=True, std=True, colocalization=True, weighted=True, border_intensity=True)


def inputs(size=2048, cell=32, side=24):
    y, x = np.indices((size, size), dtype=np.int64)
    inside = (y % cell < side) & (x % cell < side)
    labels = np.where(inside, (y // cell) * (size // cell) + x // cell + 1, 0).astype(np.int32)
    raw = np.stack([((37 * y + 11 * x + 101 * c) % 251) / 8 - 7 for c in range(2)]).astype(np.float32)
    return labels, raw


def timed(module, labels, raw, device, runs=5):
    table = module.region_table(labels, raw, device, **FLAGS)                 # warm-up
    torch.cuda.synchronize()
    seconds = []
    for _ in range(runs):
        t0 = time.perf_counter()
        module.region_table(labels, raw, device, **FLAGS)
        torch.cuda.synchronize()
        seconds.append(time.perf_counter() - t0)
        print("  run %d: %.3f s" % (len(seconds), seconds[-1]), flush=True)
    return table, seconds


def report(name, seconds):
    print("%-8s %s  median %.3f s, max - min %.3f s" % (name, " ".join("%.3f" % s for s in seconds), statistics.median(seconds),
                                                         max(seconds) - min(seconds)), flush=True)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--other", help="another version of cellulus_amd/measure.py to time first")
    args = parser.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    labels, raw = inputs()
    print("python " + " ".join(sys.argv), flush=True)
    other = None
    if args.other:
        spec = importlib.util.spec_from_file_location("cellulus_amd._measure_other", args.other)
        module = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = module
        spec.loader.exec_module(module)
        other, seconds = timed(module, labels, raw, device)
        report("other", seconds)
    table, seconds = timed(measure, labels, raw, device)
    report("tree", seconds)
    if other is not None:
        same = list(other) == list(table) and all(a.dtype == b.dtype and a.tobytes() == b.tobytes()
                                                  for a, b in zip(other.values(), table.values()))
        print("tables identical: %s (%d columns, %d rows)" % (same, len(table), len(table["label"])))
