"""Times the measure stage's kernels (clx_region_moments, clx_region_intensity) against the same per-object sums
written with torch ops on the device (torch.bincount / index_add_ / scatter_reduce per quantity over the object
pixels: what a user can do today without them), on the inference benchmark's geometry: discs of radius 12 on a
jittered grid, 4096^2 (6 400 objects) and 512^2, float32 raw.  HIP events, warm-up, the legs alternating inside every
round; min and spread over the rounds.  Three more label maps of the same size separate what bounds the kernels: the
same discs under ONE id (the same runs and edges, but one table entry and one flush per block), an all-background map
(no table, no atomics: reading and run detection only) and a map that is one object (runs of full wave length).

    python tools/bench_measure.py [--out FILE] [--rounds 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure_columns import intensity_shift  # noqa: E402

PEAK_TBS = 8.0
dev = torch.device("cuda:0")


def disc_map(size, spacing=51, radius=12, jitter=6, seed=1):
    """bench_infer.synthetic_embeddings' geometry as a label map, ids in raster order of the grid cells"""
    rs = np.random.RandomState(seed)
    n = (size + spacing - 1 - spacing // 2) // spacing + 1
    centres = spacing // 2 + spacing * np.arange(n)
    centres = centres[centres < size]
    n = len(centres)
    cy = centres[:, None] + rs.randint(-jitter, jitter + 1, size=(n, n))
    cx = centres[None, :] + rs.randint(-jitter, jitter + 1, size=(n, n))
    cell = np.minimum(np.arange(size) // spacing, n - 1)
    iy, ix = cell[:, None], cell[None, :]
    yy, xx = np.arange(size)[:, None], np.arange(size)[None, :]
    inside = (yy - cy[iy, ix]) ** 2 + (xx - cx[iy, ix]) ** 2 <= radius * radius
    return np.where(inside, iy * n + ix + 1, 0).astype(np.int32), n * n


def time_legs(legs, rounds, reps):
    """legs: name -> fn.  Returns name -> list of ms per call, one per round; the legs alternate inside a round."""
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps[name])
    return times


def bench(size, rounds, emit):
    labels_h, nobj = disc_map(size)
    nid = nobj + 1
    npix = size * size
    rng = np.random.default_rng(0)
    raw_h = (rng.random((size, size), dtype=np.float32) * 1000.0).astype(np.float32)
    lab = torch.from_numpy(labels_h).to(dev)
    maps = {"discs": lab, "discs under one id": (lab > 0).to(torch.int32), "background": torch.zeros_like(lab),
            "one object": torch.ones_like(lab)}
    raw = torch.from_numpy(raw_h).to(dev)
    st = _clx.stream_ptr(dev)
    shift = intensity_shift(float(raw_h.max()), npix)

    area = torch.empty(nid, dtype=torch.int64, device=dev)
    bbox = torch.empty((nid, 6), dtype=torch.int32, device=dev)
    sum1 = torch.empty((nid, 3), dtype=torch.int64, device=dev)
    sum2 = torch.empty((nid, 6), dtype=torch.int64, device=dev)
    isum = torch.empty(nid, dtype=torch.int64, device=dev)
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)

    def moments(m=lab):
        _clx.call("clx_region_moments", _clx.ptr(m), 1, size, size, nid, _clx.ptr(area), _clx.ptr(bbox), _clx.ptr(sum1),
                  _clx.ptr(sum2), _clx.ptr(bad), st)

    def intensity(m=lab):
        _clx.call("clx_region_intensity", _clx.ptr(m), _clx.ptr(raw), 0, npix, nid, shift, _clx.ptr(isum), _clx.ptr(vkey),
                  _clx.ptr(bad), st)

    t_out = {}

    # the torch formulation selects the object pixels first: with the background in, five pixels of six add to row 0 of
    # every quantity, and one call takes longer than all the rounds of everything else here together
    def torch_moments():
        idx = torch.nonzero(lab.reshape(-1)).reshape(-1)
        l = lab.reshape(-1)[idx].long()
        y, x = idx // size, idx % size
        t_out["area"] = torch.bincount(l, minlength=nid)
        for name, v in (("sy", y), ("sx", x), ("syy", y * y), ("sxx", x * x), ("syx", y * x)):
            t_out[name] = torch.zeros(nid, dtype=torch.int64, device=dev).index_add_(0, l, v)
        for name, v, red, init in (("ymin", y, "amin", npix), ("xmin", x, "amin", npix), ("ymax", y, "amax", -1),
                                   ("xmax", x, "amax", -1)):
            t_out[name] = torch.full((nid,), init, dtype=torch.int64, device=dev).scatter_reduce_(0, l, v, red)

    def torch_intensity():
        idx = torch.nonzero(lab.reshape(-1)).reshape(-1)
        l = lab.reshape(-1)[idx].long()
        v = raw.reshape(-1)[idx]
        t_out["isum"] = torch.zeros(nid, dtype=torch.float64, device=dev).index_add_(0, l, v.double())
        t_out["vmin"] = torch.full((nid,), float("inf"), device=dev).scatter_reduce_(0, l, v, "amin")
        t_out["vmax"] = torch.full((nid,), float("-inf"), device=dev).scatter_reduce_(0, l, v, "amax")

    # faster and different is not faster: the integer columns agree with the torch formulation
    import time
    for name, fn in (("clx_region_moments", moments), ("clx_region_intensity", intensity), ("torch moments", torch_moments),
                     ("torch intensity", torch_intensity)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        emit(f"{size} x {size}: first call of {name}: {(time.perf_counter() - t0) * 1e3:.1f} ms (host clock, includes set-up)")
    assert int(bad.item()) == 0
    assert torch.equal(area[1:], t_out["area"][1:]) and torch.equal(sum1[1:, 1], t_out["sy"][1:])
    assert torch.equal(sum1[1:, 2], t_out["sx"][1:]) and torch.equal(sum2[1:, 1], t_out["syy"][1:])
    assert torch.equal(sum2[1:, 2], t_out["sxx"][1:]) and torch.equal(sum2[1:, 5], t_out["syx"][1:])
    assert torch.equal(bbox[1:, 1].long(), t_out["ymin"][1:]) and torch.equal(bbox[1:, 5].long(), t_out["xmax"][1:])
    mean_k = torch.ldexp(isum[1:].double(), torch.tensor(-shift, device=dev)) / area[1:]
    mean_t = t_out["isum"][1:] / area[1:]
    assert float((mean_k - mean_t).abs().max()) < 1e-6

    legs = {"clx_region_moments": moments, "clx_region_intensity": intensity, "torch moments": torch_moments,
            "torch intensity": torch_intensity}
    for name, m in maps.items():
        if name != "discs":
            legs[f"clx_region_moments, {name}"] = lambda m=m: moments(m)
            legs[f"clx_region_intensity, {name}"] = lambda m=m: intensity(m)
    reps = {k: (1 if k.startswith("torch") else 10) for k in legs}
    times = time_legs(legs, rounds, reps)

    emit(f"{size} x {size}, {nobj} objects, float32 raw; {rounds} rounds, legs alternating; ms per call: min (max) of the rounds")
    best = {}
    for name, ts in times.items():
        lo, hi = min(ts), max(ts)
        best[name] = (lo, hi)
        nbytes = npix * 4 * (2 if "intensity" in name else 1)
        line = f"  {name:48s} {lo:9.4f} ({hi:9.4f}) ms"
        if name.startswith("clx"):
            tbs = nbytes / (lo * 1e-3) / 1e12
            line += f"   {nbytes / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {tbs / PEAK_TBS:4.2f} of the {PEAK_TBS:.0f} TB/s HBM peak"
        emit(line)
    for kernel, formulation in (("clx_region_moments", "torch moments"), ("clx_region_intensity", "torch intensity")):
        (klo, khi), (tlo, thi) = best[kernel], best[formulation]
        emit(f"  {formulation} / {kernel}: {tlo / klo:.1f}x (worst round of the kernel against the best of torch: {tlo / khi:.1f}x)")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 512])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_measure needs a HIP device")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for size in args.sizes:
        bench(size, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
