"""Does the split precision pay at channel counts that are multiples of 64 (clx_conv_desc.precision =
CLX_PREC_F32X3BF16_G64, CLX_PRECISION=f32x3bf16g64)?  Kernel level: the split product / weight gradient from planes, and the
same 1x1 layer through clx_conv_fwd / clx_conv_wgrad with precision = 2 (split passes included) against precision = 0
(float32 MFMA) — device events, the legs alternating in one process, ROUNDS rounds each; TFLOP/s f32-equivalent (2 M N K),
min .. max over the rounds, and the ratio of the medians.  Step level: one training step of a network under
CLX_PRECISION=f32x3bf16g64 against the default, alternating.

    python tools/bench_sp64.py [--kernels] [--steps] [--out FILE]        # default: both parts
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellulus_amd import _clx
from cellulus_amd._clx import ClxConvDesc, ClxSrc

ROUNDS = 3
REPS = 8
M_BENCH = 516128                     # 8 x 254^2: the top level of the 2-D benchmark step
SHAPES = [(64, 256), (64, 768), (64, 1024), (192, 192), (576, 576), (320, 320)]          # (N, K)
dev = torch.device("cuda:0")
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def planes_of(x):
    rows, K = x.shape
    buf = torch.empty(_clx.load().clx_planes_bytes(rows, K), dtype=torch.uint8, device=dev)
    _clx.call("clx_split_planes", _clx.ptr(x), x.stride(0), rows, K, _clx.ptr(buf), _clx.stream_ptr(dev))
    return buf


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(legs):
    """legs: name -> callable; one warm-up each, then ROUNDS rounds in turn; name -> list of ms"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    return ms


def report(what, flops, ms, base):
    med = {k: statistics.median(v) for k, v in ms.items()}
    parts = []
    for k, v in ms.items():
        tf = sorted(flops / t / 1e9 for t in v)
        ratio = "" if k == base else f" x{med[base] / med[k]:.2f}"
        parts.append(f"{k} {med[k]:7.3f} ms {tf[0]:6.1f}..{tf[-1]:6.1f} TF/s{ratio}")
    say(f"{what}  " + " | ".join(parts))


def tile256(fn):
    """fn under CLX_SP_TILE=256 (read per launch): the 256 x 128 kernel, whose last tile column is half dead at N % 128 == 64"""
    os.environ["CLX_SP_TILE"] = "256"
    try:
        fn()
    finally:
        del os.environ["CLX_SP_TILE"]


def pointwise_desc(x, M, C, N, w, out, precision, wplanes=None, aplanes=None, dyplanes=None):
    d = ClxConvDesc()
    d.nsrc = 1
    s = ClxSrc()
    s.ptr, s.C, s.ld = x.data_ptr(), C, C
    s.D, s.H, s.W = 1, 1, M
    s.oz = s.oy = s.ox = 0
    s.fz = s.fy = s.fx = 1
    d.src[0] = s
    d.B, d.ID, d.IH, d.IW = 1, 1, 1, M
    d.KD = d.KH = d.KW = 1
    d.N = N
    d.wpack = w.data_ptr() if w is not None else None
    d.out, d.ld_out = (out.data_ptr(), N) if out is not None else (None, N)
    d.precision = precision
    d.wplanes = wplanes.data_ptr() if wplanes is not None else None
    d.aplanes = aplanes.data_ptr() if aplanes is not None else None
    d.dyplanes = dyplanes.data_ptr() if dyplanes is not None else None
    return d


def kernel_level(M):
    st = _clx.stream_ptr(dev)
    say(f"# kernel level, M = {M}: f32 = float32 MFMA through clx_conv_fwd / clx_conv_wgrad (precision 0); planes = the split")
    say("# product from ready planes (clx_gemm_planes / clx_wgrad_planes; planes/256x128: forced onto the 256 x 128 kernel); layer =")
    say("# clx_conv_fwd / clx_conv_wgrad with precision 2 where the rule covers the shape (elsewhere it is float32 again), its split")
    say(f"# pass(es) included.  {ROUNDS} rounds x {REPS} launches per leg, alternating; TF/s = 2 M N K / t, min..max over the rounds;")
    say("# xR = median time of f32 / median time of the leg")
    for N, K in SHAPES:
        torch.manual_seed(0)
        x = torch.relu(torch.randn(M, K, device=dev))
        w = torch.randn(N, K, device=dev) / K ** 0.5
        bias = torch.randn(N, device=dev)
        out = torch.empty(M, N, device=dev)
        pa, pb = planes_of(x), planes_of(w)
        d0 = pointwise_desc(x, M, K, N, w, out, 0)
        d2 = pointwise_desc(x, M, K, N, w, out, 2, wplanes=pb, aplanes=pa)
        for d in (d0, d2):
            d.bias, d.relu = bias.data_ptr(), 1
        covers = _clx.load().clx_conv_sp_covers(ctypes.byref(d2), 0), _clx.load().clx_conv_sp_covers(ctypes.byref(d2), 1)
        say(f"N={N} K={K}: clx_conv_sp_covers(precision 2) = {covers}")
        ms = alternate({
            "f32": lambda: _clx.call("clx_conv_fwd", ctypes.byref(d0), st),
            "planes": lambda: _clx.call("clx_gemm_planes", _clx.ptr(pa), _clx.ptr(pb), M, N, K, _clx.ptr(bias), 1, _clx.ptr(out), N, st),
            "layer": lambda: _clx.call("clx_conv_fwd", ctypes.byref(d2), st),
            "planes/256x128": lambda: tile256(lambda: _clx.call("clx_gemm_planes", _clx.ptr(pa), _clx.ptr(pb), M, N, K, _clx.ptr(bias), 1,
                                                               _clx.ptr(out), N, st)),
        })
        report(f"fwd   N={N:4d} K={K:5d}", 2.0 * M * N * K, ms, "f32")
        # the weight gradient dW[N][K] of the same layer
        dy = out
        dy.normal_()
        pdy = planes_of(dy)
        dw = torch.zeros(N, K, device=dev)
        g0 = pointwise_desc(x, M, K, N, None, None, 0)
        g2 = pointwise_desc(x, M, K, N, None, None, 2, aplanes=pa, dyplanes=pdy)
        ms = alternate({
            "f32": lambda: _clx.call("clx_conv_wgrad", ctypes.byref(g0), _clx.ptr(dy), N, _clx.ptr(dw), None, st),
            "planes": lambda: _clx.call("clx_wgrad_planes", _clx.ptr(pdy), _clx.ptr(pa), M, N, K, _clx.ptr(dw), K, st),
            "layer": lambda: _clx.call("clx_conv_wgrad", ctypes.byref(g2), _clx.ptr(dy), N, _clx.ptr(dw), None, st),
        })
        report(f"wgrad N={N:4d} C={K:5d}", 2.0 * M * N * K, ms, "f32")
        del x, w, out, pa, pb, pdy, dw
        torch.cuda.empty_cache()


def step_level(steps):
    import bench
    from cellulus_amd.train import train_iteration

    bench.WORKLOADS["train2d_64x3"] = dict(
        name="2D 1x256x256 crops, num_fmaps=64, fmap_inc_factor=3, downsampling=[[2,2]], batch 8",
        model=dict(in_channels=1, out_channels=2, num_fmaps=64, fmap_inc_factor=3, features_in_last_layer=64,
                   downsampling_factors=[[2, 2]], num_spatial_dims=2),
        crop=(256, 256), batch=8, kappa=10.0, density=0.1)
    say()
    say(f"# step level: one training step (bench.py's inputs), {ROUNDS} rounds x {steps} steps per leg, alternating; crops/s min..max")
    names = {"default": "", "g64": "f32x3bf16g64"}
    for key in ("train2d_64x3", "train2d", "train3d"):
        legs = {}
        for leg, env in names.items():
            os.environ.pop("CLX_PRECISION", None)
            if env:
                os.environ["CLX_PRECISION"] = env
            model, crit, opt, batch = bench.build_step_inputs(key, 0, dev, broadcast=False)
            for _ in range(3):
                train_iteration(batch, model, crit, opt, dev)
            torch.cuda.synchronize()
            plan = next(iter(model._plans.values()))
            split = sorted(n for n, s in plan.sp_pass.items() if any(s))
            legs[leg] = (env, model, crit, opt, batch, split)
        rates = {leg: [] for leg in legs}
        for _ in range(ROUNDS):
            for leg, (env, model, crit, opt, batch, _s) in legs.items():
                os.environ.pop("CLX_PRECISION", None)
                if env:
                    os.environ["CLX_PRECISION"] = env
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _i in range(steps):
                    train_iteration(batch, model, crit, opt, dev)
                torch.cuda.synchronize()
                rates[leg].append(bench.WORKLOADS[key]["batch"] * steps / (time.perf_counter() - t0))
        med = {k: statistics.median(v) for k, v in rates.items()}
        say(f"{key:13s} " + " | ".join(f"{k} {min(v):7.1f}..{max(v):7.1f} crops/s" for k, v in rates.items())
            + f" | g64 / default x{med['g64'] / med['default']:.3f}")
        say(f"{'':13s} layers with a split pass: default {len(legs['default'][5])}, g64 {len(legs['g64'][5])}")
        del legs
        bench.release_device_memory()
    os.environ.pop("CLX_PRECISION", None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--rows", type=int, default=M_BENCH)
    ap.add_argument("--step-count", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    both = not (a.kernels or a.steps)
    say(f"# tools/bench_sp64.py on {torch.cuda.get_device_name(0)}")
    if a.kernels or both:
        kernel_level(a.rows)
    if a.steps or both:
        step_level(a.step_count)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
