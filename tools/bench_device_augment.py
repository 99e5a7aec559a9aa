"""Times one batch of crops with the elastic augmentation on the device (clx_elastic_crop: 8 x 256^2 from 384^2 images and
8 x 64^3 from 96^3 volumes, float32 — the shapes bench.py's train_e2e uses) with device events, and beside it
ZarrDataset._elastic_crop per crop on one core of the same host.  Also what train.loader_policy gives eight ranks on
this host, with and without CLX_DEVICE_AUGMENT.  Usage: python tools/bench_device_augment.py [--reps N]"""
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellulus_amd.configs import DatasetConfig  # noqa: E402
from cellulus_amd.datasets import get_dataset  # noqa: E402
from cellulus_amd.datasets.zarr_dataset import DeviceCropSource, _single_threaded_blas, elastic_crop_on_device  # noqa: E402
from cellulus_amd.utils import zarr_io  # noqa: E402

PEAK_TBS = 8.0
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
B = 8


def case(label, crop, tmp, dev):
    nd = len(crop)
    big = tuple(int(c * 1.5) for c in crop)
    shape = (16, 1) + big
    data = np.random.default_rng(0).random(shape, dtype=np.float32)
    path = os.path.join(tmp, f"d{nd}.zarr")
    f = zarr_io.open(path)
    f["train/raw"] = data
    f["train/raw"].attrs["axis_names"] = ["s", "c"] + ["z", "y", "x"][-nd:]
    ds = get_dataset(DatasetConfig(container_path=path, dataset_name="train/raw"), crop_size=crop, elastic_deform=True,
                     control_point_spacing=64, control_point_jitter=2.0, density=0.1, kappa=10.0, normalization_factor=1.0)
    # host: _elastic_crop alone, a numpy array as the source
    random.seed(0)
    np.random.seed(0)
    for _ in range(2):
        ds._elastic_crop(data, 0, 1.0)
    t0 = time.perf_counter()
    n_host = 10
    for _ in range(n_host):
        ds._elastic_crop(data, 0, 1.0)
    host_ms = (time.perf_counter() - t0) / n_host * 1e3
    # device: one call = one batch; the records are uploaded before the timed window
    dev_data = torch.from_numpy(data.view(np.uint8).reshape(-1)).to(dev)
    py, npr = random.Random(1), np.random.RandomState(1)
    recs = [torch.from_numpy(ds.pack_params([ds.elastic_params(shape, py, npr) for _ in range(B)])).to(dev)
            for _ in range(8)]
    out = torch.empty((B, 1) + tuple(crop), dtype=torch.float32, device=dev)
    mx = torch.empty(B, dtype=torch.float32, device=dev)
    for r in recs:
        elastic_crop_on_device(ds, dev_data, shape, np.float32, 1.0, r, dev, out, mx)
    torch.cuda.synchronize()
    times = []
    for i in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        elastic_crop_on_device(ds, dev_data, shape, np.float32, 1.0, recs[i % len(recs)], dev, out, mx)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    # a back-to-back window too: the launches of a run overlap their enqueue with the device
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(REPS):
        elastic_crop_on_device(ds, dev_data, shape, np.float32, 1.0, recs[i % len(recs)], dev, out, mx)
    e1.record()
    torch.cuda.synchronize()
    stream_ms = e0.elapsed_time(e1) / REPS
    # algorithmic bytes: the crops written + the source window a crop touches (its own extent, rotated: about as much)
    written = out.numel() * 4
    tbs = 2 * written / (med * 1e-3) / 1e12
    # the host side of a batch in the source: draw + pack the parameters
    t0 = time.perf_counter()
    for _ in range(20):
        ds.pack_params([ds.elastic_params(shape, py, npr) for _ in range(B)])
    draw_ms = (time.perf_counter() - t0) / 20 * 1e3
    print(f"{label:24s} clx_elastic_crop, batch of {B}: median {med:.3f} ms of {REPS} calls (min {times[0]:.3f}, max "
          f"{times[-1]:.3f}); back to back {stream_ms:.3f} ms per call = {B / stream_ms * 1e3:.0f} crops/s")
    print(f"{label:24s} bytes written + source touched {2 * written / 1e6:.1f} MB -> {tbs:.3f} TB/s "
          f"({100 * tbs / PEAK_TBS:.2f} % of the {PEAK_TBS:.0f} TB/s HBM peak; latency-bound at this size)")
    print(f"{label:24s} host: _elastic_crop {host_ms:.2f} ms per crop on one core = {1e3 / host_ms:.0f} crops/s per loader "
          f"process; drawing + packing a batch's parameters {draw_ms:.3f} ms")
    print(f"{label:24s} host time per crop / device time per crop: {host_ms / (stream_ms / B):.0f}x")
    src = DeviceCropSource(ds, dev, B, seed=0)
    for _ in range(3):
        next(src)
    t0 = time.perf_counter()
    for _ in range(50):
        next(src)
    torch.cuda.synchronize()
    print(f"{label:24s} DeviceCropSource on its own (draw, pack, upload, two launches, maxima read back): "
          f"{(time.perf_counter() - t0) / 50 * 1e3:.3f} ms per batch, {src.rejected} crops redrawn")


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    _single_threaded_blas()              # the host figure is one loader process's: numpy's BLAS on one thread, as there
    print(f"device: {torch.cuda.get_device_name(0)}; host cores available: {len(os.sched_getaffinity(0))}")
    with tempfile.TemporaryDirectory() as tmp:
        case("2-D 8 x 256^2 of 384^2", (256, 256), tmp, dev)
        case("3-D 8 x 64^3 of 96^3", (64, 64, 64), tmp, dev)
    from cellulus_amd.train import loader_policy

    for flag in ("0", "1"):
        os.environ["CLX_DEVICE_AUGMENT"] = flag
        p = loader_policy(8, 8)
        print(f"loader_policy(world=8, num_workers=8), CLX_DEVICE_AUGMENT={flag}: {p['loader_procs']} loader processes per "
              f"rank, {p['host_cores_per_rank']} host cores per rank [{p['why']}]")
