"""Times the skeleton stage's branch graph (cellulus_amd.skeleton -> clx_skeleton_graph, 2-D) on one workload: the territories of
tools/bench_skeleton.py on 2048^2, thinned to the fixed point.  Warm-up, then the median (min .. max) of the repeats with HIP
events.  Timed: clx_skeleton_graph through the C ABI without and with dist_sq (rows, branch_map and out all asked for), with a
pruning limit, and without rows and maps; clx_skeleton_census on the same map in the same run, for scale and not a target.
Before anything is timed the device result is compared with the restatement of tests/skeleton_graph_ref.py on a 512^2 crop.

    python tools/bench_skeleton_graph.py [--out FILE] [--repeats 20] [--size 2048]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bench_measure import dev  # noqa: E402
from bench_skeleton import summary, timed, workload  # noqa: E402
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd.measure import label_distance_sq  # noqa: E402
from cellulus_amd.skeleton import thin_labels  # noqa: E402


def bench(size, repeats, emit):
    from skeleton_graph_ref import graph

    labels_h, nobj = workload(size)
    npix = labels_h.size
    skeleton = thin_labels(torch.from_numpy(labels_h).to(dev)).contiguous()
    dist = label_distance_sq(labels_h, device=dev).reshape(-1).contiguous()
    skel = skeleton.reshape(-1)
    st, lib = _clx.stream_ptr(dev), _clx.load()
    nid = int(labels_h.max()) + 1

    nbytes = int(lib.clx_skeleton_graph_workspace(2, 1, size, size))
    work = torch.empty(nbytes // 4 + 2, dtype=torch.int32, device=dev)
    branch_map, out = (torch.empty(npix, dtype=torch.int32, device=dev) for _ in range(2))
    info = torch.empty(6, dtype=torch.int32, device=dev)

    def call(lab, Y, X, d, limit, branches, nodes, maps=True):
        cb, cn = (0 if rows is None else len(rows) for rows in (branches, nodes))
        _clx.call("clx_skeleton_graph", _clx.ptr(lab), _clx.ptr(d), 2, 1, Y, X, limit, cb, cn, _clx.ptr(branch_map if maps else None),
                  _clx.ptr(out if maps else None), _clx.ptr(branches), _clx.ptr(nodes), _clx.ptr(info), _clx.ptr(work), nbytes, st)

    def rows_for(lab, Y, X):
        call(lab, Y, X, None, 0, None, None, maps=False)
        found = info.tolist()
        return (torch.empty((found[0], 13), dtype=torch.int64, device=dev), torch.empty((found[1], 7), dtype=torch.int64, device=dev))

    crop_h = np.ascontiguousarray(skeleton.reshape(size, size)[:512, :512].cpu().numpy())
    crop_d = np.ascontiguousarray(dist.reshape(size, size)[:512, :512].cpu().numpy())
    crop = torch.from_numpy(crop_h).to(dev).reshape(-1)
    cb, cn = rows_for(crop, 512, 512)
    call(crop, 512, 512, torch.from_numpy(crop_d).to(dev).reshape(-1), 3000, cb, cn)
    want = graph(crop_h, crop_d, 3000)
    got_b, got_n = cb.cpu().numpy(), cn.cpu().numpy()
    assert info.tolist() == want["info"], "info differs from the restatement on the crop"
    assert np.array_equal(got_b[np.argsort(got_b[:, 0])], want["branches"]) and np.array_equal(got_n[np.argsort(got_n[:, 0])], want["nodes"])
    assert np.array_equal(branch_map[:512 * 512].cpu().numpy().reshape(512, 512), want["branch_map"])
    assert np.array_equal(out[:512 * 512].cpu().numpy().reshape(512, 512), want["out"])

    branches, nodes = rows_for(skel, size, size)
    words = torch.empty((nid, 10), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)

    def census():
        _clx.call("clx_skeleton_census", _clx.ptr(skel), _clx.ptr(dist), 2, 1, size, size, nid, _clx.ptr(words), _clx.ptr(bad), st)

    call(skel, size, size, None, 3000, branches, nodes)
    pruned = info.tolist()
    emit(f"territories: {size} x {size}, {nobj} objects, thinned: {int((skel != 0).sum().item())} skeleton pixels "
         f"({int((skel != 0).sum().item()) / npix:.2%} of the map), {len(branches)} branches, {len(nodes)} nodes; a limit of 3000 / 1024 pixels "
         f"prunes {pruned[3]} spurs of {pruned[2]} pixels; {repeats} repeats: median (min .. max)")
    rows = (("clx_skeleton_graph, rows and maps", lambda: call(skel, size, size, None, 0, branches, nodes)),
            ("clx_skeleton_graph, rows and maps, with dist_sq", lambda: call(skel, size, size, dist, 0, branches, nodes)),
            ("clx_skeleton_graph, rows and maps, limit 3000", lambda: call(skel, size, size, None, 3000, branches, nodes)),
            ("clx_skeleton_graph, counts only", lambda: call(skel, size, size, None, 0, None, None, maps=False)),
            ("clx_skeleton_census with dist_sq", census))
    for name, run in rows:
        emit(f"  {name:52s} (HIP events) {summary(timed(run, repeats))}")
    emit(f"  workspace {nbytes / 1e6:.1f} MB = {nbytes / npix:.0f} bytes a pixel; no counters were taken; 3-D stacks and unthinned maps were not timed")
    emit("")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_graph needs a HIP device")
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
