"""clx_label_basins, clx_basin_passes and clx_basin_relabel through the C ABI against the restatements of tests/split_ref.py.
Everything is integer work: root, the sorted summit list, the sorted pass table and info must be EQUAL.  Outputs and the
workspace are prefilled with 0xAB bytes and sit between guard words that must stay untouched.

dist_sq is an input of the ABI, so a random integer map gives hundreds of basins and ties on a tiny image.  The kernels'
constants the shapes are chosen by: a block takes tiles of 1024 pixels, at most 1024 blocks (the ascent and the passes) or 4096
blocks of 256 pixels (the roots) a launch, so 1024 * 1024 pixels is both caps; a root launch follows 64 links, so two launches
resolve chains of 65^2 links; a block's table in LDS holds 512 pairs."""

import ctypes

import numpy as np
import pytest
import torch

from inscribed_ref import DIST_INF
from split_ref import NONE, loops_basins, loops_passes, passes_of, ref_basins, ref_passes, ref_up, serpentine
from test_cpu_split import integer_maps
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

TILE, MAX_GRID, LINKS, LDS_PAIRS, MIN_CAPACITY = 1024, 1024, 64, 512, 1024


def _shape3(a):
    return (1,) * (3 - a.ndim) + a.shape


def run_basins(labels, dist, device, capacity=None):
    """-> (root int64 with NONE on background, the list as the entry point left it, info (2,)); the guard words are checked"""
    from cellulus_amd import _clx

    labels, dist = np.ascontiguousarray(labels, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.int32)
    Z, Y, X = _shape3(labels)
    capacity = labels.size if capacity is None else capacity
    nbytes = int(_clx.load().clx_label_basins_workspace(labels.size))
    assert nbytes == 64 + 4 * labels.size
    outs = dict(root=Out(labels.shape, np.int32, device), summits=Out((capacity,), np.uint32, device), info=Out((2,), np.uint32, device),
                workspace=Out((nbytes,), np.uint8, device))
    lab, d = _dev(labels, device), _dev(dist, device)
    status = _clx.load().clx_label_basins(_clx.ptr(lab), _clx.ptr(d), labels.ndim, Z, Y, X, capacity, outs["root"].ptr, outs["summits"].ptr,
                                          outs["info"].ptr, outs["workspace"].ptr, nbytes, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    outs["workspace"].get()
    return outs["root"].get().astype(np.int64), outs["summits"].get().astype(np.int64), outs["info"].get().astype(np.int64)


def run_passes(labels, dist, root, device, capacity=MIN_CAPACITY):
    """-> (rootA, rootB, pass sorted by the key; info (2,))"""
    from cellulus_amd import _clx

    labels, dist = np.ascontiguousarray(labels, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.int32)
    Z, Y, X = _shape3(labels)
    outs = dict(keys=Out((capacity,), np.uint64, device), values=Out((capacity,), np.uint64, device), info=Out((2,), np.int32, device))
    lab, d, r = _dev(labels, device), _dev(dist, device), _dev(np.asarray(root).astype(np.int32), device)
    status = _clx.load().clx_basin_passes(_clx.ptr(lab), _clx.ptr(d), _clx.ptr(r), labels.ndim, Z, Y, X, capacity, outs["keys"].ptr,
                                          outs["values"].ptr, outs["info"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    keys, values, info = outs["keys"].get(), outs["values"].get(), outs["info"].get()
    used = np.flatnonzero(keys)
    assert info[1] == len(used) and (values[keys == 0] == 0).all()
    order = used[np.argsort(keys[used], kind="stable")]
    k = keys[order]
    return ((k >> np.uint64(32)).astype(np.int64), (k & np.uint64(0xFFFFFFFF)).astype(np.int64), values[order].astype(np.int64)), info


def assert_equal(labels, dist, device, basins=loops_basins, passes=lambda *a: passes_of(loops_passes(*a)), capacity=MIN_CAPACITY):
    want_root, want_summits, want_info = basins(labels, dist)
    root, summits, info = run_basins(labels, dist, device)
    assert info[0] == want_info and info[1] == len(want_summits)
    assert np.array_equal(root, want_root), np.argwhere(root != want_root)[:5]
    assert np.array_equal(np.sort(summits[:info[1]]), want_summits)
    got, pinfo = run_passes(labels, dist, root, device, capacity)
    want = passes(labels, dist, want_root)
    assert pinfo[0] == 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
    return root, want_summits, got


@pytest.mark.parametrize("shape", [(5, 3), (7, 1), (6, 2), (1, 9), (9, 11), (4, 5, 3), (3, 4, 1), (2, 3, 7), (1, 1), (1, 1, 1)])
def test_small_widths_against_the_loops(shape, device):
    for seed in range(3):
        labels, dist = integer_maps(shape, 10 * seed + len(shape), labels=2, top=4)
        assert_equal(labels, dist, device)
        assert_equal(np.where(labels == 2, -7, labels), dist, device)          # negative values are objects


def test_row_and_slice_ends_do_not_wrap(device):
    flat = np.zeros((3, 5), np.int32)
    flat[0, 4], flat[1, 0] = 1, 1                               # consecutive in memory, no neighbours
    dist = np.where(flat > 0, np.array([[0, 0, 0, 0, 2], [3, 0, 0, 0, 0], [0] * 5]), 0).astype(np.int32)
    root, summits, passes = assert_equal(flat, dist, device)
    assert summits.tolist() == [4, 5] and len(passes[0]) == 0 and root[0, 4] == 4 and root[1, 0] == 5
    vol = np.zeros((2, 3, 4), np.int32)
    vol[0, 2, 3], vol[1, 0, 0] = 1, 1                           # the last voxel of a slice and the first of the next
    dist = np.where(vol > 0, 1, 0).astype(np.int32)
    dist[1, 0, 0] = 2
    root, summits, passes = assert_equal(vol, dist, device)
    assert summits.tolist() == [11, 12] and len(passes[0]) == 0
    corner = np.zeros((2, 2, 2), np.int32)
    corner[0, 0, 0], corner[1, 1, 1] = 1, 1                     # voxels that share a corner only are neighbours
    for heights in ((1, 1), (1, 2), (2, 1)):
        dist = np.zeros((2, 2, 2), np.int32)
        dist[0, 0, 0], dist[1, 1, 1] = heights
        root, summits, passes = assert_equal(corner, dist, device)
        assert summits.tolist() == [7 if heights == (1, 2) else 0] and len(passes[0]) == 0


def test_touching_objects_of_different_labels(device):
    labels = np.array([[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 3, 3]], np.int32)
    dist = np.array([[1, 2, 9, 1], [1, 1, 1, 1], [1, 2, 3, 8]], np.int32)
    root, summits, passes = assert_equal(labels, dist, device)
    assert summits.tolist() == [1, 2, 11] and len(passes[0]) == 0              # no ascent from label 1 to the 9 next to it, no pass
    assert (root[labels == 1] == 1).all() and (root[labels == 2] == 2).all() and (root[labels == 3] == 11).all()
    split = np.array([[1, 1, 1, 1, 1], [2, 2, 2, 2, 2]], np.int32)
    dist = np.array([[5, 1, 1, 1, 5], [1, 1, 1, 1, 1]], np.int32)
    _, summits, passes = assert_equal(split, dist, device)
    assert summits.tolist() == [0, 4, 5] and [p.tolist() for p in passes] == [[0], [4], [1]]


def test_equal_heights_and_ties(device):
    for shape in ((1, 2), (2, 1), (9, 13), (3, 5, 6)):
        labels = np.full(shape, 4, np.int32)
        for value in (0, 1, DIST_INF):
            root, summits, passes = assert_equal(labels, np.full(shape, value, np.int32), device)
            assert summits.tolist() == [0] and (root == 0).all() and len(passes[0]) == 0
    # two equal peaks next to each other, in both index orders relative to the slope between them
    labels = np.ones((1, 6), np.int32)
    for dist, tops in (([3, 3, 1, 1, 3, 3], [0, 4]), ([1, 3, 3, 1, 3, 3], [1, 4]), ([3, 1, 3, 1, 3, 1], [0, 2, 4]), ([1, 2, 2, 2, 2, 1], [1])):
        root, summits, passes = assert_equal(labels, np.array([dist], np.int32), device)
        assert summits.tolist() == tops
    root, _, passes = assert_equal(labels, np.array([[3, 1, 1, 1, 1, 3]], np.int32), device)
    assert root.tolist() == [[0, 0, 0, 0, 5, 5]] and [p.tolist() for p in passes] == [[0], [5], [1]]     # a flat floor climbs to the left


def test_serpentine_longer_than_two_launches(device):
    labels = serpentine(96)
    # heights that rise along the winding path: the ascent follows it to its end
    path, seen, at = [], np.zeros(labels.shape, bool), (0, 0)
    while at is not None:
        path.append(at)
        seen[at] = True
        y, x = at
        steps = [(y + dy, x + dx) for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)) if 0 <= y + dy < 96 and 0 <= x + dx < 96]
        at = next((q for q in steps if labels[q] and not seen[q]), None)
    assert len(path) == labels.sum()
    dist = np.zeros(labels.shape, np.int32)
    for k, p in enumerate(path):
        dist[p] = k + 1
    up, _, _ = ref_up(labels, dist)
    links, p = 0, 0
    while up[p] != p:
        p, links = up[p], links + 1
    assert links > (LINKS + 1) ** 2                             # more than two root launches resolve
    root, summits, passes = assert_equal(labels, dist, device, basins=ref_basins, passes=ref_passes)
    assert len(summits) == 1 and (root[labels > 0] == summits[0]).all() and len(passes[0]) == 0
    # the same object with equal heights: chains a row long, summits at the row ends
    assert_equal(labels, labels.copy(), device, basins=ref_basins, passes=ref_passes)


def peak_lattice(shape, seed):
    """one object with a peak on every second pixel of every second row over a random floor: a basin per peak, each with
    eight neighbouring basins"""
    dist = np.random.default_rng(seed).integers(1, 4, size=shape).astype(np.int32)
    dist[::2, ::2] = 10
    return np.ones(shape, np.int32), dist


def test_more_pairs_than_the_block_table_and_a_full_global_table(device):
    labels, dist = peak_lattice((32, 32), 7)                    # one tile, one block
    assert labels.size == TILE
    _, _, passes = assert_equal(labels, dist, device, basins=ref_basins, passes=ref_passes, capacity=4096)
    assert len(passes[0]) > LDS_PAIRS
    labels, dist = peak_lattice((72, 70), 8)
    root, _, _ = ref_basins(labels, dist)
    want = ref_passes(labels, dist, root)
    assert len(want[0]) > MIN_CAPACITY
    _, info = run_passes(labels, dist, root, device, MIN_CAPACITY)
    assert info[0] & 4 and info[1] <= MIN_CAPACITY                          # full: the table is to be discarded
    got, info = run_passes(labels, dist, root, device, 16 * MIN_CAPACITY)
    assert info[0] == 0 and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_short_summit_list_and_distance_out_of_range(device):
    labels, dist = integer_maps((12, 17), 9)
    want_root, want_summits, _ = ref_basins(labels, dist)
    assert len(want_summits) > 8
    for capacity in (1, 3, len(want_summits) - 1):
        root, summits, info = run_basins(labels, dist, device, capacity)
        assert info[0] == 4 and info[1] == len(want_summits) and np.array_equal(root, want_root)
        assert len(set(summits.tolist())) == capacity and set(summits.tolist()) <= set(want_summits.tolist())
    root, summits, info = run_basins(labels, dist, device, len(want_summits))
    assert info[0] == 0 and np.array_equal(np.sort(summits), want_summits)
    for value in (-1, DIST_INF + 1, -2 ** 31):
        dirty = dist.copy()
        at = np.argwhere(labels > 0)[[3, -2]]
        dirty[tuple(at.T)] = value
        root, _, _ = assert_equal(labels, dirty, device)
        assert (root[tuple(at.T)] == NONE).all()
        assert run_basins(labels, dirty, device)[2][0] == 2
    dirty = dist.copy()
    dirty[labels == 0] = -5                                     # under background nothing is looked at
    assert run_basins(labels, dirty, device)[2][0] == 0


def test_map_above_the_launch_caps(device):
    shape = (MAX_GRID + 1, TILE)                                # one tile more than a launch of single-tile blocks takes
    rng = np.random.default_rng(5)
    labels = np.kron(rng.integers(0, 4, size=(shape[0] // 25 + 1, shape[1] // 32)), np.ones((25, 32), np.int64))[:shape[0]].astype(np.int32)
    y, x = np.indices(shape)
    dist = (((y % 19) - 9) ** 2 + ((x % 23) - 11) ** 2 + rng.integers(0, 3, size=shape)).astype(np.int32)
    want_root, want_summits, _ = ref_basins(labels, dist)
    want = ref_passes(labels, dist, want_root)
    assert len(want_summits) > 1000 and want_root[-1].max() >= MAX_GRID * TILE          # the last tile has basins of its own
    capacity = 1 << int(4 * len(want[0])).bit_length()
    root, summits, info = run_basins(labels, dist, device)
    assert info.tolist() == [0, len(want_summits)] and np.array_equal(root, want_root)
    assert np.array_equal(np.sort(summits[:info[1]]), want_summits)
    got, pinfo = run_passes(labels, dist, root, device, capacity)
    assert pinfo[0] == 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
    again = run_basins(labels, dist, device)
    assert again[0].tobytes() == root.tobytes() and np.array_equal(np.sort(again[1][:info[1]]), want_summits)
    got_again, _ = run_passes(labels, dist, root, device, capacity)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, got_again))


def run_relabel(root, summits, ids, device):
    from cellulus_amd import _clx

    root = np.ascontiguousarray(root).astype(np.int32)
    nbytes = int(_clx.load().clx_label_basins_workspace(root.size))
    outs = dict(out=Out(root.shape, np.int32, device), bad=Out((1,), np.int32, device), workspace=Out((nbytes,), np.uint8, device))
    r, s, i = _dev(root, device), _dev(np.asarray(summits).astype(np.int32), device), _dev(np.asarray(ids).astype(np.int32), device)
    status = _clx.load().clx_basin_relabel(_clx.ptr(r), root.size, _clx.ptr(s), _clx.ptr(i), len(summits), outs["out"].ptr, outs["bad"].ptr,
                                           outs["workspace"].ptr, nbytes, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    outs["workspace"].get()
    return outs["out"].get(), int(outs["bad"].get()[0])


def test_relabel(device):
    for shape in ((11, 7), (3, 5, 6)):
        labels, dist = integer_maps(shape, 12)
        root, summits, _ = ref_basins(labels, dist)
        ids = np.random.default_rng(3).integers(1, 2 ** 31 - 1, size=len(summits))
        id_of = np.zeros(labels.size + 1, np.int64)
        id_of[summits] = ids
        out, bad = run_relabel(root, summits, ids, device)
        assert bad == 0 and np.array_equal(out, id_of[root.reshape(-1)].reshape(shape))
        out, bad = run_relabel(root, summits[1:], ids[1:], device)            # a root that is not in the list: 0, and reported
        id_of[summits[0]] = 0
        assert bad == 2 and np.array_equal(out, id_of[root.reshape(-1)].reshape(shape))
        out, bad = run_relabel(root, np.r_[summits[1:], labels.size, -1], np.r_[ids[1:], 5, 6], device)    # a summit outside the map
        assert bad == 3 and np.array_equal(out, id_of[root.reshape(-1)].reshape(shape))
    out, bad = run_relabel(np.full((4, 4), NONE), [], [], device)
    assert bad == 0 and (out == 0).all()


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    ins = {k: torch.zeros(64, dtype=torch.int32, device=device) for k in ("labels", "dist_sq", "summits_in", "ids")}
    ins["root_in"] = torch.full((64,), NONE, dtype=torch.int32, device=device)
    outs = dict(root=Out((64,), np.int32, device), summits=Out((16,), np.int32, device), info=Out((2,), np.int32, device),
                workspace=Out((80,), np.int32, device), keys=Out((1024,), np.uint64, device), values=Out((1024,), np.uint64, device),
                out=Out((64,), np.int32, device), bad=Out((1,), np.int32, device))
    null = ctypes.c_void_p(0)
    p = {k: o.ptr for k, o in outs.items()}
    p.update({k: _clx.ptr(t) for k, t in ins.items()})

    def label_basins(nd=2, Z=1, Y=8, X=8, capacity=16, nbytes=320, **ptrs):
        q = dict(p, **ptrs)
        return lib.clx_label_basins(q["labels"], q["dist_sq"], nd, Z, Y, X, capacity, q["root"], q["summits"], q["info"], q["workspace"], nbytes, st)

    def basin_passes(nd=2, Z=1, Y=8, X=8, capacity=1024, **ptrs):
        q = dict(p, **ptrs)
        return lib.clx_basin_passes(q["labels"], q["dist_sq"], q["root_in"], nd, Z, Y, X, capacity, q["keys"], q["values"], q["info"], st)

    def basin_relabel(npix=64, n=4, nbytes=320, **ptrs):
        q = dict(p, **ptrs)
        return lib.clx_basin_relabel(q["root_in"], npix, q["summits_in"], q["ids"], n, q["out"], q["bad"], q["workspace"], nbytes, st)

    shapes = [dict(nd=1), dict(nd=4), dict(Z=2), dict(Y=0), dict(X=-8), dict(nd=3, Z=0), dict(Y=65536, X=65536)]
    odd = ctypes.c_void_p(outs["workspace"].ptr.value + 2)
    refused = [(label_basins, kw) for kw in shapes + [dict(capacity=0), dict(capacity=2 ** 30 + 1), dict(nbytes=319), dict(nbytes=0),
                                                     dict(workspace=odd)]
               + [{k: null} for k in ("labels", "dist_sq", "root", "summits", "info", "workspace")]]
    refused += [(basin_passes, kw) for kw in shapes + [dict(capacity=512), dict(capacity=1536), dict(capacity=2 ** 29)]
                + [{k: null} for k in ("labels", "dist_sq", "root_in", "keys", "values", "info")]]
    refused += [(basin_relabel, kw) for kw in [dict(npix=0), dict(npix=2 ** 32), dict(n=-1), dict(n=2 ** 30 + 1), dict(nbytes=319), dict(workspace=odd)]
                + [{k: null} for k in ("root_in", "summits_in", "ids", "out", "bad", "workspace")]]
    for call, kw in refused:
        name = {label_basins: "clx_label_basins", basin_passes: "clx_basin_passes", basin_relabel: "clx_basin_relabel"}[call]
        assert call(**kw) == -1, f"{name}{kw} was accepted"
        assert lib.clx_last_error().decode().startswith(name + ":"), kw
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert label_basins() == 0 and label_basins(nd=3, Z=2, Y=4) == 0       # the same buffers are accepted with valid arguments
    torch.cuda.synchronize(device)
    assert (outs["root"].get() == NONE).all() and outs["info"].get().tolist() == [0, 0] and outs["summits"].untouched()
    assert basin_passes() == 0 and basin_relabel(n=0, summits_in=null, ids=null) == 0
    torch.cuda.synchronize(device)
    assert (outs["keys"].get() == 0).all() and (outs["values"].get() == 0).all() and (outs["out"].get() == 0).all()
    assert outs["bad"].get()[0] == 0
