"""clx_skeleton_graph through the C ABI against the restatement of tests/skeleton_graph_ref.py.  Everything is integers: the
branch rows and the node rows (sorted by first: their order is unspecified), every element of branch_map and out, and info must
be EQUAL.  Outputs and the workspace are prefilled with 0xAB bytes and sit between guard words that must stay untouched; rows
beyond the counts must stay untouched too.

The constants below mirror csrc/skeleton_graph.hip and csrc/segments.h: a wave owns a SEGMENT, 64 consecutive pixels of a row,
a block four segments (segments.h); the plain launches have at most 2048 blocks (8192 segments a trip), the emit launch at most
1024 blocks whose waves take 8 segments a trip (32768 segments)."""

import ctypes

import numpy as np
import pytest
import torch

from skeleton_graph_ref import CYCLE, END_END, JUNCTION_JUNCTION, SPUR, graph, prune_q10
from skeleton_ref import DIST_INF, noise_map, skeleton
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

SEGMENT, PLAIN_SEGMENTS, EMIT_SEGMENTS = 64, 2048 * 4, 1024 * 4 * 8
_REF = {}


def ref(key, make):
    """a reference computed once per key and left unchanged"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def run_graph(labels, device, dist=None, limit=0, capacity=None, want_map=True, want_out=True, spare=3):
    """one clx_skeleton_graph call -> dict as skeleton_graph_ref.graph's; ``capacity`` (branches, nodes), None: ``spare`` rows
    more than a first call with capacity 0 finds"""
    from cellulus_amd import _clx

    lib = _clx.load()
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    nd = labels.ndim
    Z, Y, X = (1,) * (3 - nd) + labels.shape
    lab = _dev(labels, device)
    dist_d = None if dist is None else _dev(np.ascontiguousarray(dist, dtype=np.int32), device)
    nbytes = int(lib.clx_skeleton_graph_workspace(nd, Z, Y, X))
    assert nbytes == 40 * labels.size
    workspace = Out((nbytes,), np.uint8, device)

    def call(capacity_b, capacity_n):
        branch_map, out = (Out(labels.shape, np.int32, device) if w else None for w in (want_map, want_out))
        branches, nodes, info = Out((capacity_b, 13), np.int64, device), Out((capacity_n, 7), np.int64, device), Out((6,), np.int32, device)
        status = lib.clx_skeleton_graph(_clx.ptr(lab), _clx.ptr(dist_d), nd, Z, Y, X, limit, capacity_b, capacity_n,
                                        branch_map.ptr if want_map else None, out.ptr if want_out else None, branches.ptr, nodes.ptr, info.ptr,
                                        workspace.ptr, nbytes, _clx.stream_ptr(device))
        assert status == 0, lib.clx_last_error()
        torch.cuda.synchronize(device)
        workspace.get()
        return branch_map, out, branches.get(), nodes.get(), info.get().tolist()

    if capacity is None:
        found = call(0, 0)[4]
        capacity = found[0] + spare, found[1] + spare
    branch_map, out, branches, nodes, info = call(*capacity)
    kept_b, kept_n = min(info[0], capacity[0]), min(info[1], capacity[1])
    assert (branches[kept_b:].view(np.uint8) == 0xAB).all() and (nodes[kept_n:].view(np.uint8) == 0xAB).all()
    branches, nodes = branches[:kept_b], nodes[:kept_n]
    return {"branches": branches[np.argsort(branches[:, 0], kind="stable")], "nodes": nodes[np.argsort(nodes[:, 0], kind="stable")],
            "branch_map": branch_map.get() if want_map else None, "out": out.get() if want_out else None, "info": info}


def assert_graph(labels, device, dist=None, limit=0, key=None):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    want = ref(key, lambda: graph(labels, dist, limit)) if key else graph(labels, dist, limit)
    got = run_graph(labels, device, dist, limit)
    assert got["info"] == want["info"]
    for name in ("branches", "nodes", "branch_map", "out"):
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:5])
    return got


@pytest.mark.parametrize("Y", (1, 2, 3))
def test_widths_1_to_67(Y, device):
    rng = np.random.default_rng(Y)
    for X in range(1, 68):
        assert_graph(np.where(rng.random((Y, X)) < 0.55, rng.integers(1, 3, (Y, X)), 0), device, limit=1500)
        assert_graph(np.full((Y, X), 3, np.int32), device)


def test_objects_across_segment_and_block_seams(device):
    labels = np.zeros((12, 600), np.int32)
    labels[1, 60:70] = 1                                  # across the seam at x = 64
    labels[3, 10:590] = 2                                 # across the four segments of a block and into the next blocks
    labels[2, 63], labels[4, 64], labels[2, 255], labels[4, 256], labels[2, 320] = 2, 2, 2, 2, 2      # spurs at the seams
    labels[6:10, 126:130] = 3                             # an unthinned block over the seam at x = 128
    for k in range(8):
        labels[11 - k % 2, 188 + k] = 4                   # a zigzag of diagonal links over the seam at x = 192
    labels[5, 63], labels[6, 64], labels[7, 63] = 5, 5, 5  # diagonal links that cross the seam both ways
    got = assert_graph(labels, device, limit=1025)
    assert set(got["branches"][:, 1].tolist()) == {1, 2, 3, 4, 5} and got["info"][3] == 5


def test_row_and_slice_ends_do_not_wrap(device):
    for X in (2, 6, 64, 65, 128):
        labels = np.zeros((6, X), np.int32)
        labels[0, X - 1], labels[1, 0], labels[2, X - 1], labels[3, 0], labels[3, X - 1], labels[4, 0] = 1, 1, 1, 1, 1, 1
        got = assert_graph(labels, device)
        wide = np.pad(labels, ((0, 0), (3, 3)))
        assert got["info"][:2] == graph(wide)["info"][:2]
    stack = np.zeros((3, 4, 5), np.int32)                  # the last row of a slice and the first of the next
    stack[0, 3, :], stack[1, 0, :], stack[1, 3, 4], stack[2, 0, 0] = 1, 1, 1, 1
    got = assert_graph(stack, device)
    assert got["info"][:2] == [2, 6]


def test_3d_stack_equals_its_slices(device):
    stack = ref("stack", lambda: skeleton(noise_map((3, 40, 70), 5, block=11, sigma=1.5)))
    got = assert_graph(stack, device, key="stack graph")
    plane = 40 * 70
    rows_b, rows_n = [], []
    for z in range(3):
        one = run_graph(stack[z], device)
        b, n = one["branches"].copy(), one["nodes"].copy()
        b[:, 0] += z * plane
        b[:, 6:10] += np.where(b[:, 6:10] >= 0, z * plane, 0)
        n[:, 0] += z * plane
        rows_b.append(b)
        rows_n.append(n)
        m = one["branch_map"]
        assert np.array_equal(got["branch_map"][z], m + z * plane * np.sign(m))
    assert np.array_equal(got["branches"], np.concatenate(rows_b)) and np.array_equal(got["nodes"], np.concatenate(rows_n))


def test_label_values_and_touching_labels(device):
    base = np.zeros((6, 70), np.int32)
    base[1, 2:68], base[2, 2:68], base[3, 30], base[0, 40], base[4, 10:20] = 1, 2, 2, 1, 1
    ordered = assert_graph(base, device, limit=2000)
    swapped = assert_graph(np.where(base == 1, 2, np.where(base == 2, 1, 0)), device, limit=2000)
    assert np.array_equal(ordered["branches"][:, 2:], swapped["branches"][:, 2:]) and np.array_equal(ordered["branch_map"], swapped["branch_map"])
    for lo, hi in ((-1, -2), (-2 ** 31, 2 ** 31 - 1), (2 ** 24, 1)):
        extreme = assert_graph(np.where(base == 1, lo, np.where(base == 2, hi, 0)), device, limit=2000)
        assert np.array_equal(ordered["branches"][:, 2:], extreme["branches"][:, 2:]) and set(extreme["nodes"][:, 1].tolist()) == {lo, hi}


def one_pixel_serpentine(Y, X):
    out = np.zeros((Y, X), np.int32)
    for k, y in enumerate(range(1, Y - 1, 2)):
        out[y, 1:X - 1] = 7
        if y + 2 < Y - 1:
            out[y + 1, X - 2 if k % 2 == 0 else 1] = 7
    return out


def test_union_find_stress(device):
    labels = one_pixel_serpentine(130, 200)                # one branch: a chain of unions over many blocks
    got = assert_graph(labels, device, key="serpentine")
    assert got["info"][:2] == [1, 2] and got["branches"][0, 2] == END_END and got["branches"][0, 3] == int((labels != 0).sum()) - 2
    ring = np.zeros((130, 330), np.int32)                  # a ring over five seams and many rows
    ring[5, 30:300], ring[120, 30:300], ring[5:121, 30], ring[5:121, 299] = 1, 1, 1, 1
    got = assert_graph(ring, device, key="ring")
    assert got["info"][:2] == [1, 0] and got["branches"][0, 2] == CYCLE and got["branches"][0, 6:10].tolist() == [-1] * 4
    lattice = np.zeros((100, 200), np.int32)               # many junction - junction branches
    lattice[4::8, 2:198], lattice[2:98, 4::8] = 2, 2
    got = assert_graph(lattice, device, key="lattice", limit=3000)
    assert (got["branches"][:, 2] == JUNCTION_JUNCTION).sum() > 400 and (got["branches"][:, 2] == SPUR).sum() > 50
    blob = noise_map((70, 150), 9, block=20, sigma=2.0)    # unthinned: large clusters of junction pixels, cycles of 2 x 2 blocks
    got = assert_graph(blob, device, key="blob", limit=4000)
    assert got["nodes"][:, 3].max() > 100


@pytest.mark.parametrize("seed", range(4))
def test_thinned_noise_maps(seed, device):
    skel = ref(("skel", seed), lambda: skeleton(noise_map((60, 75), seed, block=13, sigma=1.5)))
    got = assert_graph(skel, device, key=("noise", seed))
    assert got["info"][0] > 50
    spurs = got["branches"][got["branches"][:, 2] == SPUR]
    lengths = np.unique(spurs[:, 4] * 1024 + spurs[:, 5] * 1448)
    between = int(lengths[len(lengths) // 2]) + 300       # between two spur lengths
    pruned = assert_graph(skel, device, limit=between, key=("noise pruned", seed))
    assert 0 < pruned["info"][3] < (got["branches"][:, 2] == SPUR).sum() and pruned["info"][2] >= pruned["info"][3]
    everything = assert_graph(skel, device, limit=(1 << 30) - 1, key=("noise bare", seed))
    assert everything["info"][3] == (got["branches"][:, 2] == SPUR).sum()
    again = assert_graph(pruned["out"], device, limit=between)                    # a second round is a second call on out
    assert again["info"][1] < got["info"][1]


def test_capacities(device):
    skel = ref(("skel", 0), lambda: skeleton(noise_map((60, 75), 0, block=13, sigma=1.5)))
    want = ref(("noise limit", 0), lambda: graph(skel, None, 2500))
    nb, nn = want["info"][:2]
    full = run_graph(skel, device, limit=2500, capacity=(nb, nn))
    assert np.array_equal(full["branches"], want["branches"]) and np.array_equal(full["nodes"], want["nodes"])
    for capacity in ((0, 0), (nb - 1, nn), (nb, nn - 1), (nb - 1, nn - 1), (nb + 5, nn + 1), (1, 0), (0, 1)):
        got = run_graph(skel, device, limit=2500, capacity=capacity)
        assert got["info"] == want["info"]
        assert np.array_equal(got["branch_map"], want["branch_map"]) and np.array_equal(got["out"], want["out"])
        assert len(got["branches"]) == min(nb, capacity[0]) and len(got["nodes"]) == min(nn, capacity[1])
        for rows, every in ((got["branches"], want["branches"]), (got["nodes"], want["nodes"])):      # the rows kept are rows of the graph
            assert len(np.unique(rows[:, 0])) == len(rows)
            assert np.array_equal(rows, every[np.isin(every[:, 0], rows[:, 0])])
    lean = run_graph(skel, device, limit=0, capacity=(nb, nn), want_map=False, want_out=False)
    assert lean["info"][:2] == [nb, nn] and lean["info"][2:] == [0, 0, 0, 0]
    only_map = run_graph(skel, device, limit=0, capacity=(0, 0), want_out=False)
    assert np.array_equal(only_map["branch_map"], want["branch_map"])


@pytest.mark.parametrize("shape", [(PLAIN_SEGMENTS + 1, 3), (EMIT_SEGMENTS + 1, 2)])
def test_one_segment_more_than_a_launch_takes(shape, device):
    rng = np.random.default_rng(shape[0])
    labels = np.where(rng.random(shape) < 0.45, 1, 0).astype(np.int32)
    labels[-1, :] = 1                                      # the last segment has rows of its own
    first = assert_graph(labels, device, limit=2500, key=("cap", shape))
    second = run_graph(labels, device, limit=2500)
    assert all(first[name].tobytes() == second[name].tobytes() for name in ("branches", "nodes", "branch_map", "out")) and first["info"] == second["info"]
    assert first["branches"][-1, 0] >= labels.size - 2 * shape[1] or first["nodes"][-1, 0] >= labels.size - shape[1]


def test_dist_sq_words_and_the_bad_bit(device):
    skel = ref(("skel", 1), lambda: skeleton(noise_map((60, 75), 1, block=13, sigma=1.5)))
    rng = np.random.default_rng(3)
    dist = rng.integers(0, DIST_INF, skel.shape).astype(np.int32)
    clean = assert_graph(skel, device, dist=dist)
    assert clean["info"][4] == 0 and (clean["branches"][:, 12] >= 0).sum() > 50
    assert (clean["branches"][clean["branches"][:, 3] == 0][:, 10:] == [0, DIST_INF, -1]).all()
    first = int(clean["branches"][clean["branches"][:, 3] > 1][0, 0])
    for value in (-1, DIST_INF, -2 ** 31):
        spoilt = dist.copy()
        spoilt.reshape(-1)[first] = value
        got = assert_graph(skel, device, dist=spoilt)
        assert got["info"][4] == 2 and got["branches"][got["branches"][:, 0] == first][0, 10] == clean["branches"][clean["branches"][:, 0] == first][0, 10] - dist.reshape(-1)[first]
    spoilt = dist.copy()
    spoilt[clean["branch_map"] <= 0] = -1                  # bad values under background and node pixels are not looked at
    assert assert_graph(skel, device, dist=spoilt)["info"][4] == 0
    without = assert_graph(skel, device, key=("noise", 1))
    assert (without["branches"][:, 10:] == [0, DIST_INF, -1]).all() and np.array_equal(without["branches"][:, :10], clean["branches"][:, :10])


def test_prune_limits(device):
    wye = np.zeros((9, 70), np.int32)
    for k in range(1, 4):
        wye[4 - k, 64 + k] = 1                             # three diagonal links
    wye[4, 60:65], wye[5, 64], wye[6, 64] = 1, 1, 1        # four face links to the left, two down
    lengths = {2048: (2, 1), 4096: (4, 1), prune_q10(3 * 2 ** 0.5) - 1: (3, 1)}      # the largest limits that keep each arm
    assert sorted(lengths) == [2048, 4096, 4344]
    want_pixels = 0
    for spurs, limit in enumerate(sorted(lengths)):
        below, above = assert_graph(wye, device, limit=limit), assert_graph(wye, device, limit=limit + 1)
        assert below["info"][2:4] == [want_pixels, spurs] and above["info"][2:4] == [want_pixels + lengths[limit][0], spurs + 1]
        want_pixels += lengths[limit][0]
        assert above["out"][4, 64] == 1
    nothing = assert_graph(wye, device, limit=0)
    assert np.array_equal(nothing["out"], wye) and nothing["info"][2:4] == [0, 0]
    bare = assert_graph(wye, device, limit=(1 << 30) - 1)
    assert int((bare["out"] != 0).sum()) == 1
    plus = np.zeros((5, 5), np.int32)
    plus[2, 1:4], plus[1, 2], plus[3, 2] = 1, 1, 1
    assert assert_graph(plus, device, limit=1024)["info"][2:4] == [0, 0] and assert_graph(plus, device, limit=1025)["info"][2:4] == [4, 4]
    cross = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]], np.int32)
    assert assert_graph(cross, device, limit=1448)["info"][2:4] == [0, 0] and assert_graph(cross, device, limit=1449)["info"][2:4] == [4, 4]


def test_every_rejected_argument(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    labels = _dev(np.ones((4, 6), np.int32), device)
    nbytes = int(lib.clx_skeleton_graph_workspace(2, 1, 4, 6))
    outs = {name: Out(shape, dtype, device) for name, shape, dtype in (("branch_map", (4, 6), np.int32), ("out", (4, 6), np.int32),
            ("branches", (4, 13), np.int64), ("nodes", (4, 7), np.int64), ("info", (6,), np.int32), ("workspace", (nbytes + 8,), np.uint8))}
    good = {"labels": _clx.ptr(labels), "dist": None, "nd": 2, "Z": 1, "Y": 4, "X": 6, "limit": 0, "capacity_b": 4, "capacity_n": 4,
            "branch_map": outs["branch_map"].ptr, "out": outs["out"].ptr, "branches": outs["branches"].ptr, "nodes": outs["nodes"].ptr,
            "info": outs["info"].ptr, "workspace": outs["workspace"].ptr, "nbytes": nbytes}
    off = ctypes.c_void_p(outs["workspace"].ptr.value + 4)
    cases = [({"labels": None}, "null pointer"), ({"info": None}, "null pointer"), ({"workspace": None}, "null pointer"),
             ({"branches": None}, "null branches with capacity_b > 0"), ({"nodes": None}, "null nodes with capacity_n > 0"),
             ({"capacity_b": -1}, "capacity_b and capacity_n must be >= 0"), ({"capacity_n": -1}, "capacity_b and capacity_n must be >= 0"),
             ({"nd": 1}, "nd must be 2 or 3"), ({"nd": 4}, "nd must be 2 or 3"), ({"Z": 2}, "nd == 2 needs Z == 1"), ({"Y": 0}, "bad shape"),
             ({"X": -1}, "bad shape"), ({"nd": 3, "Z": 0}, "bad shape"),
             ({"nd": 3, "Z": 1 << 11, "Y": 1 << 10, "X": 1 << 10}, "Z * Y * X must be below 2^31"),
             ({"limit": -1}, "limit_q10 must lie in [0, 2^30)"), ({"limit": 1 << 30}, "limit_q10 must lie in [0, 2^30)"),
             ({"limit": 5, "out": None}, "null out with limit_q10 > 0"),
             ({"nbytes": nbytes - 1}, "workspace_bytes is below clx_skeleton_graph_workspace(nd, Z, Y, X)"),
             ({"workspace": off}, "workspace must be 8-byte aligned"),
             ({"out": _clx.ptr(labels)}, "in-place operation is not supported"), ({"branch_map": _clx.ptr(labels)}, "in-place operation is not supported"),
             ({"out": outs["branch_map"].ptr}, "out and branch_map must not be one buffer")]
    for change, message in cases:
        args = {**good, **change}
        status = lib.clx_skeleton_graph(*args.values(), _clx.stream_ptr(device))
        error = lib.clx_last_error().decode()
        assert status == -1 and error.startswith("clx_skeleton_graph: ") and message in error, (change, error)
    torch.cuda.synchronize(device)
    assert all(o.untouched() for o in outs.values())      # refused before any launch
    for change in ({"branches": None, "capacity_b": 0}, {"nodes": None, "capacity_n": 0}, {"branch_map": None}, {"out": None}, {"limit": (1 << 30) - 1}):
        assert lib.clx_skeleton_graph(*{**good, **change}.values(), _clx.stream_ptr(device)) == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    assert outs["info"].get().tolist() == graph(np.ones((4, 6), np.int32), None, (1 << 30) - 1)["info"]
