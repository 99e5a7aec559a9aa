"""clx_label_holes through the C ABI against the restatement of tests/fill_ref.py (scipy.ndimage.label of the zeros with the
face structure; per component the border test, the dilation ring and the area).  Everything is integer work: out, the hole
rows sorted by their first pixel and info must be EQUAL in every element.  Outputs and the workspace are prefilled with 0xAB
bytes and sit between guard words that must stay untouched.

The constants below mirror csrc/label_holes.hip and csrc/segments.h: a wave takes a SEGMENT of 64 pixels of a row (segments.h);
the first four launches have at most MAX_GRID (there: HOLES_MAX_GRID) blocks of 4 waves, beyond which a wave takes more than one
segment; the last has at most FILL_MAX_GRID blocks, each of which takes 4 x FILL_SEGS segments a trip."""

import ctypes

import numpy as np
import pytest
import torch

from fill_ref import HAND, comb_hole, discs_map, hand_result, random_map, ref_holes, serpentine_hole, spiral_hole
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

SEGMENT, MAX_GRID, WAVES_PER_BLOCK, FILL_MAX_GRID, FILL_SEGS = 64, 2048, 4, 1024, 8


def run_holes(labels, device, max_size=None, planewise=False, capacity=None):
    """one call -> (out, the rows that fit sorted by first, info); the guard words are checked.  capacity None: as many rows as
    the map has pixels"""
    from cellulus_amd import _clx

    labels = np.ascontiguousarray(labels, dtype=np.int32)
    nd = labels.ndim
    Z, Y, X = (1,) * (3 - nd) + labels.shape
    lib = _clx.load()
    lab = _dev(labels, device)
    nbytes = int(lib.clx_label_holes_workspace(nd, Z, Y, X))
    assert nbytes == 16 * labels.size
    capacity = labels.size if capacity is None else capacity
    outs = dict(out=Out(labels.shape, np.int32, device), info=Out((4,), np.int32, device), workspace=Out((nbytes,), np.uint8, device))
    if capacity:
        outs["holes"] = Out((capacity, 4), np.int32, device)
    status = lib.clx_label_holes(_clx.ptr(lab), nd, Z, Y, X, int(planewise), -1 if max_size is None else max_size, capacity, outs["out"].ptr,
                                 outs["holes"].ptr if capacity else ctypes.c_void_p(0), outs["info"].ptr, outs["workspace"].ptr, nbytes,
                                 _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    outs["workspace"].get()
    info = outs["info"].get().tolist()
    rows = outs["holes"].get()[:min(info[0], capacity)].astype(np.int64) if capacity else np.zeros((0, 4), np.int64)
    if capacity > info[0]:
        assert (outs["holes"].get()[info[0]:].view(np.uint8) == 0xAB).all(), "a row beyond the count was written"
    return outs["out"].get(), rows[np.argsort(rows[:, 0], kind="stable")], info


def assert_equal(labels, device, max_size=None, planewise=False, want=None):
    want = ref_holes(labels, max_size, planewise) if want is None else want
    got = run_holes(labels, device, max_size, planewise)
    assert got[2] == want[2], (got[2], want[2])
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), (got[1][:5], want[1][:5])
    return got


@pytest.mark.parametrize("name", sorted(HAND))
def test_maps_worked_by_hand(name, device):
    labels, planewise, out, rows, info = hand_result(name)
    assert_equal(labels, device, planewise=planewise, want=(out, rows, info))
    if labels.ndim == 2:                                                 # the same map as one slice of a planewise stack
        assert_equal(labels[None], device, planewise=True, want=(out[None], rows, info))


@pytest.mark.parametrize("X", (1, 2, 63, 64, 65, 129))
def test_widths_and_heights(X, device):
    for Y in (1, 2, 9):
        for seed in (0, 1):
            labels = random_map((Y, X), 10 * X + seed, block=3)
            assert_equal(labels, device)
            assert_equal(labels, device, max_size=1)
    for shape in ((3, 2, X), (4, 7, X)):
        labels = random_map(shape, X, block=3)
        assert_equal(labels, device)
        assert_equal(labels, device, planewise=True)


def test_holes_at_the_seam_of_two_segments(device):
    for lo, hi in ((60, 70), (60, 63), (64, 68), (63, 64), (1, 128), (0, 127)):       # across, ending on, starting at the seam
        labels = np.ones((3, 130), np.int32)
        labels[1, lo:hi + 1] = 0
        out, rows, info = assert_equal(labels, device)
        if lo:
            assert (out == 1).all() and rows.tolist() == [[130 + lo, 1, hi - lo + 1, 0]] and info == [1, hi - lo + 1, 1, 0]
        else:
            assert np.array_equal(out, labels) and info == [0, 0, 1, 0]
    two = np.ones((4, 130), np.int32)                                    # two runs of one row that meet only through the row below, across the seam
    two[1, 60:63], two[1, 66:70], two[2, 60:70] = 0, 0, 0
    assert assert_equal(two, device)[2] == [1, 17, 1, 0]
    late = np.ones((5, 140), np.int32)                                   # the first pixel lies in a later segment than the widest row
    late[1, 70], late[2, 5:76], late[3, 30] = 0, 0, 0
    assert assert_equal(late, device)[1].tolist() == [[140 + 70, 1, 73, 0]]


def test_chains_and_late_merges(device):
    for m in (comb_hole(), spiral_hole(), serpentine_hole(), comb_hole(7, 70).T.copy(), serpentine_hole(4, 67).T.copy()):
        out, rows, info = assert_equal(m, device)
        assert (out == 1).all() and info == [1, int((m == 0).sum()), 1, 0]
    opened = serpentine_hole()
    opened[-2, -1] = 0                                                   # the far end of the corridor reaches the border
    assert assert_equal(opened, device)[2] == [0, 0, 1, 0]
    vol = np.ones((5, 12, 70), np.int32)                                 # a comb along z: plates that meet in the last slice but one
    vol[1:4, 1:11, 2:68:2] = 0
    vol[3, 1:11, 2:68] = 0
    out, rows, info = assert_equal(vol, device)
    assert (out == 1).all() and info[0] == 1 and info[2] == 1
    assert assert_equal(vol, device, planewise=True)[2][0] == 33 + 33 + 1


def test_size_cap(device):
    labels, _, out, _, _ = hand_result("one_side_each")                  # one hole of 3 pixels
    for max_size, kept in ((2, 1), (3, 0), (4, 0), (0, 1), (None, 0), (2 ** 40, 0)):
        got = assert_equal(labels, device, max_size)
        assert np.array_equal(got[0], labels if kept else out) and got[1].tolist() == [[24, 1, 3, kept]] and got[2][1] == (0 if kept else 3)
    many = discs_map((48, 56), 3)
    census = assert_equal(many, device, max_size=0)
    assert np.array_equal(census[0], many) and census[1][:, 3].all() and census[2][1] == 0 and census[2][0] > 20
    sizes = np.unique(census[1][:, 2])
    assert len(sizes) >= 3
    for cap in (int(sizes[1]) - 1, int(sizes[1]), int(sizes[1]) + 1):
        got = assert_equal(many, device, max_size=cap)
        assert np.array_equal(got[1][:, 3], (got[1][:, 2] > cap).astype(np.int64)) and got[1][:, 3].any() and not got[1][:, 3].all()


def test_capacity(device):
    labels = discs_map((48, 56), 5)
    want = ref_holes(labels)
    n = want[2][0]
    assert n > 20
    for capacity in (0, 1, n - 1, n, n + 3):
        out, rows, info = run_holes(labels, device, capacity=capacity)
        assert info == want[2] and np.array_equal(out, want[0])           # the count is exact and out complete, whatever fits
        assert len(rows) == min(n, capacity) and len(np.unique(rows[:, 0])) == len(rows)
        assert all(r in want[1].tolist() for r in rows.tolist())
        if capacity >= n:
            assert np.array_equal(rows, want[1])


def test_3d_maps(device):
    for seed in range(3):
        for shape in ((6, 9, 70), (3, 20, 20), (9, 5, 5)):
            labels = random_map(shape, 50 + seed, block=3, knock=0.3)
            assert_equal(labels, device)
            assert_equal(labels, device, max_size=2, planewise=True)
    balls = discs_map((9, 40, 44), 2)
    assert assert_equal(balls, device)[2][0] > 20


def test_more_segments_than_waves_and_two_runs(device):
    shape = (MAX_GRID * WAVES_PER_BLOCK + 1, SEGMENT)                    # one wave makes a second trip in every launch
    labels = random_map(shape, 8, block=5, knock=0.1)
    labels[-3:, :] = 7
    labels[-2, 20:40] = 0                                                # a hole under the segment of the second trip ...
    labels[-2, 45:56], labels[-1, 50] = 0, 0                             # ... and zeros that reach the border only through that segment
    first = assert_equal(labels, device)
    assert first[2][0] > 1000 and first[1][-1].tolist() == [(shape[0] - 2) * SEGMENT + 20, 7, 20, 0] and not first[0][-2, 45:56].any()
    second = run_holes(labels, device)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2]
    # the last launch: one segment more than its blocks take in a trip, on a map three pixels wide
    tall = np.ones((FILL_MAX_GRID * WAVES_PER_BLOCK * FILL_SEGS + 1, 3), np.int32)
    tall[1:-1:2, 1] = 0                                                  # a pinhole in every other row; the last one in the last row but one
    tall[5, 0], tall[-4, 2] = 0, 0                                       # two of them open to the side
    out, rows, info = assert_equal(tall, device)
    n = (tall.shape[0] - 1) // 2
    assert info == [n - 2, n - 2, n, 0] and rows[-1].tolist() == [(tall.shape[0] - 2) * 3 + 1, 1, 1, 0] and out[5, 1] == 0 == out[-4, 1]


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    labels = torch.ones(64, dtype=torch.int32, device=device)
    labels[27] = 0
    exact = int(lib.clx_label_holes_workspace(2, 1, 8, 8))
    assert exact == int(lib.clx_label_holes_workspace(3, 2, 4, 8)) == 16 * 64
    outs = dict(out=Out((64,), np.int32, device), holes=Out((4, 4), np.int32, device), info=Out((4,), np.int32, device),
                workspace=Out((exact,), np.uint8, device))
    null = ctypes.c_void_p(0)

    def holes(nd=2, Z=1, Y=8, X=8, planewise=0, max_size=-1, capacity=4, nbytes=exact, **ptrs):
        p = {k: o.ptr for k, o in outs.items()}
        p.update(labels=_clx.ptr(labels))
        p.update(ptrs)
        return lib.clx_label_holes(p["labels"], nd, Z, Y, X, planewise, max_size, capacity, p["out"], p["holes"], p["info"], p["workspace"], nbytes, st)

    refused = [dict(nd=1), dict(nd=4), dict(Z=2), dict(Y=0), dict(X=-8), dict(nd=3, Z=0), dict(planewise=1), dict(planewise=2, nd=3, Z=2, Y=4),
               dict(planewise=-1, nd=3, Z=2, Y=4), dict(max_size=-2), dict(capacity=-1), dict(Y=32768, X=65536, nbytes=2 ** 40),
               dict(nd=3, Z=2, Y=32768, X=32768, nbytes=2 ** 40), dict(nbytes=exact - 1), dict(nbytes=0), dict(Y=16, nbytes=exact),
               dict(workspace=ctypes.c_void_p(outs["workspace"].ptr.value + 2)), dict(out=_clx.ptr(labels)), dict(holes=null)]
    refused += [{k: null} for k in ("labels", "out", "info", "workspace")]
    for kw in refused:
        assert holes(**kw) == -1, f"{kw} was accepted"
        assert lib.clx_last_error().decode().startswith("clx_label_holes:"), kw
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert labels.sum().item() == 63
    for kw in (dict(), dict(holes=null, capacity=0), dict(nd=3, Z=1), dict(nd=3, Z=1, planewise=1)):      # the same buffers, valid arguments
        assert holes(**kw) == 0
        torch.cuda.synchronize(device)
        filled = kw.get("nd") != 3 or kw.get("planewise") == 1            # one slice without planewise: z = 0 is the border
        assert outs["info"].get().tolist() == [int(filled), int(filled), 1, 0]
        assert outs["out"].get().sum() == 63 + int(filled)
    assert outs["holes"].get()[0].tolist() == [27, 1, 1, 0]
    assert holes(nd=3, Z=2, Y=4) == 0
    torch.cuda.synchronize(device)
    outs["workspace"].get()
