"""clx_label_nearest through the C ABI against the restatements of tests/nearest_ref.py (the minimum of (d², id) over all pairs
of a pixel and an object pixel; for the large maps over a k-d tree's candidates).  Everything is integer work: nearest, dist_sq
and bad must be EQUAL in every element.  Outputs and the workspace are prefilled with 0xAB bytes and sit between guard words
that must stay untouched.

The kernel's row pass takes a row in segments of 64 pixels (a wave), so its seams lie at x = 64, 128, ...: the widths 63, 64,
65 are one segment and one pixel either side, 255, 256, 257 four segments and one pixel either side, 600 ten segments with a
last one of 24.  Its passes along y and z run at most 4096 blocks of 256 pixels a trip (1 048 576 pixels), its row pass at most
4096 blocks of 4 rows (16 384 rows)."""

import itertools

import numpy as np
import pytest
import torch

from nearest_ref import DIST_INF, dots_map, ref_nearest, ref_nearest_tree
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 600)
PASS_CAP_PIXELS, ROW_CAP_ROWS = 4096 * 256, 4096 * 4


def run_nearest(labels, nid, limit_sq, device):
    """-> (nearest, dist_sq, bad) as the entry point left them; the guard words are checked"""
    from cellulus_amd import _clx

    labels = np.ascontiguousarray(labels, dtype=np.int32)
    Z, Y, X = (1,) * (3 - labels.ndim) + labels.shape
    lab = _dev(labels, device)
    nbytes = int(_clx.load().clx_label_nearest_workspace(labels.size))
    assert nbytes == 8 * labels.size
    outs = dict(nearest=Out(labels.shape, np.int32, device), dist_sq=Out(labels.shape, np.int32, device), bad=Out((1,), np.int32, device),
                workspace=Out((nbytes,), np.uint8, device))
    status = _clx.load().clx_label_nearest(_clx.ptr(lab), labels.ndim, Z, Y, X, nid, limit_sq, outs["nearest"].ptr, outs["dist_sq"].ptr,
                                           outs["bad"].ptr, outs["workspace"].ptr, nbytes, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    outs["workspace"].get()
    return outs["nearest"].get(), outs["dist_sq"].get(), int(outs["bad"].get()[0])


def assert_equal(labels, device, nid=None, limit_sq=-1, ref=ref_nearest):
    nid = int(np.max(labels)) + 1 if nid is None else nid
    got = run_nearest(labels, nid, limit_sq, device)
    want = ref(labels, nid, limit_sq)
    assert got[2] == want[2]
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    return got


def seam_row_map(rows, X):
    """object pixels at both ends of a row, at every seam of the 64-pixel segments and one pixel either side of it, spread over
    the rows with ids that fall and rise along x; the rows between stay empty"""
    lab = np.zeros((rows, X), np.int32)
    marks = sorted({x for s in range(0, X + 64, 64) for x in (s - 1, s, s + 1) if 0 <= x < X} | {0, X - 1})
    for k, x in enumerate(marks):
        lab[(k % 2) * (rows - 1), x] = 1 + (5 * k + 3) % 11
    return lab


@pytest.mark.parametrize("X", WIDTHS)
def test_row_ends_and_seams(X, device):
    for rows in (1, 3):
        lab = seam_row_map(rows, X)
        assert_equal(lab, device)
        assert_equal(lab, device, limit_sq=4)
        for x in sorted({0, X - 1, min(X - 1, 63), min(X - 1, 64), X // 2}):       # one object pixel: every other one looks one way
            one = np.zeros((rows, X), np.int32)
            one[rows - 1, x] = 3
            assert_equal(one, device)
    far = np.zeros((2, X), np.int32)                            # the nearest object pixel lies segments away, on either side
    far[0, 0], far[1, X - 1] = 2, 1
    assert_equal(far, device)


def test_empty_rows_slices_and_maps(device):
    lab = np.zeros((12, 70), np.int32)
    lab[0, 3:6], lab[10, 66:70], lab[10, 0] = 2, 1, 3           # rows 1 .. 9 and 11 are empty
    assert_equal(lab, device)
    vol = np.zeros((6, 9, 70), np.int32)
    vol[1, 2, 60:68], vol[4, 7, 1:3] = 1, 2                     # slices 0, 2, 3 and 5 are empty
    assert_equal(vol, device)
    for shape in ((7, 9), (3, 4, 70), (1, 1), (1, 1, 1)):
        nearest, dist, bad = assert_equal(np.zeros(shape, np.int32), device, nid=1)
        assert (nearest == 0).all() and (dist == DIST_INF).all() and bad == 0
        nearest, dist, bad = assert_equal(np.full(shape, 6, np.int32), device)
        assert (nearest == 6).all() and (dist == 0).all()
    for shape in ((9, 67), (3, 5, 66)):
        for corner in itertools.product(*[(0, s - 1) for s in shape]):
            lab = np.zeros(shape, np.int32)
            lab[corner] = 4
            nearest, dist, _ = assert_equal(lab, device)
            assert (nearest == 4).all() and dist.max() == sum((s - 1) ** 2 for s in shape)


TIES = {                                                        # (shape, the two or three object pixels, the tied pixel)
    "x": ((3, 9), [(1, 2), (1, 6)], (1, 4)),
    "y": ((9, 3), [(2, 1), (6, 1)], (4, 1)),
    "z": ((7, 4, 5), [(1, 2, 2), (5, 2, 2)], (3, 2, 2)),
    "diagonal": ((5, 5), [(0, 0), (4, 4)], (0, 4)),
    "3-4 against 5-0": ((12, 12), [(8, 9), (10, 5)], (5, 5)),
    "three-way": ((12, 12), [(5, 0), (0, 5), (8, 9)], (5, 5)),
}


@pytest.mark.parametrize("name", sorted(TIES))
def test_ties_go_to_the_smaller_id(name, device):
    shape, pixels, tied = TIES[name]
    for ids in itertools.permutations((3, 7, 5)[:len(pixels)]):               # the larger id first in raster order, and swapped
        lab = np.zeros(shape, np.int32)
        for p, i in zip(pixels, ids):
            lab[p] = i
        distances = {sum((a - b) ** 2 for a, b in zip(p, tied)) for p in pixels}
        assert len(distances) == 1
        nearest, dist, _ = assert_equal(lab, device)
        assert nearest[tied] == min(ids) and dist[tied] == distances.pop()


def test_limits(device):
    lab = np.zeros((20, 21), np.int32)
    lab[8, 9], lab[17:19, 1:3] = 2, 1
    at = lambda dy, dx: (8 + dy, 9 + dx)                        # noqa: E731
    for limit_sq in (-1, 0, 1, 25, 24, 26, 2 ** 30 - 1):
        nearest, dist, bad = assert_equal(lab, device, limit_sq=limit_sq)
        assert bad == 0 and nearest[8, 9] == 2 and dist[8, 9] == 0
        if limit_sq >= 0:
            assert ((dist <= limit_sq) | (dist == DIST_INF)).all() and ((nearest == 0) == (dist == DIST_INF)).all()
    nearest, dist, _ = run_nearest(lab, 3, 25, device)
    for inside in (at(3, 4), at(-4, 3), at(5, 0), at(0, -5)):
        assert nearest[inside] == 2 and dist[inside] == 25
    for outside in (at(5, 1), at(-1, 5), at(4, 4)):             # the next ring
        assert nearest[outside] == 0 and dist[outside] == DIST_INF
    nearest, dist, _ = run_nearest(lab, 3, 24, device)
    for outside in (at(3, 4), at(5, 0)):
        assert nearest[outside] == 0 and dist[outside] == DIST_INF
    assert nearest[at(2, 4)] == 2 and dist[at(2, 4)] == 20
    nearest, dist, _ = run_nearest(lab, 3, 0, device)
    assert np.array_equal(nearest, lab) and np.array_equal(dist == 0, lab > 0)


def test_3d_objects_that_differ_in_z(device):
    vol = np.zeros((5, 20, 24), np.int32)
    vol[0, 4:9, 5:11], vol[4, 4:9, 5:11], vol[2, 14:16, 18:20] = 2, 1, 3            # the same box in slices 0 and 4: slice 2 ties
    nearest, dist, _ = assert_equal(vol, device)
    assert (nearest[1, 4:9, 5:11] == 2).all() and (nearest[3, 4:9, 5:11] == 1).all() and (nearest[2, 4:9, 5:11] == 1).all()
    assert (dist[2, 4:9, 5:11] == 4).all()
    assert_equal(vol, device, limit_sq=3)
    assert_equal(dots_map((5, 20, 24), 9, 12), device)
    assert_equal(dots_map((5, 20, 24), 9, 13), device, limit_sq=10)


def test_grids_above_the_launch_caps(device):
    shape = (1100, 1000)
    assert shape[0] * shape[1] > PASS_CAP_PIXELS               # the passes along y make a second trip
    lab = dots_map(shape, 300, 21, size=3)
    nearest, dist, _ = assert_equal(lab, device, ref=ref_nearest_tree)
    assert len(np.unique(nearest)) == len(np.unique(lab)) - 1 and dist.max() > 900
    tall = dots_map((ROW_CAP_ROWS + 13, 5), 40, 22)             # the row pass makes a second trip
    tall[ROW_CAP_ROWS - 1, 4], tall[ROW_CAP_ROWS, 0], tall[-1, 2] = 41, 42, 43
    assert_equal(tall, device, limit_sq=400, ref=ref_nearest_tree)


def tie_map():
    """70 x 130: a few boxes over a lattice of single pixels 6 rows and 4 columns apart whose ids differ from their
    neighbours': the pixels half way between two of them are ties"""
    lab = dots_map((70, 130), 25, 31, size=3)
    lattice = (np.arange(12)[:, None] * 33 + np.arange(33)[None, :]) % 9 + 1
    lab[::6, ::4] = np.where(lab[::6, ::4] == 0, lattice, lab[::6, ::4])
    return lab


def test_deterministic_and_transposed(device):
    lab = tie_map()
    nid = int(lab.max()) + 1
    for limit_sq in (-1, 8):
        first = run_nearest(lab, nid, limit_sq, device)
        second = run_nearest(lab, nid, limit_sq, device)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(first, second))
        turned = run_nearest(lab.T, nid, limit_sq, device)
        assert np.array_equal(turned[0].T, first[0]) and np.array_equal(turned[1].T, first[1])
        want = ref_nearest_tree(lab, nid, limit_sq)
        assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1])
    many, _, _ = ref_nearest_tree(lab, nid)
    other, _, _ = ref_nearest_tree(np.where(lab > 0, nid - lab, 0), nid)
    assert (many != np.where(other > 0, nid - other, 0)).sum() > 50           # the map has ties between different objects


def test_bad_labels_are_background(device):
    lab = dots_map((9, 70), 6, 41)
    clean = assert_equal(lab, device)
    assert clean[2] == 0
    for value, nid in ((-1, 7), (7, 7), (2 ** 24, 7), (-2 ** 31, 7), (6, 6)):
        dirty = lab.copy()
        dirty[4, 33], dirty[8, 69] = value, value
        nearest, dist, bad = assert_equal(dirty, device, nid=nid)
        assert bad == 1 and nearest.max() < nid and nearest[4, 33] != value and dist[4, 33] > 0


def test_rejected_arguments_launch_nothing(device):
    import ctypes

    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(64, dtype=torch.int32, device=device)
    outs = dict(nearest=Out((64,), np.int32, device), dist_sq=Out((64,), np.int32, device), bad=Out((1,), np.int32, device),
                workspace=Out((128,), np.int32, device))
    null = ctypes.c_void_p(0)

    def nearest(nd=2, Z=1, Y=8, X=8, nid=4, limit_sq=-1, nbytes=512, **ptrs):
        p = {k: o.ptr for k, o in outs.items()}
        p["labels"] = _clx.ptr(lab)
        p.update(ptrs)
        return lib.clx_label_nearest(p["labels"], nd, Z, Y, X, nid, limit_sq, p["nearest"], p["dist_sq"], p["bad"], p["workspace"], nbytes, st)

    refused = [dict(nd=1), dict(nd=4), dict(Z=2), dict(Y=0), dict(X=-8), dict(nd=3, Z=0), dict(nid=0), dict(nid=2 ** 24 + 1),
               dict(limit_sq=-2), dict(limit_sq=2 ** 30), dict(Y=65536, X=65536, nbytes=2 ** 40), dict(Y=2, X=32769, nbytes=2 ** 30),
               dict(nbytes=511), dict(nbytes=0), dict(workspace=ctypes.c_void_p(outs["workspace"].ptr.value + 2))]
    refused += [{k: null} for k in ("labels", "nearest", "dist_sq", "bad", "workspace")]
    for kw in refused:
        assert nearest(**kw) == -1, f"{kw} was accepted"
        assert lib.clx_last_error().decode().startswith("clx_label_nearest:"), kw
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert nearest() == 0 and nearest(nd=3, Z=2, Y=4) == 0       # the same buffers are accepted with valid arguments
    torch.cuda.synchronize(device)
    assert (outs["nearest"].get() == 0).all() and (outs["dist_sq"].get() == DIST_INF).all() and outs["bad"].get()[0] == 0
