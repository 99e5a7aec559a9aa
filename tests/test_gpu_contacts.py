"""clx_region_contacts / clx_region_perimeter through the C ABI against the restatements of tests/contacts_ref.py
(shifted comparisons + np.unique; mask minus erosion, convolution, histogram per object).  Everything is integer
work: the sorted (key, count) set and the class counts from row 1 up must be EQUAL.  Outputs are prefilled with 0xAB
bytes (or other garbage) and sit between guard words that must stay untouched."""

import ctypes
import os

import numpy as np
import pytest
import torch

from contacts_ref import ref_contacts, ref_perimeter
from test_gpu_measure import GUARD, Out, _blobs, _dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_LABEL, FULL = 1, 4                          # bits of info[0]


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))[f"{name}/labels"]


def call_contacts(labels, nd, nid, capacity, device, offset=0, fill=0xAB):
    """-> (keys, counts, info) as the entry point left them; the guard words are checked"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    Z, Y, X = (1,) * (3 - labels.ndim) + labels.shape
    lab = _dev(labels, device, offset)
    outs = dict(keys=Out((capacity,), np.uint64, device), counts=Out((capacity,), np.uint64, device), info=Out((2,), np.int32, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = _clx.load().clx_region_contacts(_clx.ptr(lab), nd, Z, Y, X, nid, capacity, outs["keys"].ptr, outs["counts"].ptr,
                                             outs["info"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return outs["keys"].get(), outs["counts"].get(), outs["info"].get()


def run_contacts(labels, nd, nid, device, capacity=1024, **kw):
    """-> (sorted keys, their counts, info[0]) of a call that placed every pair"""
    keys, counts, info = call_contacts(labels, nd, nid, capacity, device, **kw)
    assert not info[0] & FULL, "the table was reported full"
    used = keys != 0
    assert info[1] == used.sum() and (counts[~used] == 0).all() and (counts[used] > 0).all()
    order = np.argsort(keys[used])
    return keys[used][order], counts[used][order].astype(np.int64), int(info[0])


def assert_contacts_equal(labels, nd, nid, device, **kw):
    keys, counts, flags = run_contacts(labels, nd, nid, device, **kw)
    want_keys, want_counts = ref_contacts(labels, nd, nid)
    assert np.array_equal(keys, want_keys), (len(keys), len(want_keys))
    assert np.array_equal(counts, want_counts)
    lab = np.asarray(labels)
    assert flags == (BAD_LABEL if ((lab < 0) | (lab >= nid)).any() else 0)


def _noise(shape, ids, seed):
    """every pixel its own draw of `ids` ids: faces of every kind at every position"""
    return np.random.default_rng(seed).integers(0, ids, size=shape).astype(np.int32)


def _contact_cases():
    c = {}
    # row ends: a lane's 4 pixels straddle rows unless X is a multiple of 4
    for X in (1, 2, 3, 5):
        c[f"row_ends_9x{X}"] = (_noise((9, X), 4, X), 2, 4)
    c["row_ends_3x1027"] = (_noise((3, 1027), 3, 7), 2, 3)
    c["one_row_1x37"] = (_noise((1, 37), 4, 8), 2, 4)
    c["one_pixel"] = (np.ones((1, 1), np.int32), 2, 2)
    c["one_pixel_3d"] = (np.ones((1, 1, 1), np.int32), 3, 2)
    # 3-D
    c["3d_2x5x7"] = (_noise((2, 5, 7), 4, 9), 3, 4)
    c["3d_5x6x10"] = (_noise((5, 6, 10), 3, 10), 3, 3)
    slabs = np.zeros((5, 6, 8), np.int32)
    slabs[1, 1:4, 2:6] = 1
    slabs[2, 1:4, 2:6] = 2                              # 1 and 2 touch only across a slice
    slabs[4, 0:2, 0:3] = 3
    c["3d_touch_across_z"] = (slabs, 3, 4)
    flat = _blobs((12, 19), 6, 11)
    c["flat_as_3d"] = (flat[None], 3, 7)                # Z == 1 under nd == 3: two z faces to id 0 per object pixel
    c["flat_as_2d"] = (flat, 2, 7)
    # seams: an object edge exactly on a multiple of 1024 pixels, along x and along y
    seam = np.ones((8, 512), np.int32)
    seam[2:] = 2                                        # pixel 1024 starts row 2
    seam[4:, 256:] = 3                                  # pixel 2048 + 256
    c["edge_on_tile_seam_8x512"] = (seam, 2, 4)
    rows = np.repeat(np.arange(1, 6, dtype=np.int32), 1024).reshape(5, 1024)
    c["one_id_per_tile_5x1024"] = (rows, 2, 6)
    # more tiles than the grid has blocks (MAX_GRID = 1024 tiles of 1024 pixels): blocks take two tiles
    c["second_trip_1100x1000"] = (_blobs((1100, 1000), 400, 12), 2, 401)
    c["blobs_3d_6x40x70"] = (_blobs((6, 40, 70), 20, 13), 3, 21)
    # labels
    c["all_background"] = (np.zeros((7, 19), np.int32), 2, 5)
    c["one_object_fills_13x21"] = (np.full((13, 21), 3, np.int32), 2, 4)
    c["one_object_fills_3x5x8"] = (np.full((3, 5, 8), 1, np.int32), 3, 2)
    c["golden_2d"] = (_golden("2d"), 2, int(_golden("2d").max()) + 1)
    c["golden_2d_edge"] = (_golden("2d_edge"), 2, int(_golden("2d_edge").max()) + 1)
    c["golden_3d"] = (_golden("3d"), 3, int(_golden("3d").max()) + 1)
    return c


CONTACT_CASES = _contact_cases()
DISTINCT = np.arange(1, 64 * 64 + 1, dtype=np.int32).reshape(64, 64)       # 2 * 64 * 63 + 252 = 8316 pairs, 8320 faces


@pytest.mark.parametrize("name", sorted(CONTACT_CASES))
def test_contacts_equal_numpy(name, device):
    labels, nd, nid = CONTACT_CASES[name]
    assert_contacts_equal(labels, nd, nid, device)


def test_contacts_by_hand(device):
    keys, counts, _ = run_contacts(np.ones((1, 1), np.int32), 2, 2, device)
    assert keys.tolist() == [1] and counts.tolist() == [4]
    keys, counts, _ = run_contacts(np.ones((1, 1, 1), np.int32), 3, 2, device)
    assert keys.tolist() == [1] and counts.tolist() == [6]
    keys, counts, _ = run_contacts(np.zeros((7, 19), np.int32), 2, 5, device)
    assert len(keys) == 0
    keys, counts, _ = run_contacts(np.full((13, 21), 3, np.int32), 2, 4, device)
    assert keys.tolist() == [3] and counts.tolist() == [2 * (13 + 21)]
    flat = CONTACT_CASES["flat_as_2d"][0]
    k2, c2, _ = run_contacts(flat, 2, 7, device)
    k3, c3, _ = run_contacts(flat[None], 3, 7, device)
    assert np.array_equal(k2, k3)
    extra = c3 - c2                                     # the z faces: two per pixel of the object, all to id 0
    for key, n in zip(k2, extra):
        assert n == (2 * (flat == int(key)).sum() if key >> np.uint64(32) == 0 else 0)
    for name, pairs, between, faces in (("2d", 29, 15, 489), ("2d_edge", 3, 0, 322), ("3d", 13, 4, 489)):
        labels, nd, nid = CONTACT_CASES[f"golden_{name}"]
        keys, counts, _ = run_contacts(labels, nd, nid, device)
        assert (len(keys), int(((keys >> np.uint64(32)) > 0).sum()), int(counts.sum())) == (pairs, between, faces)


@pytest.mark.parametrize("name", ["row_ends_9x5", "row_ends_3x1027", "3d_5x6x10", "edge_on_tile_seam_8x512", "golden_2d"])
def test_contacts_unaligned_labels(name, device):
    """a label map that does not start on a 16-byte boundary takes the 4-byte loads"""
    labels, nd, nid = CONTACT_CASES[name]
    assert_contacts_equal(labels, nd, nid, device, offset=1)


def test_contacts_block_table_overflow(device):
    """8316 pairs from 4 blocks of 512 LDS slots each: most pairs go straight to the global table"""
    assert_contacts_equal(DISTINCT, 2, 64 * 64 + 1, device, capacity=16384)


def test_contacts_table_full_is_flagged_and_bounded(device):
    from cellulus_amd.measure import contact_pairs

    keys, counts, info = call_contacts(DISTINCT, 2, 64 * 64 + 1, 1024, device)      # checks the guard words
    assert info[0] & FULL and not info[0] & BAD_LABEL
    assert 0 <= info[1] <= 1024 and info[1] == (keys != 0).sum()
    a, b, faces = contact_pairs(DISTINCT, device)       # starts at 32768 slots: exact without a retry
    want_keys, want_counts = ref_contacts(DISTINCT, 2)
    assert np.array_equal((a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64), want_keys)
    assert np.array_equal(faces, want_counts)


def test_contact_pairs_retries_with_a_larger_table(device, monkeypatch):
    from cellulus_amd import measure

    capacities = []
    real = measure._clx.call

    def spy(name, *args):
        if name == "clx_region_contacts":
            capacities.append(args[6])
        return real(name, *args)

    monkeypatch.setattr(measure, "_pair_capacity", lambda objects: 1024)
    monkeypatch.setattr(measure._clx, "call", spy)
    a, b, faces = measure.contact_pairs(DISTINCT, device)
    assert capacities == [1024, 2048, 4096, 8192, 16384][:len(capacities)] and len(capacities) >= 4     # 8316 pairs
    want_keys, want_counts = ref_contacts(DISTINCT, 2)
    assert np.array_equal((a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64), want_keys)
    assert np.array_equal(faces, want_counts)
    assert a.dtype == b.dtype == faces.dtype == np.int64


def test_contacts_bad_labels(device):
    labels = _blobs((12, 70), 9, 5)
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[3, 7] = value
        lab[11, 69] = value
        lab[0, 0] = value
        keys, counts, flags = run_contacts(lab, 2, 10, device)
        assert flags == BAD_LABEL
        want_keys, want_counts = ref_contacts(lab, 2, 10)
        assert np.array_equal(keys, want_keys) and np.array_equal(counts, want_counts)
        vol = np.stack([lab, labels])
        assert_contacts_equal(vol, 3, 10, device)


def test_contacts_deterministic_and_stale_buffers(device):
    labels, nd, nid = CONTACT_CASES["second_trip_1100x1000"]
    first = run_contacts(labels, nd, nid, device, capacity=4096)
    again = run_contacts(labels, nd, nid, device, capacity=4096, fill=0x5C)
    zeros = run_contacts(labels, nd, nid, device, capacity=4096, fill=0)
    for other in (again, zeros):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]) and first[2] == other[2]
    noise = CONTACT_CASES["3d_5x6x10"]
    assert all(np.array_equal(x, y) for x, y in zip(run_contacts(*noise, device), run_contacts(*noise, device, fill=0xFF)))


# ------------------------------------------------------------------------------------------------- perimeter
def call_perimeter(labels, nid, device, offset=0, fill=0xAB):
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    Y, X = labels.shape
    lab = _dev(labels, device, offset)
    outs = dict(classes=Out((nid, 4), np.uint64, device), bad=Out((1,), np.int32, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = _clx.load().clx_region_perimeter(_clx.ptr(lab), Y, X, nid, outs["classes"].ptr, outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return outs["classes"].get().astype(np.int64), int(outs["bad"].get()[0])


def assert_perimeter_equal(labels, nid, device, **kw):
    classes, bad = call_perimeter(labels, nid, device, **kw)
    want, _ = ref_perimeter(labels, nid)
    assert np.array_equal(classes[1:], want[1:])
    lab = np.asarray(labels)
    assert bad == int(((lab < 0) | (lab >= nid)).any())
    return classes


def _ellipses(shape, centres, radii):
    yy, xx = np.indices(shape)
    lab = np.zeros(shape, np.int32)
    for i, ((cy, cx), (ry, rx)) in enumerate(zip(centres, radii), 1):
        lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = i
    return lab


def _perimeter_cases():
    c = {}
    c["noise_45x70"] = (_noise((45, 70), 4, 21), 4)                      # every code at every position of a tile
    c["noise_coarse_67x99"] = (np.kron(_noise((23, 33), 5, 22), np.ones((3, 3), np.int32))[:67, :99], 5)
    c["one_pixel_image"] = (np.ones((1, 1), np.int32), 2)
    c["thin_1x40"] = (_noise((1, 40), 3, 23), 3)
    c["thin_40x1"] = (_noise((40, 1), 3, 24), 3)
    # objects whose border crosses the corners of the 32 x 32 tiles
    c["tile_corners_100x100"] = (_ellipses((100, 100), [(32, 32), (64, 64), (32, 64), (63, 31), (96, 96)],
                                           [(9, 12), (14, 8), (5, 5), (7, 7), (6, 9)]), 6)
    diag = np.zeros((70, 70), np.int32)
    diag[np.arange(3, 67), np.arange(3, 67)] = 1                        # crosses (32, 32) and (64, 64): the sqrt 2 class
    diag[np.arange(5, 40), 69 - np.arange(5, 40)] = 2
    c["diagonal_lines_70x70"] = (diag, 3)
    hole = np.zeros((40, 50), np.int32)
    hole[5:30, 6:41] = 1
    hole[12:20, 15:30] = 0
    hole[14:17, 18:25] = 2                                              # an object inside the hole
    c["rectangle_with_hole"] = (hole, 3)
    side = np.zeros((20, 40), np.int32)
    side[4:15, 5:18] = 1
    side[4:15, 18:33] = 2                                               # the shared edge is border for both
    c["side_by_side"] = (side, 3)
    edge = np.zeros((35, 66), np.int32)
    edge[0:9, 0:12] = 1
    edge[20:35, 50:66] = 2
    edge[0:4, 30:40] = 3
    c["on_the_image_edge"] = (edge, 4)
    c["one_object_fills_33x65"] = (np.full((33, 65), 1, np.int32), 2)
    c["all_background"] = (np.zeros((9, 40), np.int32), 3)
    c["golden_2d"] = (_golden("2d"), int(_golden("2d").max()) + 1)
    c["golden_2d_edge"] = (_golden("2d_edge"), int(_golden("2d_edge").max()) + 1)
    # 33 x 33 = 1089 tiles of 32 x 32 against a grid of 1024 blocks: blocks take two tiles
    c["second_trip_1040x1050"] = (_blobs((1040, 1050), 400, 25), 401)
    # 300 ids in one tile against the 256 slots of the block's table: the overflow route
    c["distinct_30x30"] = (np.arange(1, 901, dtype=np.int32).reshape(30, 30), 901)
    return c


PERIMETER_CASES = _perimeter_cases()


@pytest.mark.parametrize("name", sorted(PERIMETER_CASES))
def test_perimeter_equal_numpy(name, device):
    labels, nid = PERIMETER_CASES[name]
    assert_perimeter_equal(labels, nid, device)


def test_perimeter_by_hand(device):
    from cellulus_amd.measure import perimeter_from_classes

    for h, w, y, x in ((2, 2, 3, 3), (3, 9, 30, 28), (12, 5, 60, 1), (40, 37, 10, 20), (2, 70, 31, 2)):
        lab = np.zeros((96, 80), np.int32)
        lab[y:y + h, x:x + w] = 1
        classes, _ = call_perimeter(lab, 2, device)
        assert classes[1].tolist() == [2 * (h + w) - 4, 2 * (h + w) - 4, 0, 0], (h, w)
        assert perimeter_from_classes(classes[1:])[0] == 2 * (h + w) - 4
    classes, _ = call_perimeter(np.ones((1, 1), np.int32), 2, device)
    assert classes[1].tolist() == [1, 0, 0, 0]                          # code 1: no weight
    diag, _ = PERIMETER_CASES["diagonal_lines_70x70"]
    classes, _ = call_perimeter(diag, 3, device)
    assert classes[1].tolist() == [64, 0, 62, 0] and classes[2].tolist() == [35, 0, 33, 0]       # the ends have code 11
    side, _ = PERIMETER_CASES["side_by_side"]
    classes, _ = call_perimeter(side, 3, device)
    assert classes[1, 0] == 2 * (11 + 13) - 4 and classes[2, 0] == 2 * (11 + 15) - 4
    labels, nid = PERIMETER_CASES["golden_2d_edge"]
    perimeter = perimeter_from_classes(call_perimeter(labels, nid, device)[0])
    assert perimeter[2] == pytest.approx(34.41421356237309, rel=1e-14) and perimeter[3] == 136.0 and perimeter[7] == 0.0


def test_perimeter_unaligned_bad_labels_determinism_stale(device):
    labels, nid = PERIMETER_CASES["noise_coarse_67x99"]
    first = assert_perimeter_equal(labels, nid, device)
    assert np.array_equal(first[1:], assert_perimeter_equal(labels, nid, device, offset=1)[1:])
    assert np.array_equal(first[1:], assert_perimeter_equal(labels, nid, device, fill=0x5C)[1:])
    assert np.array_equal(first[1:], assert_perimeter_equal(labels, nid, device, fill=0)[1:])
    for value in (-1, -2 ** 31, 5, 2 ** 31 - 1):
        lab = labels.copy()
        lab[0, 0] = lab[31, 32] = lab[66, 98] = lab[40, 7] = value
        classes, bad = call_perimeter(lab, nid, device)
        assert bad == 1
        assert np.array_equal(classes[1:], ref_perimeter(lab, nid)[0][1:])


# ------------------------------------------------------------------------------------------- rejected arguments
def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(64, dtype=torch.int32, device=device)
    outs = {k: Out((1024,), np.uint64, device) for k in ("keys", "counts", "info", "classes", "bad")}
    null = ctypes.c_void_p(0)

    def contacts(nd=2, Z=1, Y=8, X=8, nid=4, capacity=1024, **ptrs):
        p = dict(labels=_clx.ptr(lab), keys=outs["keys"].ptr, counts=outs["counts"].ptr, info=outs["info"].ptr)
        p.update(ptrs)
        return lib.clx_region_contacts(p["labels"], nd, Z, Y, X, nid, capacity, p["keys"], p["counts"], p["info"], st)

    def perimeter(Y=8, X=8, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(lab), classes=outs["classes"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_perimeter(p["labels"], Y, X, nid, p["classes"], p["bad"], st)

    refused = [lambda k=k: contacts(**{k: null}) for k in ("labels", "keys", "counts", "info")] + [
        lambda: contacts(nd=1), lambda: contacts(nd=4), lambda: contacts(nd=0),
        lambda: contacts(nd=2, Z=2, Y=4, X=8),                  # 2-D needs Z == 1
        lambda: contacts(Z=0), lambda: contacts(Y=0), lambda: contacts(X=-1), lambda: contacts(nd=3, Z=-2),
        lambda: contacts(Y=65536, X=65536),                     # npix = 2^32
        lambda: contacts(nd=3, Z=2, Y=46341, X=46341),          # just above 2^32
        lambda: contacts(nid=0), lambda: contacts(nid=-3), lambda: contacts(nid=2 ** 24 + 1),
        lambda: contacts(capacity=0), lambda: contacts(capacity=512), lambda: contacts(capacity=1025),
        lambda: contacts(capacity=3072), lambda: contacts(capacity=2 ** 29), lambda: contacts(capacity=-1024),
    ] + [lambda k=k: perimeter(**{k: null}) for k in ("labels", "classes", "bad")] + [
        lambda: perimeter(Y=0), lambda: perimeter(X=-1), lambda: perimeter(Y=65536, X=65536),
        lambda: perimeter(nid=0), lambda: perimeter(nid=2 ** 24 + 1),
    ]
    for i, call in enumerate(refused):
        status = call()
        assert status < 0, f"case {i} was accepted"
        assert len(lib.clx_last_error()) > 0, f"case {i} left no message"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert contacts() == 0 and contacts(nd=3, Z=2, Y=4, X=8) == 0 and perimeter() == 0      # accepted with valid arguments
    torch.cuda.synchronize(device)
