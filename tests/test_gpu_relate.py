"""clx_label_overlaps / clx_region_clearance through the C ABI against the restatements of tests/relate_ref.py (np.unique over
the stacked pairs; one mask per object).  Everything is integer work: the sorted (key, count) set and every word of the
clearance rows must be EQUAL.  Outputs are prefilled with 0xAB bytes (or other garbage) and sit between guard words that must
stay untouched; inputs are followed by a tail of valid values that would change the result if it were read."""

import numpy as np
import pytest
import torch

from inscribed_ref import ref_distance_sq
from relate_ref import ALL_ONES, DIST_INF, blob_map, clearance_words, ref_clearance, ref_overlaps
from test_cpu_relate import CHILDREN, PARENTS
from test_gpu_measure import GUARD, Out

pytestmark = pytest.mark.gpu

BAD_A, BAD_B, FULL = 1, 2, 4                    # bits of info[0]
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)          # a lane, a wave, a tile and one pixel either side
OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 1))      # the scalar path of one map meets the vector path of the other
TAIL = 8


def dev_in(values, device, offset=0, tail=1):
    """int32 -> flat device tensor that starts `offset` elements into a 16-byte-aligned allocation and is followed by TAIL
    elements of `tail`, a valid value: a read past the end changes the result"""
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).reshape(-1)
    big = torch.full((offset + t.numel() + TAIL,), tail, dtype=torch.int32, device=device)
    big[offset:offset + t.numel()] = t.to(device)
    return big[offset:offset + t.numel()]


def call_overlaps(a, b, nid_a, nid_b, capacity, device, offsets=(0, 0), fill=0xAB):
    """-> (keys, counts, info) as the entry point left them; the guard words are checked"""
    from cellulus_amd import _clx

    da, db = dev_in(a, device, offsets[0]), dev_in(b, device, offsets[1])
    outs = dict(keys=Out((capacity,), np.uint64, device), counts=Out((capacity,), np.uint64, device), info=Out((2,), np.int32, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = _clx.load().clx_label_overlaps(_clx.ptr(da), _clx.ptr(db), da.numel(), nid_a, nid_b, capacity, outs["keys"].ptr,
                                            outs["counts"].ptr, outs["info"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return outs["keys"].get(), outs["counts"].get(), outs["info"].get()


def run_overlaps(a, b, nid_a, nid_b, device, capacity=1024, **kw):
    """-> (sorted keys, their counts, info[0]) of a call that placed every pair"""
    keys, counts, info = call_overlaps(a, b, nid_a, nid_b, capacity, device, **kw)
    assert not info[0] & FULL, "the table was reported full"
    used = keys != 0
    assert info[1] == used.sum() and (counts[~used] == 0).all() and (counts[used] > 0).all()
    order = np.argsort(keys[used])
    return keys[used][order], counts[used][order].astype(np.int64), int(info[0])


def assert_overlaps_equal(a, b, nid_a, nid_b, device, **kw):
    keys, counts, flags = run_overlaps(a, b, nid_a, nid_b, device, **kw)
    want_keys, want_counts, want_flags = ref_overlaps(a, b, nid_a, nid_b)
    assert np.array_equal(keys, want_keys), (len(keys), len(want_keys))
    assert np.array_equal(counts, want_counts)
    assert flags == want_flags
    return keys, counts


def runs(n, ids, seed, longest=40):
    """n values below `ids` in runs of random length: uniform lanes, run ends inside lanes, background stretches"""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, ids, size=n + 1)
    lengths = rng.integers(1, longest, size=n + 1)
    return np.repeat(values, lengths)[:n].astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_overlaps_sizes_and_alignment(n, device):
    a, b = runs(n, 5, n), runs(n, 4, n + 1)
    a[-1], b[0] = 4, 3                                          # the last and the first pixel always count
    for offsets in OFFSETS:
        assert_overlaps_equal(a, b, 5, 4, device, offsets=offsets)
    noise = np.random.default_rng(n).integers(0, 3, size=(2, n)).astype(np.int32)       # no runs at all
    for offsets in OFFSETS:
        assert_overlaps_equal(noise[0], noise[1], 3, 3, device, offsets=offsets)


def test_overlaps_by_hand(device):
    keys, counts, info = call_overlaps(np.zeros(700, np.int32), np.zeros(700, np.int32), 5, 5, 1024, device)
    assert not keys.any() and not counts.any() and info.tolist() == [0, 0]          # an empty table
    keys, counts, _ = run_overlaps(CHILDREN, PARENTS, 6, 7, device)
    a, b = (keys >> np.uint64(32)).tolist(), (keys & np.uint64(0xFFFFFFFF)).tolist()
    assert list(zip(a, b, counts.tolist())) == [(0, 1, 3), (0, 3, 1), (0, 6, 2), (1, 1, 4), (2, 0, 4), (3, 1, 1), (3, 2, 4), (3, 3, 1),
                                                (4, 3, 4), (5, 4, 2), (5, 5, 2)]
    # ids at the top of the range, one pixel each
    a, b = np.zeros(9, np.int32), np.zeros(9, np.int32)
    a[2], b[2], b[7] = 2 ** 24 - 1, 2 ** 24 - 1, 1
    keys, counts, _ = run_overlaps(a, b, 2 ** 24, 2 ** 24, device)
    assert keys.tolist() == [1, ((2 ** 24 - 1) << 32) | (2 ** 24 - 1)] and counts.tolist() == [1, 1]


def test_overlaps_pairs_change_inside_a_lane_and_whole_wave_runs(device):
    n = 1024 + 512
    one = np.ones(n, np.int32)
    for period in (1, 2, 3):                                    # a stays constant, b changes inside every lane
        b = (np.arange(n) // period % 3).astype(np.int32)
        assert_overlaps_equal(one, b, 2, 3, device)
        assert_overlaps_equal(b, one, 3, 2, device)
    for length in (256, 252, 248, 260, 512, 4):                 # runs that span a wave, end one lane short of it, cross into the next
        a = (np.arange(n) // length % 2 + 1).astype(np.int32)
        b = (np.arange(n) // length % 3).astype(np.int32)
        keys, counts = assert_overlaps_equal(a, b, 3, 3, device)
        assert counts.sum() == n
        assert_overlaps_equal(a, b, 3, 3, device, offsets=(1, 1))
    # a run of background pairs between two runs of one pair: the skipped lanes do not join them
    a = np.ones(n, np.int32)
    a[256:512] = 0
    a[1000:1030] = 0
    keys, counts = assert_overlaps_equal(a, np.zeros(n, np.int32), 2, 1, device)
    assert keys.tolist() == [1 << 32] and counts.tolist() == [n - 286]


def test_overlaps_block_table_overflow_full_table_and_determinism(device):
    """48 x 48 ids in a: 2304 pairs from 3 blocks of 512 LDS slots each, so most go straight to the global table"""
    a = np.arange(1, 48 * 48 + 1, dtype=np.int32).reshape(48, 48)
    b = blob_map((48, 48), 9, 5)
    nid_a = 48 * 48 + 1
    keys, counts, info = call_overlaps(a, b, nid_a, 10, 1024, device)                # checks the guard words
    assert info[0] == FULL and 0 <= info[1] <= 1024 and info[1] == (keys != 0).sum()
    first = assert_overlaps_equal(a, b, nid_a, 10, device, capacity=4096)
    assert len(first[0]) == 48 * 48
    again = run_overlaps(a, b, nid_a, 10, device, capacity=4096, fill=0x5C)
    zeros = run_overlaps(a, b, nid_a, 10, device, capacity=4096, fill=0)
    for other in (again, zeros):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])
    assert_overlaps_equal(b, a, 10, nid_a, device, capacity=8192)


def test_overlaps_bad_labels(device):
    a, b = blob_map((12, 70), 9, 5), blob_map((12, 70), 6, 6)
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        for in_a, in_b, want in ((True, False, BAD_A), (False, True, BAD_B), (True, True, BAD_A | BAD_B)):
            x, y = a.copy(), b.copy()
            for m, hit in ((x, in_a), (y, in_b)):
                if hit:
                    m[3, 7] = m[11, 69] = m[0, 0] = value
            keys, counts, flags = run_overlaps(x, y, 10, 7, device)
            assert flags == want
            want_keys, want_counts, _ = ref_overlaps(x, y, 10, 7)
            assert np.array_equal(keys, want_keys) and np.array_equal(counts, want_counts)     # those pixels count as 0


def test_overlaps_more_tiles_than_blocks(device):
    n = 1025 * 1024 + 3                                         # the grid is capped at 1024 blocks: blocks take two tiles
    a, b = runs(n, 300, 1, 2000), runs(n, 200, 2, 3000)
    a[-3:], b[-3:] = 299, 0
    keys, counts = assert_overlaps_equal(a, b, 300, 200, device, capacity=1 << 17)
    assert counts.sum() == ((a > 0) | (b > 0)).sum()
    again = run_overlaps(a, b, 300, 200, device, capacity=1 << 17, fill=0)
    assert np.array_equal(keys, again[0]) and np.array_equal(counts, again[1])


# ------------------------------------------------------------------------------------------------- clearance
def call_clearance(a, b, dist, parent, nid_a, device, offsets=(0, 0, 0), fill=0xAB):
    """-> (out uint64 (nid_a, 3), bad) as the entry point left them; the guard words are checked"""
    from cellulus_amd import _clx

    da, db = dev_in(a, device, offsets[0]), dev_in(b, device, offsets[1], tail=int(np.max(parent)))
    dd = dev_in(dist, device, offsets[2], tail=0)
    dp = dev_in(parent, device)
    assert len(dp) == nid_a
    outs = dict(out=Out((nid_a, 3), np.uint64, device), bad=Out((1,), np.int32, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = _clx.load().clx_region_clearance(_clx.ptr(da), _clx.ptr(db), _clx.ptr(dd), _clx.ptr(dp), da.numel(), nid_a, outs["out"].ptr,
                                              outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return outs["out"].get(), int(outs["bad"].get()[0])


def assert_clearance_equal(a, b, dist, parent, nid_a, device, **kw):
    out, bad = call_clearance(a, b, dist, parent, nid_a, device, **kw)
    rows, want_bad = ref_clearance(a, b, dist, parent, nid_a)
    assert np.array_equal(out, clearance_words(rows)), np.flatnonzero((out != clearance_words(rows)).any(axis=1))[:8]
    assert bad == want_bad
    return out


def test_clearance_by_hand(device):
    dist = ref_distance_sq(PARENTS, False)
    # 1 inside its parent, 2 has none, 3 lies across three and belongs to 2, 4 inside 3, 5 is given 6, which it never meets
    out = assert_clearance_equal(CHILDREN, PARENTS, dist, [0, 1, 0, 2, 3, 6], 6, device)
    assert out[1].tolist() == [4, (2 << 32) | 7, 18]            # the nearest pixel of 1 is (1, 1), sqrt 2 from (2, 2)
    assert out[2].tolist() == [0, ALL_ONES, 0] and out[5].tolist() == [0, ALL_ONES, 0] and out[0].tolist() == [0, ALL_ONES, 0]
    assert out[3].tolist() == [4, (1 << 32) | 14, 4]            # four pixels tie at distance 1: the first in raster order, (2, 2)
    assert out[4].tolist() == [4, (1 << 32) | 25, 10]           # (4, 1) and (5, 1) tie: (4, 1)
    # the same child counted inside another of the parents it meets
    out = assert_clearance_equal(CHILDREN, PARENTS, dist, [0, 0, 0, 1, 0, 5], 6, device)
    assert out[3].tolist() == [1, (1 << 32) | 13, 1] and out[5].tolist() == [2, (1 << 32) | 29, 2]
    # negative parents and parents that no pixel carries are only compared
    assert_clearance_equal(CHILDREN, PARENTS, dist, [7, -1, -5, 2 ** 31 - 1, 3, 1000], 6, device)


def test_clearance_bad_distances_and_labels(device):
    dist = ref_distance_sq(PARENTS, False).astype(np.int32)
    parent = [0, 1, 0, 2, 3, 4]
    for value in (-1, DIST_INF + 1, -2 ** 31, 2 ** 31 - 1):
        d = dist.copy()
        d[0, 0] = d[3, 3] = value                               # under counted pixels of 1 and 3: skipped
        out, bad = call_clearance(CHILDREN, PARENTS, d, parent, 6, device)
        rows, want_bad = ref_clearance(CHILDREN, PARENTS, d, parent, 6)
        assert bad == want_bad == 2 and np.array_equal(out, clearance_words(rows))
        assert out[1, 0] == 3 and out[3, 0] == 3
        d = dist.copy()
        d[0, 4] = d[2, 1] = d[2, 0] = value                     # under 2 (no parent), under 3 outside its parent, under no child
        assert call_clearance(CHILDREN, PARENTS, d, parent, 6, device)[1] == 0
    d = dist.copy()
    d[1, 1] = DIST_INF                                          # the largest value that counts
    out = assert_clearance_equal(CHILDREN, PARENTS, d, parent, 6, device)
    assert out[1, 2] == 16 + DIST_INF
    for value in (-1, 6, 2 ** 31 - 1):
        a = CHILDREN.copy()
        a[0, 0] = a[5, 5] = value
        out, bad = call_clearance(a, PARENTS, dist, parent, 6, device)
        rows, want_bad = ref_clearance(a, PARENTS, dist, parent, 6)
        assert bad == want_bad == 1 and np.array_equal(out, clearance_words(rows))


@pytest.mark.parametrize("n", SIZES)
def test_clearance_sizes_and_alignment(n, device):
    rng = np.random.default_rng(n)
    a, b = runs(n, 6, n + 2), runs(n, 4, n + 3)
    a[-1], b[-1], a[0], b[0] = 5, 3, 1, 2
    dist = rng.integers(0, 40, size=n).astype(np.int32)
    parent = np.array([0, 2, 1, 0, 3, 3], np.int32)
    for offsets in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 2, 3)):
        assert_clearance_equal(a, b, dist, parent, 6, device, offsets=offsets)
    flat = np.full(n, 7, np.int32)                              # every pixel ties: index 0 wins, in every run of the wave
    out = assert_clearance_equal(np.ones(n, np.int32), np.ones(n, np.int32), flat, [0, 1], 2, device)
    assert out[1].tolist() == [n, 7 << 32, 7 * n]


def test_clearance_block_table_overflow_more_tiles_than_blocks_determinism(device):
    # 1600 ids in two blocks against 256 slots: the straight-to-global route
    a = np.arange(1, 1601, dtype=np.int32).reshape(40, 40)
    b = blob_map((40, 40), 5, 8)
    dist = ref_distance_sq(b, True).astype(np.int32)
    parent = np.r_[0, b.reshape(-1)].astype(np.int32)           # every pixel's own parent; 0 over background
    parent[5::7] = 3
    assert_clearance_equal(a, b, dist, parent, 1601, device)
    n = 1025 * 1024 + 3
    a, b = runs(n, 300, 3, 2000), runs(n, 200, 4, 3000)
    a[-3:], b[-3:] = 299, 7
    rng = np.random.default_rng(5)
    dist = rng.integers(0, 2 ** 20, size=n).astype(np.int32)
    parent = rng.integers(0, 200, size=300).astype(np.int32)
    parent[299] = 7
    first = assert_clearance_equal(a, b, dist, parent, 300, device)
    assert first[299, 0] >= 3
    again, _ = call_clearance(a, b, dist, parent, 300, device, fill=0)
    assert np.array_equal(first, again)


def test_rejected_arguments_launch_nothing(device):
    import ctypes

    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(64, dtype=torch.int32, device=device)
    outs = {k: Out((1024,), np.uint64, device) for k in ("keys", "counts", "info", "out", "bad")}
    null = ctypes.c_void_p(0)

    def overlaps(npix=64, nid_a=4, nid_b=4, capacity=1024, **ptrs):
        p = dict(a=_clx.ptr(lab), b=_clx.ptr(lab), keys=outs["keys"].ptr, counts=outs["counts"].ptr, info=outs["info"].ptr)
        p.update(ptrs)
        return lib.clx_label_overlaps(p["a"], p["b"], npix, nid_a, nid_b, capacity, p["keys"], p["counts"], p["info"], st)

    def clearance(npix=64, nid_a=4, **ptrs):
        p = dict(a=_clx.ptr(lab), b=_clx.ptr(lab), dist_sq=_clx.ptr(lab), parent=_clx.ptr(lab), out=outs["out"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_clearance(p["a"], p["b"], p["dist_sq"], p["parent"], npix, nid_a, p["out"], p["bad"], st)

    refused = [lambda k=k: overlaps(**{k: null}) for k in ("a", "b", "keys", "counts", "info")] + [
        lambda: overlaps(npix=0), lambda: overlaps(npix=2 ** 32), lambda: overlaps(nid_a=0), lambda: overlaps(nid_b=2 ** 24 + 1),
        lambda: overlaps(capacity=512), lambda: overlaps(capacity=1025), lambda: overlaps(capacity=2 ** 29),
    ] + [lambda k=k: clearance(**{k: null}) for k in ("a", "b", "dist_sq", "parent", "out", "bad")] + [
        lambda: clearance(npix=0), lambda: clearance(npix=2 ** 32), lambda: clearance(nid_a=0), lambda: clearance(nid_a=2 ** 24 + 1),
    ]
    for i, call in enumerate(refused):
        assert call() == -1, f"case {i} was accepted"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert overlaps() == 0 and clearance() == 0                 # accepted with valid arguments
    torch.cuda.synchronize(device)
