"""clx_region_weighted and clx_region_border_intensity through the C ABI against the restatement of tests/weighted_ref.py
(Python-int sums per id).  Everything is integer work: every word of every id from 1 up and bad must be EQUAL.  The outputs are
prefilled with 0xAB bytes (or other garbage) and sit between guard words that must stay untouched."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

from test_gpu_measure import F32, F64, GUARD, I32, Out, _blobs, _dev, _raw, run_intensity
from weighted_ref import (BAD_LABEL, BAD_VALUE, NB, NO_PEAK, NW, border_words, ref_border, ref_border_mask, ref_keys, ref_max_keys,
                          ref_weighted, weighted_words)

pytestmark = pytest.mark.gpu

RAW_TYPE = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}


def _zyx(labels):
    return (1,) * (3 - labels.ndim) + labels.shape


def call_weighted(labels, raw, nid, shift, peak_keys, device, offsets=(0, 0), fill=0xAB):
    """one clx_region_weighted call -> (words uint64 (nid, 21), bad); guard words checked.  offsets: elements by which the label
    and raw pointers are moved off their 16-byte-aligned allocations"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    raw = np.ascontiguousarray(raw)
    assert raw.size == labels.size
    lab, raw_d = _dev(labels, device, offsets[0]), _dev(raw, device, offsets[1])
    keys = None if peak_keys is None else _dev(np.asarray(peak_keys, dtype=np.uint64).view(np.int64), device)
    out, bad = Out((nid, NW), np.uint64, device), Out((1,), np.int32, device)
    for o in (out, bad):
        o.buf[GUARD:GUARD + o.nbytes] = fill
    lib = _clx.load()
    status = lib.clx_region_weighted(_clx.ptr(lab), _clx.ptr(raw_d), RAW_TYPE[raw.dtype], *_zyx(labels), nid, shift, _clx.ptr(keys),
                                     out.ptr, bad.ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return out.get(), int(bad.get()[0])


def call_border(labels, raw, nid, nd, shift, device, offsets=(0, 0), fill=0xAB):
    """one clx_region_border_intensity call -> (words uint64 (nid, 7), bad); guard words checked"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    raw = np.ascontiguousarray(raw)
    assert raw.size == labels.size
    lab, raw_d = _dev(labels, device, offsets[0]), _dev(raw, device, offsets[1])
    out, bad = Out((nid, NB), np.uint64, device), Out((1,), np.int32, device)
    for o in (out, bad):
        o.buf[GUARD:GUARD + o.nbytes] = fill
    lib = _clx.load()
    status = lib.clx_region_border_intensity(_clx.ptr(lab), _clx.ptr(raw_d), RAW_TYPE[raw.dtype], nd, *_zyx(labels), nid, shift,
                                             out.ptr, bad.ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return out.get(), int(bad.get()[0])


def _differ(words, want):
    differ = np.argwhere(words[1:] != want[1:])
    return len(differ), [(p.tolist(), hex(int(words[1:][tuple(p)])), hex(int(want[1:][tuple(p)]))) for p in differ[:4]]


def check_weighted(labels, raw, nid, device, shift=0, peak="max", want_bad=0, small=False, **kw):
    """-> (words from id 1 up, the restatement's rows from id 1 up) after comparing every word and bad.  peak "max": the
    largest keys of the counted pixels, as clx_region_intensity leaves them"""
    keys = ref_max_keys(labels, raw, nid, shift) if isinstance(peak, str) else peak
    words, bad = call_weighted(labels, raw, nid, shift, keys, device, **kw)
    rows, ref_bad = ref_weighted(labels, raw, nid, shift, keys, small=small)
    n, first = _differ(words, weighted_words(rows))
    assert n == 0, (n, first)
    assert bad == ref_bad == want_bad
    return words[1:], rows[1:]


def check_border(labels, raw, nid, device, nd=None, shift=0, want_bad=0, small=False, **kw):
    nd = np.asarray(labels).ndim if nd is None else nd
    words, bad = call_border(labels, raw, nid, nd, shift, device, **kw)
    rows, ref_bad = ref_border(labels, raw, nid, nd, shift, small=small)
    n, first = _differ(words, border_words(rows))
    assert n == 0, (n, first)
    assert bad == ref_bad == want_bad
    return words[1:], rows[1:]


def _values(shape, seed, dtype=np.float32):
    """values that quantise exactly at shift 4: multiples of 1/16 in (-2048, 2048)"""
    return (np.random.default_rng(seed).integers(-2 ** 15, 2 ** 15, size=shape) / 16.0).astype(dtype)


SHAPES = [(1, 1), (5, 1), (4, 2), (2, 3, 3), (3, 5), (7, 129), (33, 31), (5, 4, 37), (9, 130)]


@pytest.mark.parametrize("offsets", list(itertools.product((0, 1, 3), repeat=2)), ids=lambda o: "".join(map(str, o)))
def test_row_ends_and_tails(offsets, device):
    """row ends inside a lane, X < 4, the scalar tail past the last whole lane, and the 16-byte or 4-byte loads decided for
    each pointer (and for the rows and slices of the stencil) alone; every raw type"""
    for shape in SHAPES:
        labels = _blobs(shape, 5, 3 + len(shape))
        if labels.max() == 0:
            labels[:] = 1
        nid = int(labels.max()) + 2                          # the last id is absent
        for raw, shift in ((_values(shape, 2), 4), (_values(shape, 3, np.float64), 2), (_raw("i32", shape, 4), 0)):
            check_weighted(labels, raw, nid, device, shift, offsets=offsets)
            check_border(labels, raw, nid, device, shift=shift, offsets=offsets)
            if labels.ndim == 3:
                check_border(labels.reshape(1, -1, shape[2]), raw, nid, device, nd=3, shift=shift, offsets=offsets)


def test_128_bit_sums(device):
    """a 1 x 70001 row of one object: x^2 exceeds 2^32, float64 values at +-bound in alternating blocks make the partial sums
    run up and down through the low limb's wrap, in LDS (one id) and in the global fall-back (the id among PROBES + 1
    colliding ones in every tile)"""
    X = 70001
    bound = float(2 ** 62 >> int(X).bit_length())
    x = np.arange(X)
    raw = np.where((x // 1500) % 2 == 0, bound, -bound).reshape(1, X)
    raw[0, ::7] += np.where(raw[0, ::7] > 0, -3.0, 5.0)     # not all equal, still within the bound
    labels = np.ones((1, X), np.int32)
    words, rows = check_weighted(labels, raw, 2, device)
    assert all(int(words[0][4 + 2 * p]) not in (0, 2 ** 64 - 1) for p in (2, 5)), "Σq·x and Σq·x² must need the high limb"
    assert abs(rows[0][8]) > 2 ** 64 and rows[0][3] == 0 and rows[0][6] == 0
    # twenty ids that collide in one slot chain share the row in runs of two lanes: PROBES = 8 of them fit a block's table, the
    # others send every piece to global memory, limb by limb
    ids = 2 + 256 * np.arange(20, dtype=np.int32)
    labels = ids[(x // 8) % 20].reshape(1, X)
    words, rows = check_weighted(labels, raw, int(ids[-1]) + 1, device)
    assert all(abs(rows[i - 1][8]) > 2 ** 64 and int(words[i - 1][14]) not in (0, 2 ** 64 - 1) for i in ids)
    assert any(rows[i - 1][8] < 0 for i in ids) and any(rows[i - 1][8] > 0 for i in ids)
    # two image rows with y = 1: Σq·yx and Σq·y are formed at the run's head from S1 and S0
    labels = np.ones((2, 35001), np.int32)
    raw2 = np.where((np.arange(70002) // 900) % 2 == 0, bound, -bound + 1).reshape(2, 35001)
    check_weighted(labels, raw2, 2, device)
    check_border(labels, raw2, 2, device)                    # Σq² near 2^(2 * 45) * 7e4
    # shift 1 moves the same values over the bound: every pixel is refused
    words, bad = call_weighted(labels, raw2, 2, 1, None, device)
    assert bad == BAD_VALUE and not words[1, :2].any() and not words[1, 3:].any() and words[1, 2] == NO_PEAK


def test_shift_at_both_clamps(device):
    labels = _blobs((9, 40), 6, 8)
    rng = np.random.default_rng(6)
    tiny = rng.integers(-2 ** 20, 2 ** 20, size=labels.shape) * 2.0 ** -1040
    huge = rng.integers(-2 ** 20, 2 ** 20, size=labels.shape) * 2.0 ** 1003
    for raw, shift in ((tiny, 1023), (huge, -1022)):
        _, rows = check_weighted(labels, raw, 8, device, shift)
        assert any(r[5] for r in rows)
        check_border(labels, raw, 8, device, shift=shift)


def test_lds_table(device):
    """far more ids than the 256 slots of a block's table, more ids congruent modulo the slot count in one tile than find_slot
    probes, and one object over a whole map, every lane of every wave in the same slot"""
    rng = np.random.default_rng(3)
    many = rng.integers(1, 2001, size=(40, 100)).astype(np.int32)
    raw = _values(many.shape, 9)
    check_weighted(many, raw, 2001, device, 4)
    check_border(many, raw, 2001, device, shift=4)
    ids = 1 + 256 * np.arange(20, dtype=np.int32)            # 20 ids in slot 1's chain: PROBES = 8 of them fit
    collide = np.repeat(ids, 48).reshape(-1)
    rng.shuffle(collide[400:])                               # runs, then single pixels
    collide = collide.reshape(8, 120)
    raw = _values(collide.shape, 1, np.float64)
    _, rows = check_weighted(collide, raw, int(ids[-1]) + 1, device, 4)
    assert all(rows[i - 1][0] > 0 for i in ids)
    _, rows = check_border(collide, raw, int(ids[-1]) + 1, device, shift=4)
    assert all(rows[i - 1][0] > 0 for i in ids)
    check_weighted(collide.reshape(2, 4, 120), raw, int(ids[-1]) + 1, device, 4)      # the 3-D table and its way to global memory
    check_border(collide.reshape(2, 4, 120), raw, int(ids[-1]) + 1, device, shift=4)
    one = np.ones((64, 64), np.int32)
    raw = _values(one.shape, 1, np.float64) * 2.0 ** 30
    _, rows = check_weighted(one, raw, 2, device, 4)
    assert rows[0][0] == one.size
    _, rows = check_border(one, raw, 2, device, shift=4)
    assert rows[0][0] == 4 * 63


def test_grid_above_the_launch_caps(device):
    """more than 1024 tiles of 1024 pixels (1025 x 1028): every block takes a second tile; objects span block ranges, touch
    along rows and reach into the tail tile; uint8-sized values keep an int64 restatement exact and cheap"""
    labels = np.zeros((1025, 1028), np.int32)
    labels[10:500, 20:600] = 1
    labels[500:1020, 20:300] = 2
    labels[300:900, 700:1000] = 4
    labels[1021:, :] = 3
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, size=labels.shape).astype(np.int32)
    words, rows = check_weighted(labels, raw, 5, device, small=True)
    assert sum(r[0] for r in rows) == int((labels > 0).sum())
    again, _ = call_weighted(labels, raw, 5, 0, ref_max_keys(labels, raw, 5), device, fill=0x5C)    # the same bits in every run
    assert again[1:].tobytes() == words.tobytes()
    check_weighted(labels, raw.astype(np.float32), 5, device, small=True, offsets=(0, 1))
    words, rows = check_border(labels, raw, 5, device, small=True)
    assert rows[0][0] == 2 * 490 + 2 * 580 - 4 and rows[2][0] == 2 * 1028 + 2 * 4 - 4
    check_border(labels, raw.astype(np.float32), 5, device, small=True, offsets=(1, 0))


def test_peak(device):
    """ties inside a lane, across lanes, across tiles and across blocks: the smallest flat index wins; -0.0 against +0.0; no
    keys; a key that no pixel has"""
    labels = np.zeros((1200, 1030), np.int32)                # 1207 tiles: blocks take two
    labels[:, :] = 1
    labels[5:9, 100:900] = 2
    labels[700:, 3:1000] = 3
    raw = np.random.default_rng(1).integers(0, 100, size=labels.shape).astype(np.float32)
    flat = raw.reshape(-1)
    for p in (8 * 1030 + 112, 8 * 1030 + 113, 8 * 1030 + 300, 5 * 1030 + 897):       # object 2: one lane, two lanes, an earlier row
        flat[p] = 500.0
    for p in (1199 * 1030 + 999, 900 * 1030 + 3, 701 * 1030 + 640):                   # object 3: far apart, in several blocks
        flat[p] = 777.0
    for p in (1199 * 1030 + 1029, 650 * 1030 + 1010, 2):                              # object 1: the last pixel, the middle, the third
        flat[p] = 900.0
    words, rows = check_weighted(labels, raw, 4, device, small=True)
    assert [r[2] for r in rows] == [2, 5 * 1030 + 897, 701 * 1030 + 640]
    none, _ = call_weighted(labels, raw, 4, 0, None, device)
    assert (none[1:, 2] == NO_PEAK).all() and np.array_equal(np.delete(none[1:], 2, axis=1), np.delete(words, 2, axis=1))
    keys = ref_max_keys(labels, raw, 4)
    keys[2] = ref_keys(np.array([12345.0], np.float32))[0]   # no pixel has this value
    words, rows = check_weighted(labels, raw, 4, device, peak=keys, small=True)
    assert rows[1][2] == NO_PEAK and rows[0][2] == 2
    # -0.0 sorts below +0.0: the peak of {-0.0, +0.0} is the first +0.0; the quantised values are all 0
    for dtype in (np.float32, np.float64):
        zeros = np.full((3, 50), -0.0, dtype)
        zeros[1, 17] = zeros[2, 4] = 0.0
        lab = np.ones((3, 50), np.int32)
        _, rows = check_weighted(lab, zeros, 2, device, 3)
        assert rows[0][2] == 67 and rows[0][1] == 0
    ints = np.full((3, 50), -7, np.int32)
    ints[2, 49] = ints[1, 0] = -6
    _, rows = check_weighted(np.ones((3, 50), np.int32), ints, 2, device)
    assert rows[0][2] == 50


def test_border_cases(device):
    """objects on the image edge, X = 1, one-pixel objects, a checkerboard, neighbours that differ only in z, nd = 3 with Z = 1
    against nd = 2, neighbours across lane 63 / lane 0 and across tile and block ends"""
    rng = np.random.default_rng(2)

    def both(labels, nid, **kw):
        raw = rng.integers(-999, 1000, size=labels.shape).astype(np.int32)
        return check_border(labels, raw, nid, device, **kw)[1]

    edge = np.zeros((12, 20), np.int32)
    edge[:4, :5] = 1
    edge[8:, 15:] = 2
    edge[5, 9] = 3                                           # one pixel
    edge[0, 19] = 4
    rows = both(edge, 5)
    assert [r[0] for r in rows] == [14, 14, 1, 1]
    column = np.array([1, 1, 1, 0, 2, 2, 2, 2, 2, 3], np.int32).reshape(-1, 1)       # X = 1
    assert [r[0] for r in both(column, 4)] == [3, 5, 1]
    yy, xx = np.indices((16, 70))
    board = ((yy + xx) % 2 + 1).astype(np.int32)
    assert [r[0] for r in both(board, 3)] == [560, 560]
    stack = np.ones((6, 9, 12), np.int32)                    # a block of one id whose layers 2 and 3 carry another id inside
    stack[2:4, 3:6, 4:8] = 2
    rows = both(stack, 3)
    mask = ref_border_mask(stack, 3, 3)
    assert mask[1, 4, 5] and mask[4, 4, 5] and rows[1][0] == 24
    assert not ref_border_mask(stack[1], 3, 2)[4, 5]         # in 2-D that pixel is interior: only z tells
    flat = _blobs((1, 30, 41), 6, 9)
    flat[flat == 0] = 7
    rows3 = both(flat, 8, nd=3)
    assert [r[0] for r in rows3] == [int((flat == i).sum()) for i in range(1, 8)]     # Z = 1: every pixel is a border pixel
    rows2 = both(flat[0], 8)
    assert sum(r[0] for r in rows2) < sum(r[0] for r in rows3)
    # one object whose ends fall on lane, wave, tile and block ends; rows of 256, 1024 and 4096 pixels put the neighbours in
    # y at the same lane of another wave, tile and block
    for X in (256, 1024, 4096):
        lab = np.zeros((6, X), np.int32)
        lab[1:5, :] = 1
        lab[2, 255] = lab[3, X // 2] = lab[2, X - 1] = 2
        lab[1:4, 0] = 3
        rows = both(lab, 4)
        assert rows[0][0] > 2 * X
        both(np.concatenate([lab[None], lab[None][:, ::-1]]), 4)             # 3-D: planes of 6 X
    # three equal rows of 3072 pixels: in the middle one only x tells, at the ends of a lane, a wave, a tile and a block
    line = np.ones((3, 3072), np.int32)
    line[:, 256:260] = 2
    line[:, 1023] = 3
    line[:, 1024] = 4
    line[:, 2048:] = 5
    assert [r[0] for r in both(line, 6)] == [2 * 2042 + 6, 2 * 4 + 2, 3, 3, 2 * 1024 + 2]


def test_border_pixels_equal_perimeter_class_0(device):
    from cellulus_amd import _clx

    for shape, n, seed in (((33, 31), 7, 1), ((9, 130), 6, 2), ((40, 131), 25, 3)):
        labels = _blobs(shape, n, seed)
        labels[labels == 0] = np.where(np.indices(shape)[1] % 9 == 0, 0, n + 1)[labels == 0]       # touching neighbours too
        nid = n + 2
        words, _ = check_border(labels, np.zeros(shape, np.int32), nid, device)
        classes, bad = Out((nid, 4), np.uint64, device), Out((1,), np.int32, device)
        lab = _dev(labels, device)
        assert _clx.load().clx_region_perimeter(_clx.ptr(lab), *shape, nid, classes.ptr, bad.ptr, _clx.stream_ptr(device)) == 0
        torch.cuda.synchronize(device)
        assert np.array_equal(classes.get()[1:, 0], words[:, 0]) and words[:, 0].sum() > 0


def test_invariants(device):
    labels = _blobs((40, 70), 12, 21)
    nid = int(labels.max()) + 2
    for kind, shift in (("f32", 9), ("f64", 20), ("i32", 0)):
        raw = _raw(kind, labels.shape, 4)
        whole, _ = run_intensity(labels, raw, nid, shift, device)
        assert whole["bad"][0] == 0
        words, rows = check_weighted(labels, raw, nid, device, shift, peak=whole["vkey"][:, 1])
        # Σq is clx_region_intensity's isum bit for bit, and the peak carries the largest value
        assert np.array_equal(words[:, 1].view(np.int64), whole["isum"][1:])
        flat = raw.reshape(-1)
        for i, r in enumerate(rows, 1):
            if r[0]:
                assert flat[r[2]] == raw[labels == i].max() and labels.reshape(-1)[r[2]] == i
    # a constant channel: the weighted sums are the coordinate sums times the constant
    ones = np.full(labels.shape, 3, np.int32)
    _, rows = check_weighted(labels, ones, nid, device)
    z, y, x = np.indices(_zyx(labels))
    for i in (1, 5, nid - 2):
        m = (labels == i).reshape(_zyx(labels))
        assert rows[i - 1][5] == 3 * int(x[m].sum()) and rows[i - 1][11] == 3 * int((y[m] * x[m]).sum())


def test_every_bad_bit_alone(device):
    labels = _blobs((12, 70), 9, 5)
    nid = int(labels.max()) + 2
    raw = _values(labels.shape, 8, np.float64)
    clean_w, _ = check_weighted(labels, raw, nid, device, 4)
    clean_b, _ = check_border(labels, raw, nid, device, shift=4)
    ys, xs = np.nonzero(labels)
    interior = ~ref_border_mask(labels, nid, 2) & (labels > 0)
    iy, ix = np.argwhere(interior)[0]
    # bit 0: labels outside [0, nid) count as background, and make border pixels of their neighbours
    for value in (nid, 2 ** 31 - 1, -1, -2 ** 31):
        lab = labels.copy()
        lab[ys[::29], xs[::29]] = value
        lab[0, 0] = value
        lab[iy, ix] = value
        words, _ = check_weighted(lab, raw, nid, device, 4, want_bad=BAD_LABEL)
        want, bad = ref_weighted(np.where(lab == value, 0, lab), raw, nid, 4, ref_max_keys(lab, raw, nid, 4))
        assert bad == 0 and np.array_equal(words, weighted_words(want)[1:])
        words, _ = check_border(lab, raw, nid, device, shift=4, want_bad=BAD_LABEL)
        want, bad = ref_border(np.where(lab == value, 0, lab), raw, nid, 2, 4)
        assert bad == 0 and np.array_equal(words, border_words(want)[1:])
        assert ref_border_mask(lab, nid, 2)[iy, ix + 1] or ref_border_mask(lab, nid, 2)[iy, ix - 1]
    # bit 1: a NaN, an Inf, a value above the per-pixel bound: on the background ignored, under an object skipped
    on_border = np.argwhere(ref_border_mask(labels, nid, 2))[3]
    for poison in (np.nan, np.inf, -np.inf, 2.0 ** 60):
        r = raw.copy()
        r[labels == 0] = poison
        assert np.array_equal(check_weighted(labels, r, nid, device, 4)[0], clean_w)
        assert np.array_equal(check_border(labels, r, nid, device, shift=4)[0], clean_b)
        r = raw.copy()
        r[tuple(on_border)] = poison
        hit = labels[tuple(on_border)] - 1
        words, _ = check_weighted(labels, r, nid, device, 4, want_bad=BAD_VALUE)
        assert words[hit, 0] == clean_w[hit, 0] - 1
        words, _ = check_border(labels, r, nid, device, shift=4, want_bad=BAD_VALUE)
        assert words[hit, 0] == clean_b[hit, 0] and words[hit, 1] == clean_b[hit, 1] - 1     # counted in word 0, not in word 1
        # an unfit value inside an object is none of the border kernel's business
        r = raw.copy()
        r[iy, ix] = poison
        assert np.array_equal(check_border(labels, r, nid, device, shift=4)[0], clean_b)
        check_weighted(labels, r, nid, device, 4, want_bad=BAD_VALUE)
    # both bits together
    lab = labels.copy()
    lab[0, 0] = nid
    r = raw.copy()
    r[tuple(on_border)] = np.nan
    check_weighted(lab, r, nid, device, 4, want_bad=BAD_LABEL | BAD_VALUE)
    check_border(lab, r, nid, device, shift=4, want_bad=BAD_LABEL | BAD_VALUE)


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    zeros = torch.zeros(4096, dtype=torch.int64, device=device)
    outs = {k: Out((4096,), np.int64, device) for k in ("out", "bad")}
    null = ctypes.c_void_p(0)

    def message():
        return lib.clx_last_error().decode()

    def weighted(raw_type=F32, Z=1, Y=8, X=8, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(zeros), raw=_clx.ptr(zeros), keys=_clx.ptr(zeros), out=outs["out"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_weighted(p["labels"], p["raw"], raw_type, Z, Y, X, nid, 0, p["keys"], p["out"], p["bad"], st)

    def border(raw_type=F32, nd=2, Z=1, Y=8, X=8, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(zeros), raw=_clx.ptr(zeros), out=outs["out"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_border_intensity(p["labels"], p["raw"], raw_type, nd, Z, Y, X, nid, 0, p["out"], p["bad"], st)

    shapes = [(dict(Z=0), "shape"), (dict(Y=0), "shape"), (dict(X=-1), "shape"), (dict(Z=2 ** 11, Y=2 ** 11, X=2 ** 10), "2^32"),
              (dict(Z=1, Y=2 ** 16, X=2 ** 16), "2^32")]
    common = [(dict(raw_type=3), "raw_type"), (dict(raw_type=-1), "raw_type"), (dict(nid=0), "nid"), (dict(nid=-3), "nid"),
              (dict(nid=2 ** 24 + 1), "nid")]
    refused = [("clx_region_weighted", lambda kw=kw: weighted(**kw), word) for kw, word in
               [({k: null}, "null") for k in ("labels", "raw", "out", "bad")] + common + shapes]
    refused += [("clx_region_border_intensity", lambda kw=kw: border(**kw), word) for kw, word in
                [({k: null}, "null") for k in ("labels", "raw", "out", "bad")] + common +
                [(dict(nd=3, **kw), word) for kw, word in shapes] + [(dict(nd=1), "nd"), (dict(nd=4), "nd"), (dict(nd=2, Z=2), "nd == 2")]]
    for i, (who, call, word) in enumerate(refused):
        status = call()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message().startswith(who) and word in message(), f"case {i}: {message()!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    # accepted: every raw type, with and without keys, both nd
    assert weighted() == 0 and weighted(keys=null) == 0 and weighted(raw_type=F64) == 0 and weighted(raw_type=I32, Z=2, Y=4) == 0, message()
    torch.cuda.synchronize(device)
    got = outs["out"].get().view(np.uint64)[:4 * NW].reshape(4, NW)
    assert int(outs["bad"].get().view(np.int32)[0]) == 0 and (got[:, 2] == NO_PEAK).all() and not np.delete(got, 2, axis=1).any()
    assert border() == 0 and border(raw_type=F64) == 0 and border(raw_type=I32, nd=3, Z=2, Y=4) == 0, message()
    torch.cuda.synchronize(device)
    got = outs["out"].get().view(np.uint64)[:4 * NB].reshape(4, NB)
    assert int(outs["bad"].get().view(np.int32)[0]) == 0 and (got[:, 3] == NO_PEAK).all() and not np.delete(got, 3, axis=1).any()
