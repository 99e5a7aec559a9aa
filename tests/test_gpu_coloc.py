"""clx_region_products through the C ABI against the restatement of tests/coloc_ref.py (Python-int sums of products per id).
Everything is integer work: all twenty words of every id from 1 up and bad must be EQUAL.  The outputs are prefilled with 0xAB
bytes (or other garbage) and sit between guard words that must stay untouched."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

from coloc_ref import BAD_LABEL, BAD_VALUE, NW, ref_products, words_of
from test_gpu_measure import F32, F64, GUARD, I32, Out, _blobs, _dev, _raw, run_intensity, run_moments

pytestmark = pytest.mark.gpu

RAW_TYPE = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def call_products(labels, raw_a, raw_b, nid, shift_a, shift_b, thr_a, thr_b, device, offsets=(0, 0, 0), fill=0xAB, same=False):
    """one clx_region_products call -> (words uint64 (nid, 20), bad); guard words checked.  offsets: elements by which the label,
    raw_a and raw_b pointers are moved off their 16-byte-aligned allocations; same: raw_b is raw_a's pointer"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    raw_a, raw_b = np.ascontiguousarray(raw_a), np.ascontiguousarray(raw_b)
    assert raw_a.dtype == raw_b.dtype and raw_a.size == raw_b.size == labels.size
    lab = _dev(labels, device, offsets[0])
    a_d = _dev(raw_a, device, offsets[1])
    b_d = a_d if same else _dev(raw_b, device, offsets[2])
    ta = None if thr_a is None else _dev(np.asarray(thr_a, dtype=np.int64), device)
    tb = None if thr_b is None else _dev(np.asarray(thr_b, dtype=np.int64), device)
    out, bad = Out((nid, NW), np.uint64, device), Out((1,), np.int32, device)
    for o in (out, bad):
        o.buf[GUARD:GUARD + o.nbytes] = fill
    lib = _clx.load()
    status = lib.clx_region_products(_clx.ptr(lab), _clx.ptr(a_d), _clx.ptr(b_d), RAW_TYPE[raw_a.dtype], labels.size, nid, shift_a,
                                     shift_b, _clx.ptr(ta), _clx.ptr(tb), out.ptr, bad.ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return out.get(), int(bad.get()[0])


def check(labels, raw_a, raw_b, nid, device, shift_a=0, shift_b=0, thr_a=None, thr_b=None, want_bad=0, small=False, **kw):
    """-> (words from id 1 up, the restatement's rows from id 1 up) after comparing every word and bad"""
    words, bad = call_products(labels, raw_a, raw_b, nid, shift_a, shift_b, thr_a, thr_b, device, **kw)
    rows, ref_bad = ref_products(labels, raw_a, raw_b, nid, shift_a, shift_b, thr_a, thr_b, small=small)
    want = words_of(rows)
    differ = np.argwhere(words[1:] != want[1:])
    assert len(differ) == 0, (len(differ), [(p.tolist(), hex(int(words[1:][tuple(p)])), hex(int(want[1:][tuple(p)]))) for p in differ[:4]])
    assert bad == ref_bad == want_bad
    return words[1:], rows[1:]


def _values(shape, seed, dtype=np.float32):
    """values that quantise exactly at shift 4: multiples of 1/16 in (-2048, 2048)"""
    return (np.random.default_rng(seed).integers(-2 ** 15, 2 ** 15, size=shape) / 16.0).astype(dtype)


def _thresholds(nid, seed, lo=-2 ** 15, hi=2 ** 15):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, size=nid), rng.integers(lo, hi, size=nid)


SHAPES = [(1, 1), (3, 5), (7, 129), (33, 31), (5, 4, 37), (9, 130)]


@pytest.mark.parametrize("offsets", list(itertools.product((0, 1, 3), repeat=3)), ids=lambda o: "".join(map(str, o)))
def test_row_ends_and_tails(offsets, device):
    """lanes whose 4 pixels straddle runs, the scalar tail past the last whole lane, a second tile that is a tail, and the
    16-byte or 4-byte loads decided for each of the three pointers alone"""
    for shape in SHAPES:
        labels = _blobs(shape, 5, 3 + len(shape)).reshape(-1)
        if labels.max() == 0:
            labels[:] = 1
        nid = int(labels.max()) + 2                          # the last id is absent
        a, b = _values(labels.shape, 2), _values(labels.shape, 7)
        ta, tb = _thresholds(nid, 5)
        check(labels, a, b, nid, device, 4, 4, ta, tb, offsets=offsets)
        check(labels, a, b, nid, device, 4, 2, offsets=offsets)
    labels = _blobs((9, 130), 6, 1).reshape(-1)
    check(labels, _values(labels.shape, 3, np.float64), _values(labels.shape, 4, np.float64), 8, device, 4, 4, *_thresholds(8, 1), offsets=offsets)
    check(labels, _raw("i32", labels.shape, 3).reshape(-1), _raw("i32", labels.shape, 4).reshape(-1), 8, device, offsets=offsets)


@pytest.mark.parametrize("kind", ["f32", "f64", "i32"])
def test_raw_types(kind, device):
    from cellulus_amd.measure import intensity_shift

    labels = _blobs((12, 70), 9, 5)
    a, b = _raw(kind, labels.shape, 11), -_raw(kind, labels.shape, 12)       # negative values among them
    sa = 0 if kind == "i32" else intensity_shift(float(np.abs(a.astype(np.float64)).max()), labels.size)
    sb = 0 if kind == "i32" else intensity_shift(float(np.abs(b.astype(np.float64)).max()), labels.size) - 3
    _, rows = check(labels, a, b, 11, device, sa, sb)
    assert any(r[1] < 0 for r in rows) and any(r[1] > 0 for r in rows) and any(r[10] < 0 for r in rows)
    if kind != "i32":
        assert max(r[8] for r in rows) > 2 ** 64             # the shift fills the 62 - L bits: squares need the high limb
    qa_max = max(abs(r[1]) for r in rows)
    check(labels, a, b, 11, device, sa, sb, *_thresholds(11, 3, -qa_max // 50, qa_max // 50))


def test_shift_at_both_clamps(device):
    """intensity_shift clamps to [-1022, 1023]: float64 values near the ends of the exponent range"""
    labels = _blobs((9, 40), 6, 8)
    rng = np.random.default_rng(6)
    tiny = rng.integers(-2 ** 20, 2 ** 20, size=labels.shape) * 2.0 ** -1040          # multiples of 2^-1040, subnormals among them
    huge = rng.integers(-2 ** 20, 2 ** 20, size=labels.shape) * 2.0 ** 1003
    _, rows = check(labels, tiny, huge, 8, device, 1023, -1022)
    assert any(r[8] for r in rows) and any(r[9] for r in rows) and max(abs(r[2]) for r in rows) < 2 ** 12
    check(labels, huge, tiny, 8, device, -1022, 1023, *_thresholds(8, 2, -8, 8))


def test_128_bit_sums(device):
    """the low limb wraps many times, a negative cross sum borrows from the high limb, and products near 2^98"""
    m = 2 ** 31 - 1
    labels = np.ones((32, 32), np.int32)
    a = np.where(np.indices(labels.shape).sum(axis=0) % 3 == 0, -m, m).astype(np.int32)
    words, rows = check(labels, a, -a, 2, device)
    assert rows[0][8] == 1024 * m * m > 2 ** 71 and rows[0][10] == -1024 * m * m
    assert int(words[0][13]) >> 63 == 1 and int(words[0][9]) == (1024 * m * m) >> 64    # a negative high limb; 2^7 wraps of the low one
    check(labels, a, -a, 2, device, thr_a=[0, 0], thr_b=[0, 0])                     # no pixel is above both
    check(labels, a, a // 3, 2, device, thr_a=[0, -m], thr_b=[0, -m // 3])
    # float64 at the per-pixel bound of a 64 x 64 map: L = 13, |q| <= 2^49, products up to 2^98, sums up to 2^110
    labels = _blobs((64, 64), 7, 3)
    labels[labels == 0] = 8
    rng = np.random.default_rng(4)
    big = np.where(rng.random(labels.shape) < 0.5, 2.0 ** 49, -(2.0 ** 49)) - rng.integers(-3, 4, size=labels.shape) * (rng.random(labels.shape) < 0.5)
    big = np.clip(big, -(2.0 ** 49), 2.0 ** 49)
    other = np.where(rng.random(labels.shape) < 0.5, 2.0 ** 49, -(2.0 ** 49) + 1)
    _, rows = check(labels, big, other, 9, device)
    assert max(r[8] for r in rows) > 2 ** 106 and min(r[10] for r in rows) < 0
    check(labels, big, other, 9, device, thr_a=[0] * 9, thr_b=[2 ** 49] * 9)
    # shift 1 moves the same values over the bound: every pixel is refused
    words, bad = call_products(labels, big, other, 9, 1, 1, None, None, device)
    assert bad == BAD_VALUE and not words[1:].any()


def test_invariants(device):
    labels = _blobs((40, 70), 12, 21)
    nid = int(labels.max()) + 2
    area = run_moments(labels, nid, device)["area"].astype(np.int64)
    for kind, sa, sb in (("f32", 9, 5), ("f64", 20, 23), ("i32", 0, 0)):
        a, b = _raw(kind, labels.shape, 4), _raw(kind, labels.shape, 5)
        words, rows = check(labels, a, b, nid, device, sa, sb)
        # Σa, Σb are clx_region_intensity's isum bit for bit, n the area
        for column, raw, shift in ((1, a, sa), (2, b, sb)):
            whole = run_intensity(labels, raw, nid, shift, device)[0]
            assert whole["bad"][0] == 0 and np.array_equal(words[:, column].view(np.int64), whole["isum"][1:])
        assert np.array_equal(words[:, 0].view(np.int64), area[1:])
        # no thresholds: the conditioned words equal the unconditioned ones
        assert np.array_equal(words[:, 3], words[:, 0]) and np.array_equal(words[:, 4], words[:, 1]) and np.array_equal(words[:, 5], words[:, 2])
        assert np.array_equal(words[:, 6], words[:, 1]) and np.array_equal(words[:, 7], words[:, 2]) and np.array_equal(words[:, 14:20], words[:, 8:14])
        # thresholds below every value do the same
        low, _ = check(labels, a, b, nid, device, sa, sb, [I64_MIN] * nid, [I64_MIN] * nid)
        assert np.array_equal(low, words)
        # swapping the channels swaps the words
        ta, tb = _thresholds(nid, 9, -2 ** 9, 2 ** 9)
        ab, _ = check(labels, a, b, nid, device, sa, sb, ta, tb)
        ba, _ = check(labels, b, a, nid, device, sb, sa, tb, ta)
        swap = [0, 2, 1, 3, 5, 4, 7, 6, 10, 11, 8, 9, 12, 13, 16, 17, 14, 15, 18, 19]
        assert np.array_equal(ba, ab[:, swap])
        # a == b (one pointer): the three second-order sums are equal
        for thr in (None, ta):
            same, _ = check(labels, a, a, nid, device, sa, sa, thr, thr, same=True)
            assert np.array_equal(same[:, 8:10], same[:, 10:12]) and np.array_equal(same[:, 8:10], same[:, 12:14])
            assert np.array_equal(same[:, 14:16], same[:, 16:18]) and np.array_equal(same[:, 14:16], same[:, 18:20])


def test_thresholds(device):
    """per-id thresholds equal to, one below and one above pixel values, and the ends of int64"""
    labels = np.repeat(np.arange(1, 9, dtype=np.int32), 40).reshape(8, 40)
    rng = np.random.default_rng(8)
    a = rng.integers(-20, 21, size=labels.shape).astype(np.int32)
    b = rng.integers(-20, 21, size=labels.shape).astype(np.int32)
    nid = 10
    ta = [0, 5, 4, 6, I64_MIN, I64_MAX, -20, 21, 0, 0]
    tb = [0, -3, -4, -2, I64_MIN, 0, I64_MAX, -20, 20, 0]
    words, rows = check(labels, a, b, nid, device, thr_a=ta, thr_b=tb)
    for i in (1, 2, 3):                                      # at, below and above the value 5: the pixels equal to it move
        assert rows[i - 1][4] == int(a[i - 1][a[i - 1] >= ta[i]].sum())
    assert rows[3][3] == 40 and rows[4][3] == 0 and rows[5][3] == 0 and rows[4][4] == 0 and rows[5][5] == 0
    assert rows[4][5] == int(b[4][b[4] >= 0].sum()) and rows[6][3] == 0 and rows[6][4] == 0
    f = _values(labels.shape, 3, np.float64)
    q = np.rint(f * 16).astype(np.int64)
    for delta in (-1, 0, 1):
        ta = [0] + [int(q[i, 7]) + delta for i in range(8)] + [0]
        tb = [0] + [int(q[i, 9]) - delta for i in range(8)] + [0]
        check(labels, f, f[::-1].copy(), nid, device, 4, 4, ta, tb)


def test_lds_table(device):
    """far more ids than the 256 slots of a block's table (most go straight to global memory), more ids congruent modulo the slot
    count in one tile than find_slot probes, and one object over a whole map, every lane of every wave in the same slot"""
    rng = np.random.default_rng(3)
    many = rng.integers(1, 2001, size=(40, 100)).astype(np.int32)
    a, b = _values(many.shape, 9), _values(many.shape, 10)
    check(many, a, b, 2001, device, 4, 4)
    check(many, a, b, 2001, device, 4, 4, *_thresholds(2001, 4), offsets=(1, 0, 3))
    ids = 1 + 256 * np.arange(20, dtype=np.int32)            # 20 ids in slot 1's chain: PROBES = 8 of them fit
    collide = np.repeat(ids, 48).reshape(-1)[:1000]
    rng.shuffle(collide[400:])                               # runs, then single pixels
    a, b = _values(collide.shape, 1), _values(collide.shape, 2)
    _, rows = check(collide, a, b, int(ids[-1]) + 1, device, 4, 4, *_thresholds(int(ids[-1]) + 1, 6))
    assert all(rows[i - 1][0] > 0 for i in ids)
    one = np.ones((64, 64), np.int32)
    a, b = _values(one.shape, 1, np.float64) * 2.0 ** 30, _values(one.shape, 2, np.float64) * 2.0 ** 30
    for thr in (None, [0, 2 ** 33]):
        _, rows = check(one, a, b, 2, device, 4, 4, thr, thr)
        assert rows[0][0] == one.size and rows[0][8] > 2 ** 64


def test_grid_above_the_launch_cap(device):
    """more than 1024 tiles of 1024 pixels: every block takes a second tile; four objects and uint8-sized values keep an int64
    restatement exact and cheap"""
    labels = np.zeros((1025, 1024), np.int32)
    labels[10:500, 20:600] = 1
    labels[500:1020, 20:300] = 2                             # touches 1 along a row
    labels[300:900, 700:1000] = 4
    labels[1021:, :] = 3                                     # the last rows, into the tail tile
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=labels.shape).astype(np.int32)
    b = rng.integers(0, 256, size=labels.shape).astype(np.int32)
    ta, tb = [0, 38, 100, 0, 255], [0, 38, 0, 200, 256]
    words, rows = check(labels, a, b, 5, device, thr_a=ta, thr_b=tb, small=True)
    assert sum(r[0] for r in rows) == int((labels > 0).sum()) and rows[3][3] == 0
    again, _ = call_products(labels, a, b, 5, 0, 0, ta, tb, device, fill=0x5C)                # the same bits in every run
    assert again[1:].tobytes() == words.tobytes()
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    check(labels, fa, fb, 5, device, small=True, offsets=(0, 1, 0))


def test_every_bad_bit_alone(device):
    labels = _blobs((12, 70), 9, 5)
    nid = int(labels.max()) + 2
    a, b = _values(labels.shape, 8, np.float64), _values(labels.shape, 9, np.float64)
    ta, tb = _thresholds(nid, 1, -2 ** 10, 2 ** 10)
    clean, _ = check(labels, a, b, nid, device, 4, 4, ta, tb)
    ys, xs = np.nonzero(labels)
    # bit 0: labels outside [0, nid) count as background; every other pixel still lands
    for value in (nid, 2 ** 31 - 1, -1, -2 ** 31):
        lab = labels.copy()
        lab[ys[::29], xs[::29]] = value
        lab[0, 0] = value
        words, _ = check(lab, a, b, nid, device, 4, 4, ta, tb, want_bad=BAD_LABEL)
        want, bad = ref_products(np.where(lab == value, 0, lab), a, b, nid, 4, 4, ta, tb)
        assert bad == 0 and np.array_equal(words, words_of(want)[1:])
    # bit 1: a NaN, an Inf, a value above the per-pixel bound, in channel a only and in channel b only: the pixel is skipped
    # in all twenty words; on the background such values are ignored
    hit = labels[ys[7], xs[7]] - 1
    others = np.arange(nid - 1) != hit
    for poison in (np.nan, np.inf, -np.inf, 2.0 ** 60):
        for in_a in (True, False):
            ra, rb = a.copy(), b.copy()
            (ra if in_a else rb)[labels == 0] = poison
            words, _ = check(labels, ra, rb, nid, device, 4, 4, ta, tb)
            assert np.array_equal(words, clean)
            ra, rb = a.copy(), b.copy()
            (ra if in_a else rb)[ys[7], xs[7]] = poison
            words, _ = check(labels, ra, rb, nid, device, 4, 4, ta, tb, want_bad=BAD_VALUE)
            assert np.array_equal(words[others], clean[others]) and words[hit, 0] == clean[hit, 0] - 1
            skipped = labels.copy()
            skipped[ys[7], xs[7]] = 0
            want, _ = ref_products(skipped, a, b, nid, 4, 4, ta, tb)
            assert np.array_equal(words, words_of(want)[1:])
    # both bits together
    lab = labels.copy()
    lab[0, 0] = nid
    ra = a.copy()
    ra[ys[7], xs[7]] = np.nan
    check(lab, ra, b, nid, device, 4, 4, want_bad=BAD_LABEL | BAD_VALUE)


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    zeros = torch.zeros(4096, dtype=torch.int64, device=device)
    outs = {k: Out((4096,), np.int64, device) for k in ("out", "bad")}
    null = ctypes.c_void_p(0)

    def message():
        m = lib.clx_last_error()
        return m.decode() if isinstance(m, bytes) else str(m)

    def products(raw_type=F32, npix=64, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(zeros), raw_a=_clx.ptr(zeros), raw_b=_clx.ptr(zeros), thr_a=_clx.ptr(zeros), thr_b=_clx.ptr(zeros),
                 out=outs["out"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_products(p["labels"], p["raw_a"], p["raw_b"], raw_type, npix, nid, 0, 0, p["thr_a"], p["thr_b"], p["out"],
                                       p["bad"], st)

    refused = [(lambda k=k: products(**{k: null}), "null") for k in ("labels", "raw_a", "raw_b", "out", "bad", "thr_a", "thr_b")] + [
        (lambda: products(raw_type=3), "raw_type"), (lambda: products(raw_type=-1), "raw_type"),
        (lambda: products(nid=0), "nid"), (lambda: products(nid=-3), "nid"), (lambda: products(nid=2 ** 24 + 1), "nid"),
        (lambda: products(npix=0), "npix"), (lambda: products(npix=-1), "npix"), (lambda: products(npix=2 ** 32), "npix"),
    ]
    for i, (call, word) in enumerate(refused):
        status = call()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message().startswith("clx_region_products") and word in message(), f"case {i}: {message()!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    # accepted: with and without the threshold pair, every raw type, one pointer for both channels
    assert products() == 0 and products(thr_a=null, thr_b=null) == 0 and products(raw_type=F64) == 0 and products(raw_type=I32) == 0, message()
    torch.cuda.synchronize(device)
    assert int(outs["bad"].get().view(np.int32)[0]) == 0 and not outs["out"].get()[:4 * NW].any()
