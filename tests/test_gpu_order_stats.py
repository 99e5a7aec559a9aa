"""clx_region_order_stats through the C ABI against the restatement of tests/order_ref.py (a plain sort of every object's
keys).  An order statistic is one of the values: every key must be EQUAL, for all three raw types.  The outputs and the
workspace are prefilled with 0xAB bytes (or other garbage) and sit between guard zones that must stay untouched; labels and
raw are also passed one element into their allocations.  The lengths at which the select kernel changes its method are read
from the comment in DESIGN.md 3.3g that quotes them."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from order_ref import ABSENT, BAD_AREA, BAD_LABEL, BAD_RANK, BAD_VALUE, F32, F64, I32, decode_key, raw_type_of, ref_order_stats
from test_gpu_measure import GUARD, Out, _blobs, _dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f32": np.float32, "f64": np.float64, "i32": np.int32}


def thresholds():
    """SORT_MAX, BLOCK_MAX, PART_KEYS as DESIGN.md 3.3g quotes them from csrc/region_order.hip"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"<!-- region_order\.hip: SORT_MAX=(\d+) BLOCK_MAX=(\d+) PART_KEYS=(\d+) -->", text)
    assert m, "DESIGN.md 3.3g does not quote the select kernel's constants"
    return tuple(int(v) for v in m.groups())


def call_order(labels, raw, nid, rank, device, area=None, centre=None, offset=0, fill=0xAB, seg_base=None, total=None):
    """-> (out uint64 (nid, nq), bad) as the entry point left them; the guard zones of both and of the workspace are checked.
    area: what the caller claims (default: the truth); seg_base and total follow from it unless they are given too"""
    from cellulus_amd import _clx

    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    raw = np.ascontiguousarray(raw).reshape(-1)
    rank = np.ascontiguousarray(rank, dtype=np.uint64)
    nq = rank.shape[1]
    if area is None:
        area = np.bincount(labels[(labels >= 1) & (labels < nid)], minlength=nid)
    area = np.asarray(area, dtype=np.uint64).copy()
    counted = area.copy()
    counted[0] = 0
    seg_base = np.cumsum(counted) - counted if seg_base is None else np.asarray(seg_base, dtype=np.uint64)
    total = int(counted.sum()) if total is None else total
    lib = _clx.load()
    nbytes = lib.clx_region_order_workspace(total, nid)
    assert nbytes >= 8 * total + 8 * nid
    outs = dict(out=Out((nid, nq), np.uint64, device), bad=Out((1,), np.int32, device), work=Out((nbytes,), np.uint8, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    lab_d, raw_d = _dev(labels, device, offset), _dev(raw, device, offset)
    area_d, base_d, rank_d = (_dev(v.view(np.int64), device) for v in (area, seg_base, rank))
    centre_d = None if centre is None else _dev(np.asarray(centre, dtype=np.float64), device)
    status = lib.clx_region_order_stats(_clx.ptr(lab_d), _clx.ptr(raw_d), raw_type_of(raw), labels.size, nid, _clx.ptr(area_d),
                                        _clx.ptr(base_d), total, _clx.ptr(centre_d), _clx.ptr(rank_d), nq, outs["out"].ptr,
                                        outs["work"].ptr, nbytes, outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    outs["work"].get()
    return outs["out"].get(), int(outs["bad"].get()[0])


def spread_ranks(labels, nid, nq=6):
    """(nid, nq) ranks below every present id's area: both ends, both medians, the quartiles, then steps through the rest"""
    labels = np.asarray(labels).reshape(-1)
    area = np.bincount(labels[(labels >= 1) & (labels < nid)], minlength=nid).astype(np.int64)
    a = np.maximum(area, 1)
    cols = [0 * a, a - 1, (a - 1) // 2, a // 2, (a - 1) // 4, (3 * (a - 1)) // 4]
    cols += [((j * 2654435761) % (2 ** 32)) % a for j in range(1, nq - 5)]
    return np.stack(cols[:nq], axis=1).astype(np.uint64)


def assert_order_equal(labels, raw, nid, device, rank=None, rows=None, want_bad=0, **kw):
    rank = spread_ranks(labels, nid) if rank is None else rank
    out, bad = call_order(labels, raw, nid, rank, device, **kw)
    want, ref_bad = ref_order_stats(labels, raw, nid, rank, area=kw.get("area"), centre=kw.get("centre"))
    assert bad == ref_bad == want_bad, (bad, ref_bad, want_bad)
    rows = np.arange(1, nid) if rows is None else np.asarray(rows)
    differ = [(int(i), out[i].tolist(), want[i].tolist()) for i in rows if (out[i] != want[i]).any()]
    assert not differ, (len(differ), differ[:3])
    return out


def values_for(kind, shape, seed):
    """seeded raw of the dtype `kind` names, with ties, both signs and the edge values of the type"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "i32":
        v = rng.integers(-300, 300, n).astype(np.int32)
        v[rng.random(n) < 0.05] = -2 ** 31
        v[rng.random(n) < 0.05] = 2 ** 31 - 1
    else:
        v = np.round(rng.normal(size=n) * 8) / 4                                     # many ties
        v[rng.random(n) < 0.1] = -0.0
        v[rng.random(n) < 0.1] = 0.0
        tiny = 1e-45 if kind == "f32" else 5e-324                                    # denormals of the type
        v = v.astype(DTYPES[kind])
        v[rng.random(n) < 0.05] = tiny
        v[rng.random(n) < 0.05] = -tiny
        v[rng.random(n) < 0.03] = np.finfo(DTYPES[kind]).max
        v[rng.random(n) < 0.03] = np.finfo(DTYPES[kind]).min
    return v.reshape(shape)


def _maps():
    m = {}
    m["one_pixel"] = (np.ones((1, 1), np.int32), 2)
    m["areas_2_and_3"] = (np.array([[1, 2, 2, 0, 1, 2]], np.int32), 3)
    m["tail_lanes_5x67"] = (_blobs((5, 67), 6, 1), 7)
    m["one_label_3x1031"] = (np.full((3, 1031), 3, np.int32), 4)                     # one run per row, over many waves; ids 1, 2 absent
    m["distinct_16x70"] = (np.arange(1, 1121, dtype=np.int32).reshape(16, 70), 1121)
    yy, xx = np.indices((16, 70))
    m["checkerboard_16x70"] = (((yy + xx) % 2 + 1).astype(np.int32), 3)              # two cursors, every pixel its own stretch
    sparse = np.zeros((9, 33), np.int32)
    sparse[2, 5:9] = 1
    sparse[7, 30:] = 40
    sparse[8, 0] = 40
    sparse[4, 3:20] = 7
    m["absent_ids_between"] = (sparse, 42)
    m["separated_40x131"] = (_blobs((40, 131), 25, 2), 26)
    return m


MAPS = _maps()


@pytest.mark.parametrize("kind", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(MAPS))
def test_keys_equal_restatement(name, kind, device):
    labels, nid = MAPS[name]
    raw = values_for(kind, labels.shape, len(name))
    out = assert_order_equal(labels, raw, nid, device)
    present = np.unique(labels[labels > 0])
    absent = np.setdiff1d(np.arange(1, nid), present)
    assert (out[absent] == ABSENT).all() and (out[present] != ABSENT).all()
    assert_order_equal(labels, raw, nid, device, offset=1)                           # the 4-byte loads
    if name == "one_pixel":
        assert decode_key(out[1, :1], raw_type_of(raw)).tobytes() == raw.tobytes()


def test_every_rank_of_a_small_object(device):
    labels = np.zeros((4, 40), np.int32)
    labels[1, 3:35] = 1                                                              # 32 pixels: ranks 0 .. 31 at nq = 32
    labels[2:, 10:30] = 2
    for kind in sorted(DTYPES):
        raw = values_for(kind, labels.shape, 5)
        rank = np.zeros((3, 32), np.uint64)
        rank[1] = np.arange(32)
        rank[2] = np.arange(32) + 8
        out = assert_order_equal(labels, raw, 3, device, rank=rank)
        assert (np.diff(out[1].astype(object)) >= 0).all()
        for nq in (1, 2, 31):
            assert_order_equal(labels, raw, 3, device, rank=rank[:, :nq].copy())


def _digits_cases():
    c = {}
    # all values of an object equal: every histogram has one bin
    c["constant_f32"] = np.full(5000, -2.5, np.float32)
    c["constant_f64"] = np.full(5000, 1e300, np.float64)
    c["constant_i32"] = np.full(5000, 77, np.int32)
    rng = np.random.default_rng(8)
    # keys that differ in the lowest digit only, and in the highest only
    c["low_digit_i32"] = (1000 + rng.integers(0, 256, 5000)).astype(np.int32)
    c["high_digit_i32"] = np.array([-2 ** 31, 2 ** 31 - 1, 0, -1], np.int32)[rng.integers(0, 4, 5000)]
    c["low_digit_f32"] = (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, 5000).astype(np.uint32)).view(np.float32)
    c["signs_f32"] = np.array([-0.0, 0.0, -1e-45, 1e-45, -3e38, 3e38], np.float32)[rng.integers(0, 6, 5000)]
    c["signs_f64"] = np.array([-0.0, 0.0, -5e-324, 5e-324, -1e308, 1e308], np.float64)[rng.integers(0, 6, 5000)]
    # float64 values that differ only below bit 32 of their key
    c["below_bit_32_f64"] = (np.float64(1.5).view(np.uint64) + rng.integers(0, 2 ** 32, 5000).astype(np.uint64)).view(np.float64)
    c["low_digit_f64"] = (np.float64(-7.25).view(np.uint64) + rng.integers(0, 256, 5000).astype(np.uint64)).view(np.float64)
    # a long tie that straddles the ranks: 40 % below, a tie of 30 % around the median, the rest above
    tie = np.concatenate([rng.integers(0, 100, 2000), np.full(1500, 100), rng.integers(101, 200, 1500)])
    c["tie_i32"] = rng.permutation(tie).astype(np.int32)
    c["tie_f64"] = rng.permutation(tie).astype(np.float64) / 7
    return c


DIGITS = _digits_cases()


@pytest.mark.parametrize("name", sorted(DIGITS))
def test_digits_and_ties(name, device):
    """each value set as a short object (the LDS sort: its first 700 values) and as one above SORT_MAX (the radix select)"""
    values = DIGITS[name]
    sort_max = thresholds()[0]
    assert len(values) > sort_max
    labels = np.concatenate([np.full(700, 1), np.zeros(3), np.full(len(values), 2)]).astype(np.int32)
    raw = np.concatenate([values[:700], values[:3], values])
    assert_order_equal(labels, raw, 3, device, rank=spread_ranks(labels, 3, nq=12))


def _threshold_map():
    sort_max, block_max, part = thresholds()
    areas = [sort_max - 1, sort_max, sort_max + 1, block_max - 1, block_max, block_max + 1, block_max + part + 1]
    labels = np.concatenate([np.concatenate([np.full(a, i + 1), np.zeros(i % 3)]) for i, a in enumerate(areas)]).astype(np.int32)
    return labels, len(areas) + 1, areas


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_one_below_at_and_above_every_threshold(kind, device):
    """segments of SORT_MAX - 1, SORT_MAX, SORT_MAX + 1 keys (sort / one-block select), BLOCK_MAX - 1, BLOCK_MAX, BLOCK_MAX + 1
    (one block / many blocks) and one more part than that, in one map: the constants come from DESIGN.md 3.3g"""
    labels, nid, areas = _threshold_map()
    raw = values_for(kind, labels.shape, 11)
    rank = spread_ranks(labels, nid, nq=8)
    out = assert_order_equal(labels, raw, nid, device, rank=rank)
    assert (out[1:] != ABSENT).all()
    if kind == "f32":
        centre = np.arange(nid) + 0.5
        assert_order_equal(labels, raw, nid, device, rank=rank, centre=centre)


def test_one_object_above_the_launch_cap(device):
    """1031 x 1031 pixels of one id: more than MAX_GRID x TILE pixels for the gather, a segment longer than every threshold"""
    shape = (1031, 1031)
    assert shape[0] * shape[1] > 1024 * 1024 and shape[0] * shape[1] > thresholds()[1]
    labels = np.ones(shape, np.int32)
    rng = np.random.default_rng(4)
    raw16 = rng.integers(0, 65536, shape).astype(np.int32)                           # uint16 counts as int32
    rank = spread_ranks(labels, 2, nq=6)
    first = assert_order_equal(labels, raw16, 2, device, rank=rank)
    again, _ = call_order(labels, raw16, 2, rank, device, fill=0x5C)
    assert first[1:].tobytes() == again[1:].tobytes()
    raw64 = rng.normal(size=shape)
    assert_order_equal(labels, raw64, 2, device, rank=rank)
    assert_order_equal(labels, raw64, 2, device, rank=rank[:, :2].copy(), centre=np.array([0.0, 0.25]))
    # two long segments and short ones beside them
    labels[:, 500:] = 2
    labels[5:9, 3:40] = 3
    assert_order_equal(labels, raw16.astype(np.float32) * np.float32(0.37), 5, device)


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_centre_mode(kind, device):
    labels, nid = MAPS["separated_40x131"]
    raw = values_for(kind, labels.shape, 21)
    if kind != "i32":
        raw = np.clip(raw, -1e30, 1e30).astype(raw.dtype)                            # |v - c| stays finite
    centre = np.arange(nid) - nid / 2 + 0.5                                          # half-integers
    out = assert_order_equal(labels, raw, nid, device, centre=centre)
    present = np.unique(labels[labels > 0])
    assert (decode_key(out[present], F64) >= 0).all()
    assert_order_equal(labels, raw, nid, device, centre=centre, offset=1)
    # the keys decode as float64 whatever the raw type: |v - c| by hand
    lab = np.array([[1, 1, 1, 2]], np.int32)
    v = np.array([[3, -4, 10, 7]]).astype(raw.dtype)
    out, bad = call_order(lab, v, 3, np.array([[0, 0, 0], [0, 1, 2], [0, 0, 0]], np.uint64), device, centre=np.array([0.0, 2.5, 7.5]))
    assert bad == 0 and decode_key(out[1], F64).tolist() == [0.5, 6.5, 7.5] and decode_key(out[2], F64).tolist() == [0.5] * 3


def test_second_run_gives_equal_outputs(device):
    labels, nid, _ = _threshold_map()
    raw = values_for("f64", labels.shape, 3)
    rank = spread_ranks(labels, nid, nq=7)
    a, _ = call_order(labels, raw, nid, rank, device)
    b, _ = call_order(labels, raw, nid, rank, device, fill=0xFF)
    z, _ = call_order(labels, raw, nid, rank, device, fill=0)
    assert a[1:].tobytes() == b[1:].tobytes() == z[1:].tobytes()
    labels, nid = MAPS["checkerboard_16x70"]
    raw = values_for("f32", labels.shape, 3)
    a, _ = call_order(labels, raw, nid, spread_ranks(labels, nid), device)
    b, _ = call_order(labels, raw, nid, spread_ranks(labels, nid), device, fill=0)
    assert a[1:].tobytes() == b[1:].tobytes()


def test_flags(device):
    labels = _blobs((12, 70), 9, 5)
    nid = 10
    raw = values_for("f32", labels.shape, 6)
    raw = np.clip(raw, -1e30, 1e30).astype(np.float32)
    present = np.unique(labels[labels > 0])
    assert_order_equal(labels, raw, nid, device)
    # bit 0: a label outside [0, nid) is skipped
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[[3, 11, 0], [7, 69, 0]] = value
        assert_order_equal(lab, raw, nid, device, want_bad=BAD_LABEL)
    # bit 1: NaN and Inf under one object: the other rows are right; non-finite values on background are ignored
    victim = int(present[len(present) // 2])
    ys, xs = np.nonzero(labels == victim)
    for value in (np.nan, np.inf, -np.inf):
        v = raw.copy()
        v[labels == 0] = value
        assert_order_equal(labels, v, nid, device)
        v[ys[0], xs[0]] = value
        assert_order_equal(labels, v, nid, device, rows=[i for i in range(1, nid) if i != victim], want_bad=BAD_VALUE)
        assert_order_equal(labels, v.astype(np.float64), nid, device, rows=[i for i in range(1, nid) if i != victim], want_bad=BAD_VALUE)
    # bit 2: area one smaller and one larger than the truth for one id: the other rows are right
    truth = np.bincount(labels.reshape(-1), minlength=nid)
    assert truth[victim] >= 3
    rank = np.zeros((nid, 2), np.uint64)
    rank[:, 1] = np.maximum(truth, 2) - 2                                            # below the smaller area too
    rank[0] = 0
    ok_rows = [i for i in present if truth[i] >= 2 and i != victim]
    for delta in (-1, 1):
        area = truth.copy()
        area[victim] += delta
        assert_order_equal(labels, raw, nid, device, rank=rank, rows=ok_rows, want_bad=BAD_AREA, area=area)
    # bit 3: a rank equal to the area
    rank = spread_ranks(labels, nid)
    rank[victim, 2] = truth[victim]
    out = assert_order_equal(labels, raw, nid, device, rank=rank, want_bad=BAD_RANK)
    assert out[victim, 2] == ABSENT and (out[victim, :2] != ABSENT).all()
    # ... also where the segment is selected by radix passes
    long_labels, long_nid, areas = _threshold_map()
    long_raw = values_for("i32", long_labels.shape, 9)
    rank = spread_ranks(long_labels, long_nid)
    rank[3, 1] = areas[2]
    rank[7, 0] = areas[6] + 5
    out = assert_order_equal(long_labels, long_raw, long_nid, device, rank=rank, want_bad=BAD_RANK)
    assert out[3, 1] == ABSENT and out[7, 0] == ABSENT


def test_segments_that_disagree_with_area(device):
    """bit 2's third meaning: a seg_base that does not go with area.  A segment that does not lie inside [0, total) is neither
    read nor written (its row stays ~0, the guard zones around the workspace stay intact); segments that claim more long
    objects than total has room for overflow the list of long segments.  The rows that are consistent stay right."""
    labels = _blobs((12, 70), 9, 5)
    nid = 10
    raw = values_for("f32", labels.shape, 6)
    truth = np.bincount(labels.reshape(-1), minlength=nid)
    truth[0] = 0
    base = np.cumsum(truth) - truth
    total = int(truth.sum())
    present = np.flatnonzero(truth)
    victim = int(present[len(present) // 2])
    rank = spread_ranks(labels, nid)
    want, _ = ref_order_stats(labels, raw, nid, rank)
    others = [i for i in present if i != victim]
    for value in (total, total - truth[victim] + 1, 2 ** 40, 2 ** 64 - 1):            # at the end, one too far, far out, wrapping
        moved = base.astype(np.uint64)
        moved[victim] = value
        out, bad = call_order(labels, raw, nid, rank, device, seg_base=moved)
        assert bad == BAD_AREA and (out[victim] == ABSENT).all() and np.array_equal(out[others], want[others]), value
    # the same where the segment would be selected by radix passes by one block and by many: nothing of it is touched
    long_labels, long_nid, areas = _threshold_map()
    long_raw = values_for("i32", long_labels.shape, 9)
    long_rank = spread_ranks(long_labels, long_nid)
    long_want, _ = ref_order_stats(long_labels, long_raw, long_nid, long_rank)
    a = np.array([0] + areas)
    for victim in (4, 7):
        moved = (np.cumsum(a) - a).astype(np.uint64)
        moved[victim] = int(a.sum()) - areas[victim - 1] + 1
        out, bad = call_order(long_labels, long_raw, long_nid, long_rank, device, seg_base=moved)
        others = [i for i in range(1, long_nid) if i != victim]
        assert bad == BAD_AREA and (out[victim] == ABSENT).all() and np.array_equal(out[others], long_want[others]), victim
    # total has room for one long segment, two ids claim one each (both inside [0, total)): the list of long segments is full
    block_max = thresholds()[1]
    lab = np.concatenate([np.full(block_max + 500, 1), np.full(3000, 2), np.full(40, 3), np.zeros(block_max)]).astype(np.int32)
    v = values_for("i32", lab.shape, 12)
    area = np.array([0, block_max + 500, block_max + 500, 40])
    total = block_max + 500 + 3000 + 40
    assert total // block_max == 1
    base = np.array([0, 0, 0, block_max + 500 + 3000], np.uint64)                    # id 2 claims id 1's segment
    rk = np.zeros((4, 2), np.uint64)
    rk[:, 1] = [0, 700, 700, 39]
    out, bad = call_order(lab, v, 4, rk, device, area=area, seg_base=base, total=total)
    assert bad & BAD_AREA and not bad & (BAD_LABEL | BAD_VALUE | BAD_RANK)
    good, _ = ref_order_stats(lab, v, 4, rk)
    assert np.array_equal(out[3], good[3])


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    n = 4096
    lab = torch.zeros(n, dtype=torch.int32, device=device)
    raw = torch.zeros(n, dtype=torch.float64, device=device)
    ins = {k: torch.zeros(n, dtype=torch.int64, device=device) for k in ("area", "seg_base", "rank")}
    centre = torch.zeros(n, dtype=torch.float64, device=device)
    outs = {k: Out((n,), np.uint64, device) for k in ("out", "workspace", "bad")}
    null = ctypes.c_void_p(0)
    need = lib.clx_region_order_workspace(64, 4)

    def message():
        m = lib.clx_last_error()
        return m.decode() if isinstance(m, bytes) else str(m)

    def order(raw_type=F32, npix=64, nid=4, total=64, nq=2, nbytes=None, **ptrs):
        p = dict(labels=_clx.ptr(lab), raw=_clx.ptr(raw), area=_clx.ptr(ins["area"]), seg_base=_clx.ptr(ins["seg_base"]),
                 centre=null, rank=_clx.ptr(ins["rank"]), out=outs["out"].ptr, workspace=outs["workspace"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        nbytes = lib.clx_region_order_workspace(total, nid) if nbytes is None else nbytes
        return lib.clx_region_order_stats(p["labels"], p["raw"], raw_type, npix, nid, p["area"], p["seg_base"], total, p["centre"],
                                          p["rank"], nq, p["out"], p["workspace"], nbytes, p["bad"], st)

    odd = ctypes.c_void_p(outs["workspace"].ptr.value + 4)
    refused = [(lambda k=k: order(**{k: null}), "null") for k in ("labels", "raw", "area", "seg_base", "rank", "out", "workspace", "bad")] + [
        (lambda: order(raw_type=3), "raw_type"), (lambda: order(raw_type=-1), "raw_type"),
        (lambda: order(nid=0, nbytes=need), "nid"), (lambda: order(nid=-3, nbytes=need), "nid"), (lambda: order(nid=2 ** 24 + 1, nbytes=need), "nid"),
        (lambda: order(npix=0, total=0), "npix"), (lambda: order(npix=-1, total=0), "npix"), (lambda: order(npix=2 ** 32), "npix"),
        (lambda: order(nq=0), "nq"), (lambda: order(nq=33), "nq"), (lambda: order(nq=-2), "nq"),
        (lambda: order(total=-1, nbytes=need), "total"), (lambda: order(total=65, nbytes=8 * n), "total"),
        (lambda: order(nbytes=need - 1), "workspace_bytes"), (lambda: order(nbytes=0), "workspace_bytes"),
        (lambda: order(workspace=odd), "aligned"),
    ]
    for i, (call, word) in enumerate(refused):
        status = call()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message().startswith("clx_region_order_stats") and word in message(), f"case {i}: {message()!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    # accepted: a background-only map, with and without a centre; total == 0 launches the initialisation only
    assert order() == 0 and order(centre=_clx.ptr(centre)) == 0 and order(total=0) == 0 and order(nq=32, nid=2) == 0, message()
    assert order(raw_type=F64) == 0 and order(raw_type=I32, nq=1) == 0, message()
    torch.cuda.synchronize(device)
    assert int(outs["bad"].get()[:1].view(np.int32)[0]) == 0
    assert (outs["out"].get()[:4] == ABSENT).all()


def test_phases_alone_give_the_whole_call(device):
    """clx_region_order_phase, the timing tool's entry: phase 1 then phase 2 (twice: it can be repeated) leave what the whole
    call leaves; any other phase is refused"""
    from cellulus_amd import _clx

    labels, nid, _ = _threshold_map()
    raw = values_for("f32", labels.shape, 17)
    rank = spread_ranks(labels, nid)
    want, _ = call_order(labels, raw, nid, rank, device)
    lib = _clx.load()
    area = np.bincount(labels, minlength=nid).astype(np.int64)
    area[0] = 0
    total = int(area.sum())
    nbytes = lib.clx_region_order_workspace(total, nid)
    lab_d, raw_d, area_d, base_d, rank_d = (_dev(v, device) for v in (labels, raw, area, np.cumsum(area) - area, rank.view(np.int64)))
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    out = torch.full((nid, rank.shape[1]), 0x5C, dtype=torch.int64, device=device)
    bad = torch.full((1,), 0x5C, dtype=torch.int32, device=device)

    def phase(k):
        return lib.clx_region_order_phase(_clx.ptr(lab_d), _clx.ptr(raw_d), F32, labels.size, nid, _clx.ptr(area_d), _clx.ptr(base_d), total,
                                          ctypes.c_void_p(0), _clx.ptr(rank_d), rank.shape[1], _clx.ptr(out), _clx.ptr(work), nbytes,
                                          _clx.ptr(bad), k, _clx.stream_ptr(device))

    for k in (0, 3, -1):
        assert phase(k) == -1 and lib.clx_last_error().startswith(b"clx_region_order_phase: phase")
    assert lib.clx_region_order_phase(None, _clx.ptr(raw_d), F32, labels.size, nid, _clx.ptr(area_d), _clx.ptr(base_d), total, None,
                                      _clx.ptr(rank_d), rank.shape[1], _clx.ptr(out), _clx.ptr(work), nbytes, _clx.ptr(bad), 1,
                                      _clx.stream_ptr(device)) == -1
    assert lib.clx_last_error().startswith(b"clx_region_order_phase: null")      # a refusal names the entry that was called
    torch.cuda.synchronize(device)
    assert bool((out == 0x5C).all().item())
    assert phase(1) == 0 and phase(2) == 0 and phase(2) == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    assert int(bad.item()) == 0 and np.array_equal(out.cpu().numpy().view(np.uint64)[1:], want[1:])
