"""clx_inst_stats / clx_inst_histogram / clx_inst_refine (csrc/nucleus.hip), clx_peak_local_max (csrc/seeds.hip) and the
unaligned branch of clx_cc_label_filter through the C ABI against NumPy / SciPy (tests/nucleus_ref.py).  All of it is integer
or bit-exact work: every comparison is EQUALITY.  Outputs are prefilled (0xAB bytes unless a test says otherwise) and sit
between guard words that are checked after every call."""

import ctypes

import numpy as np
import pytest
import torch

from nucleus_ref import (BIG, DTYPES, F32, F64, GRID_CAP, I32, NBINS, THRESHOLD, big_label_map, blobs, cavity_3d, corner_link,
                         histogram_case, histogram_case_int, nested, raw_of, ref_histogram, ref_refine, ref_stats, serpentine,
                         special_values, thin_3d, thin_boxes, wide_box)
from test_gpu_measure import GUARD, Out, _dev

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
RAW_TYPES = [F32, F64, I32]
TYPE_IDS = {F32: "f32", F64: "f64", I32: "i32"}


def _lib():
    from cellulus_amd import _clx
    return _clx.load()


def _stream(device):
    from cellulus_amd import _clx
    return _clx.stream_ptr(device)


def _ptr(t):
    from cellulus_amd import _clx
    return _clx.ptr(t)


def _zyx(a):
    return (1,) * (3 - a.ndim) + tuple(a.shape)


def _set(out, host):
    """replace the 0xAB prefill of an Out by the bytes of `host` (the guard zones stay)"""
    host = np.ascontiguousarray(host, dtype=out.dtype)
    assert host.nbytes == out.nbytes
    out.buf[GUARD:GUARD + out.nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8).copy()).to(out.buf.device)


# ===================================================================================================== clx_inst_stats
def run_stats(seg, raw, nid, device, offset=0, outs=None):
    seg = np.asarray(seg, dtype=np.int32)
    Z, Y, X = _zyx(seg)
    lab, rw = _dev(seg, device, offset), _dev(raw, device, offset)
    if outs is None:
        outs = (Out((nid, 6), np.int32, device), Out((nid, 2), np.uint64, device))
    rt = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}[np.asarray(raw).dtype]
    status = _lib().clx_inst_stats(_ptr(lab), _ptr(rw), rt, Z, Y, X, nid, outs[0].ptr, outs[1].ptr, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return outs[0].get(), outs[1].get(), outs


def _stats_maps():
    """name -> (label map, nid): negative ids, ids >= nid, absent ids and a single-pixel id in every map that has room"""
    m = {}
    m["1x1"] = (np.ones((1, 1), np.int32), 3)                                   # id 1 = a single pixel, id 2 absent
    lab = blobs((5, 67), 6, 1)
    lab[0, 0], lab[4, 66], lab[2, 30], lab[3, 3] = -1, 9, -2 ** 31, 8           # 9 >= nid; 8 = a single pixel; 7 absent
    m["5x67"] = (lab, 9)
    lab = blobs((3, 1031), 5, 2)
    lab[1, 1030], lab[2, 0], lab[0, 515] = 7, -3, 2 ** 31 - 1                   # 7 = a single pixel (nid 9: 6 and 8 absent)
    m["3x1031"] = (lab, 9)
    lab = blobs((3, 40, 70), 12, 3)
    lab[2, 39, 69], lab[0, 0, 0], lab[1, 20, 35] = 14, -7, 16                   # 14 = a single pixel; 13, 15 absent; 16 >= nid
    m["3x40x70"] = (lab, 16)
    lab = big_label_map()
    lab[7, 7], lab[1029, 1000] = -5, 30                                         # 30 >= nid, on the second trip; 24 absent
    m["1030x1031"] = (lab, 25)
    return m


STATS_MAPS = _stats_maps()


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
@pytest.mark.parametrize("name", list(STATS_MAPS))
def test_inst_stats_equal_numpy(name, raw_type, device):
    seg, nid = STATS_MAPS[name]
    raw = special_values(seg, raw_type, 7)
    want_b, want_k = ref_stats(seg, raw, nid)
    got_b, got_k, outs = run_stats(seg, raw, nid, device)
    assert np.array_equal(got_b, want_b)
    assert np.array_equal(got_k, want_k)
    # absent ids (and row 0) hold the identity elements
    absent = np.union1d([0], np.setdiff1d(np.arange(nid), np.unique(seg)))
    assert len(absent) >= 2
    assert (got_b[absent, :3] == 0x7FFFFFFF).all() and (got_b[absent, 3:] == -1).all()
    assert (got_k[absent, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (got_k[absent, 1] == 0).all()
    # a second call on the stale outputs starts over
    again_b, again_k, _ = run_stats(seg, raw, nid, device, outs=outs)
    assert np.array_equal(again_b, want_b) and np.array_equal(again_k, want_k)
    # ... also when the stale rows belong to another image (the monotonic filters must not see them)
    other = np.where(seg > 0, seg, 0).astype(np.int32)[..., ::-1].copy()
    run_stats(other, raw, nid, device, outs=outs)
    last_b, last_k, _ = run_stats(seg, raw, nid, device, outs=outs)
    assert np.array_equal(last_b, want_b) and np.array_equal(last_k, want_k)


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
@pytest.mark.parametrize("offset", [1, 3])
def test_inst_stats_unaligned_inputs(offset, raw_type, device):
    for name in ("5x67", "3x40x70"):
        seg, nid = STATS_MAPS[name]
        raw = special_values(seg, raw_type, 8)
        want_b, want_k = ref_stats(seg, raw, nid)
        got_b, got_k, _ = run_stats(seg, raw, nid, device, offset=offset)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_k, want_k)


def test_inst_stats_float_edge_values(device):
    """one object each: all negative; -0.0 and +0.0 only (min is -0.0, max +0.0, whichever comes first); denormals only;
    -inf .. +inf; a single negative denormal"""
    for dtype in (np.float32, np.float64):
        tiny = np.nextafter(dtype(0), dtype(1))
        seg = np.repeat(np.arange(1, 7, dtype=np.int32), 8).reshape(6, 8)
        raw = np.empty((6, 8), dtype=dtype)
        raw[0] = [-1, -2.5, -1e-30, -3e30, -7, -tiny, -1, -2]
        raw[1] = [0.0, -0.0, 0.0, 0.0, -0.0, 0.0, 0.0, 0.0]
        raw[2] = [-0.0, -0.0, 0.0, -0.0, -0.0, -0.0, -0.0, -0.0]
        raw[3] = [tiny, -tiny, 3 * tiny, -2 * tiny, 0.0, tiny, tiny, tiny]
        raw[4] = [1, np.inf, -np.inf, 0, 5, -5, np.finfo(dtype).max, -np.finfo(dtype).max]
        raw[5] = -tiny
        want_b, want_k = ref_stats(seg, raw, 7)
        got_b, got_k, _ = run_stats(seg, raw, 7, device)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_k, want_k)
        from cellulus_amd.segment import _decode_keys
        vals = _decode_keys(got_k, F32 if dtype == np.float32 else F64)
        assert vals[1, 1] == -tiny and vals[1, 0] == dtype(-3e30)
        for row in (2, 3):
            assert np.signbit(vals[row, 0]) and vals[row, 0] == 0 and not np.signbit(vals[row, 1]) and vals[row, 1] == 0
        assert vals[4, 0] == -2 * tiny and vals[4, 1] == 3 * tiny
        assert vals[5, 0] == -np.inf and vals[5, 1] == np.inf
        assert vals[6, 0] == -tiny and vals[6, 1] == -tiny


# ================================================================================================= clx_inst_histogram
def run_histogram(seg, raw, slot, nid, aux, nbins, counts_in, device, offset=0):
    seg = np.asarray(seg, dtype=np.int32)
    rt = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}[np.asarray(raw).dtype]
    lab, rw = _dev(seg, device, offset), _dev(raw, device, offset)
    slot_d, aux_d = _dev(slot, device), _dev(aux, device)
    counts = Out(counts_in.shape, np.uint32, device)
    _set(counts, counts_in)
    status = _lib().clx_inst_histogram(_ptr(lab), _ptr(rw), rt, seg.size, _ptr(slot_d), nid, _ptr(aux_d), nbins, counts.ptr,
                                       _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return counts.get()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape,n_uniform,offset", [((150, 131), 2000, 0), ((150, 131), 2000, 1), ((150, 131), 2000, 3),
                                                    (BIG, 60000, 0)], ids=["150x131", "offset1", "offset3", "1030x1031"])
def test_inst_histogram_float_equals_numpy(shape, n_uniform, offset, dtype, device):
    seg, raw, slot, nid, edges = histogram_case(shape, dtype, n_uniform, 5)
    for e in edges:
        assert len(np.unique(e)) == NBINS + 1                                  # the condition under which numpy has an answer
    if shape == BIG:
        tail = seg.reshape(-1)[GRID_CAP:]
        assert all((tail == i).any() for i in range(1, 7))                      # every instance has pixels on the second trip
    rng = np.random.default_rng(1)
    counts_in = rng.integers(1, 1000, size=(6, NBINS)).astype(np.uint32)
    want = ref_histogram(seg, raw, slot, nid, edges, NBINS, counts_in)
    got = run_histogram(seg, raw, slot, nid, edges, NBINS, counts_in, device, offset)
    assert np.array_equal(got, want)
    assert int((want - counts_in).sum()) == int(np.isin(seg, np.arange(1, 7)).sum())


@pytest.mark.parametrize("shape,offset", [((40, 53), 0), ((40, 53), 1), ((40, 53), 3), (BIG, 0)],
                         ids=["40x53", "offset1", "offset3", "1030x1031"])
def test_inst_histogram_int_equals_numpy(shape, offset, device):
    seg, raw, slot, nid, vmin, nbins, widths = histogram_case_int(shape, 9)
    rng = np.random.default_rng(2)
    counts_in = rng.integers(1, 1000, size=(4, nbins)).astype(np.uint32)
    want = ref_histogram(seg, raw, slot, nid, vmin, nbins, counts_in)
    got = run_histogram(seg, raw, slot, nid, vmin, nbins, counts_in, device, offset)
    assert np.array_equal(got, want)
    for s in range(4):
        assert np.array_equal(got[s, widths[s]:], counts_in[s, widths[s]:])   # the tails of the narrower instances
        assert (got[s, :widths[s]] > counts_in[s, :widths[s]]).any()


# ==================================================================================================== clx_inst_refine
SLICE_GAP = 64


def run_refine(seg, raw, ndim, ids, thr, device, offset=0, prefill=-7, bbox=None, nid=None):
    """clx_inst_refine alone: bbox, thresholds and scratch offsets come from NumPy.  `out` starts as `prefill` everywhere;
    the scratch slices are SLICE_GAP bytes apart and the gaps must keep their 0xAB bytes.  -> out"""
    seg = np.asarray(seg, dtype=np.int32)
    raw = np.ascontiguousarray(raw)
    rt = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}[raw.dtype]
    Z, Y, X = _zyx(seg)
    assert ndim == 3 or Z == 1
    nid = nid or int(seg.max()) + 1
    if bbox is None:
        bbox, _ = ref_stats(seg, raw, nid)
    ids = np.asarray(ids, dtype=np.int32)
    n = len(ids)
    box = bbox[ids].astype(np.int64)
    vol = (box[:, 3] - box[:, 0] + 1) * (box[:, 4] - box[:, 1] + 1) * (box[:, 5] - box[:, 2] + 1)
    assert (vol > 0).all()
    off = SLICE_GAP + np.concatenate([[0], np.cumsum(vol + SLICE_GAP)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    total = int(SLICE_GAP + (vol + SLICE_GAP).sum())
    scratch = Out((total,), np.uint8, device)
    out = Out(seg.shape, np.int32, device)
    _set(out, np.full(seg.shape, prefill, np.int32))
    lab, rw = _dev(seg, device, offset), _dev(raw, device, offset)
    ids_d, bbox_d = _dev(ids if n else np.zeros(1, np.int32), device), _dev(bbox, device)
    thr_d = _dev(np.asarray(thr, dtype=np.float64) if n else np.zeros(1), device)
    off_d = _dev(off if n else np.zeros(1, np.int64), device)
    status = _lib().clx_inst_refine(_ptr(lab), _ptr(rw), rt, ndim, Z, Y, X, _ptr(ids_d), _ptr(bbox_d), _ptr(thr_d), _ptr(off_d),
                                    scratch.ptr, n, out.ptr, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    s = scratch.get()
    used = np.zeros(total, dtype=bool)
    for o, v in zip(off, vol):
        used[o:o + v] = True
    assert (s[~used] == 0xAB).all(), "a block wrote outside its scratch slice"
    assert (s[used] <= 2).all()                                                 # every state byte of every slice was set
    return out.get()


def check_refine(seg, bright, ndim, ids, raw_type, device, offset=0):
    raw = raw_of(bright, raw_type)
    thr = [THRESHOLD[raw_type]] * len(ids)
    want = ref_refine(seg, raw, ndim, ids, thr, np.full(seg.shape, -7, np.int32))
    got = run_refine(seg, raw, ndim, ids, thr, device, offset)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
@pytest.mark.parametrize("transpose", [False, True], ids=["rows", "columns"])
def test_refine_serpentine(transpose, raw_type, device):
    """the flood has to walk a ten-row corridor from its one opening; sealed, the whole corridor is a hole"""
    seg, bright, corridor = serpentine(True, transpose)
    got = check_refine(seg, bright, 2, [1], raw_type, device)
    assert (got == 1).all()
    seg, bright, corridor = serpentine(False, transpose)
    for offset in (0, 1, 3):
        got = check_refine(seg, bright, 2, [1], raw_type, device, offset)
        assert (got[corridor] == -7).all() and (got[bright] == 1).all()


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
def test_refine_wide_thin_and_corner_boxes(raw_type, device):
    seg, bright = wide_box()                                                    # > 256 x-lines and y-lines
    got = check_refine(seg, bright, 2, [1], raw_type, device)
    assert got[275, 270] == 1 and got[199, 279] == 1 and got[150, 295] == -7 and got[2, 20] == -7
    got = check_refine(seg.T.copy(), bright.T.copy(), 2, [1], raw_type, device)
    assert got[270, 275] == 1 and got[295, 150] == -7
    seg, bright = thin_boxes()                                                  # 1 x N and N x 1: nothing is filled
    got = check_refine(seg, bright, 2, [1, 2], raw_type, device)
    assert np.array_equal(got, np.where(bright & (seg > 0), seg, -7))
    seg, bright, hole = corner_link()                                           # face connectivity: the corner does not open it
    got = check_refine(seg, bright, 2, [1], raw_type, device)
    assert got[hole] == 1 and got[1, 1] == -7


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
def test_refine_3d(raw_type, device):
    seg, bright, cavity = cavity_3d(capped=False)                               # closed in every plane, open along z
    got = check_refine(seg, bright, 3, [1], raw_type, device)
    assert (got[cavity] == -7).all() and (got[bright] == 1).all()
    seg, bright, cavity = cavity_3d(capped=True)
    for offset in (0, 1, 3):
        got = check_refine(seg, bright, 3, [1], raw_type, device, offset)
        assert (got == 1).all()
    for Z in (1, 2):                                                            # every voxel on a z face: nothing is filled
        seg, bright = thin_3d(Z)
        got = check_refine(seg, bright, 3, [1], raw_type, device)
        assert np.array_equal(got == 1, bright) and (got[~bright] == -7).all()
    seg, bright = thin_3d(1)                                                    # the same slice as a 2-D call: z is no border
    got = check_refine(seg[0], bright[0], 2, [1], raw_type, device)
    assert (got == 1).all()


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
@pytest.mark.parametrize("ring,blob", [(2, 5), (5, 2)])
def test_refine_nested_is_per_pixel_maximum(ring, blob, raw_type, device):
    seg, bright = nested(ring, blob)
    for ids in ([2, 5, 7, 8], [8, 5, 7, 2]):                                    # the order of the list does not matter
        got = check_refine(seg, bright, 2, ids, raw_type, device)
        assert got[6, 6] == ring and got[9, 9] == max(ring, blob) and got[8, 8] == max(ring, blob)
    # a subset: the other instances stay unwritten
    got = check_refine(seg, bright, 2, [blob, 8], raw_type, device)
    assert got[6, 6] == -7 and (got[seg == 7] == -7).all() and got[9, 9] == blob
    assert set(np.unique(got).tolist()) == {-7, blob, 8}
    # a prefilled output is only ever raised: maximum(prefill, .)
    raw = raw_of(bright, raw_type)
    thr = [THRESHOLD[raw_type]] * 4
    for prefill in (3, 6, 100):
        want = ref_refine(seg, raw, 2, [2, 5, 7, 8], thr, np.full(seg.shape, prefill, np.int32))
        got = run_refine(seg, raw, 2, [2, 5, 7, 8], thr, device, prefill=prefill)
        assert np.array_equal(got, want)
        from_zero = ref_refine(seg, raw, 2, [2, 5, 7, 8], thr, np.zeros(seg.shape, np.int32))
        assert np.array_equal(got, np.where(from_zero > 0, np.maximum(from_zero, prefill), prefill))


@pytest.mark.parametrize("raw_type", RAW_TYPES, ids=TYPE_IDS.get)
def test_refine_random_maps(raw_type, device):
    """blobs that overwrite each other (nested, touching, split), noisy raw values, per-instance thresholds; 2-D and 3-D"""
    rng = np.random.default_rng(17)
    for shape, n, frac in (((67, 90), 14, 0.5), ((9, 30, 41), 10, 0.85)):
        seg = blobs(shape, n, 21 + len(shape))
        if len(shape) == 3:                                                     # boxes thick enough in z to enclose something
            seg[1:8, 2:20, 3:25], seg[3:9, 10:28, 15:40], seg[0:4, 22:30, 0:12], seg[4:7, 5:9, 6:12] = 11, 12, 13, 14
        if raw_type == I32:
            raw = rng.integers(-50, 150, size=shape).astype(np.int32)
        else:
            raw = (rng.random(shape) - 0.4).astype(DTYPES[raw_type])
        raw[rng.random(shape) < frac] = raw.max()                               # enough bright pixels to enclose holes
        ids = [int(i) for i in np.unique(seg) if i > 0]
        thr = [float(np.mean(raw[seg == i].astype(np.float64))) for i in ids]
        want = ref_refine(seg, raw, len(shape), ids, thr, np.full(shape, -7, np.int32))
        got = run_refine(seg, raw, len(shape), ids, thr, device)
        assert np.array_equal(got, want)
        unfilled = np.full(shape, -7, np.int32)
        for i, t in zip(ids, thr):
            unfilled[(seg == i) & (raw.astype(np.float64) > t)] = i
        assert (want != unfilled).any()                                         # some hole was filled


def test_refine_nothing_listed(device):
    seg, bright = nested(2, 5)
    raw = raw_of(bright, F32)
    got = run_refine(seg, raw, 2, [], [], device)
    assert (got == -7).all()
    # n == 0 returns before the per-instance pointers are looked at
    lab, rw = _dev(seg, device), _dev(raw, device)
    out = Out(seg.shape, np.int32, device)
    status = _lib().clx_inst_refine(_ptr(lab), _ptr(rw), F32, 2, 1, seg.shape[0], seg.shape[1], NULL, NULL, NULL, NULL, NULL, 0,
                                    out.ptr, _stream(device))
    torch.cuda.synchronize(device)
    assert status == 0 and out.untouched()


def test_refine_threshold_is_strict(device):
    """a pixel AT the threshold is not part of the mask; float32 values are compared as float64"""
    v = np.float32(0.1)
    up = np.nextafter(v, np.float32(1))
    seg = np.ones((7, 9), dtype=np.int32)
    raw = np.full((7, 9), v, dtype=np.float32)
    raw[2:5, 2:6] = up
    raw[3, 3] = v                                                               # enclosed by brighter pixels
    raw[0, 0] = np.float32(0.05)
    for thr, expect in ((float(v), raw > v), (0.1, raw > np.float64(0.1)), (float(up), np.zeros((7, 9), bool))):
        want = ref_refine(seg, raw, 2, [1], [thr], np.full(seg.shape, -7, np.int32))
        got = run_refine(seg, raw, 2, [1], [thr], device)
        assert np.array_equal(got, want)
        hole = expect.any()
        mask = expect.copy()
        if hole:
            mask[3, 3] = True
        assert np.array_equal(got == 1, mask)
    assert float(v) > 0.1                                                       # float32(0.1) lies above the double 0.1 ...
    # ... so with the double 0.1 as the threshold every 0.1f pixel is in, with float(v) none is
    raw64 = raw.astype(np.float64)
    got = run_refine(seg, raw64, 2, [1], [float(v)], device)
    assert np.array_equal(got, ref_refine(seg, raw64, 2, [1], [float(v)], np.full(seg.shape, -7, np.int32)))
    rawi = np.where(raw > v, 4, 3).astype(np.int32)
    for thr in (3.0, 3.5, 4.0, 2.999999):
        got = run_refine(seg, rawi, 2, [1], [thr], device)
        assert np.array_equal(got, ref_refine(seg, rawi, 2, [1], [thr], np.full(seg.shape, -7, np.int32)))


# ================================================================================================== rejected arguments
def _small(device):
    seg = np.zeros((6, 9), dtype=np.int32)
    seg[0:3, 0:4], seg[2:6, 5:9], seg[4:6, 0:3] = 1, 2, 3
    raw = np.arange(54, dtype=np.float32).reshape(6, 9)
    return seg, raw, _dev(seg, device), _dev(raw, device)


def test_inst_stats_rejects_bad_arguments(device):
    seg, raw, lab, rw = _small(device)
    lib, st = _lib(), _stream(device)
    bbox, vkey = Out((4, 6), np.int32, device), Out((4, 2), np.uint64, device)
    good = dict(seg=_ptr(lab), raw=_ptr(rw), rt=F32, Z=1, Y=6, X=9, nid=4, bbox=bbox.ptr, vkey=vkey.ptr)
    bad = [dict(seg=NULL), dict(raw=NULL), dict(bbox=NULL), dict(vkey=NULL), dict(rt=-1), dict(rt=3), dict(Z=0), dict(Y=0),
           dict(X=-1), dict(nid=0), dict(nid=-4)]
    for change in bad:
        a = dict(good, **change)
        status = lib.clx_inst_stats(a["seg"], a["raw"], a["rt"], a["Z"], a["Y"], a["X"], a["nid"], a["bbox"], a["vkey"], st)
        torch.cuda.synchronize(device)
        assert status != 0, change
        assert lib.clx_last_error().decode().startswith("clx_inst_stats"), change
        assert bbox.untouched() and vkey.untouched(), change
    a = good
    assert lib.clx_inst_stats(a["seg"], a["raw"], a["rt"], a["Z"], a["Y"], a["X"], a["nid"], a["bbox"], a["vkey"], st) == 0
    torch.cuda.synchronize(device)
    want = ref_stats(seg, raw, 4)
    assert np.array_equal(bbox.get(), want[0]) and np.array_equal(vkey.get(), want[1])


def test_inst_histogram_rejects_bad_arguments(device):
    seg, raw, lab, rw = _small(device)
    lib, st = _lib(), _stream(device)
    slot = np.array([-1, 0, 1, 2], dtype=np.int32)
    edges = np.stack([np.linspace(raw[seg == i].min(), raw[seg == i].max(), 9, dtype=np.float32) for i in (1, 2, 3)])
    slot_d, edges_d = _dev(slot, device), _dev(edges, device)
    counts = Out((3, 8), np.uint32, device)
    good = dict(seg=_ptr(lab), raw=_ptr(rw), rt=F32, npix=54, slot=_ptr(slot_d), nid=4, aux=_ptr(edges_d), nbins=8,
                counts=counts.ptr)
    bad = [dict(seg=NULL), dict(raw=NULL), dict(slot=NULL), dict(aux=NULL), dict(counts=NULL), dict(rt=-1), dict(rt=3),
           dict(npix=0), dict(npix=-54), dict(nid=0), dict(nid=-1), dict(nbins=0), dict(nbins=-8)]
    for change in bad:
        a = dict(good, **change)
        status = lib.clx_inst_histogram(a["seg"], a["raw"], a["rt"], a["npix"], a["slot"], a["nid"], a["aux"], a["nbins"],
                                        a["counts"], st)
        torch.cuda.synchronize(device)
        assert status != 0, change
        assert lib.clx_last_error().decode().startswith("clx_inst_histogram"), change
        assert counts.untouched(), change
    _set(counts, np.zeros((3, 8), np.uint32))
    a = good
    assert lib.clx_inst_histogram(a["seg"], a["raw"], a["rt"], a["npix"], a["slot"], a["nid"], a["aux"], a["nbins"], a["counts"],
                                  st) == 0
    torch.cuda.synchronize(device)
    assert np.array_equal(counts.get(), ref_histogram(seg, raw, slot, 4, edges, 8, np.zeros((3, 8), np.uint32)))


def test_inst_refine_rejects_bad_arguments(device):
    seg, raw, lab, rw = _small(device)
    lib, st = _lib(), _stream(device)
    bbox, _ = ref_stats(seg, raw, 4)
    ids = np.array([1, 2, 3], dtype=np.int32)
    vol = np.prod(bbox[ids, 3:].astype(np.int64) - bbox[ids, :3] + 1, axis=1)
    off = np.concatenate([[0], np.cumsum(vol)[:-1]]).astype(np.int64)
    ids_d, bbox_d, off_d = _dev(ids, device), _dev(bbox, device), _dev(off, device)
    thr_d = _dev(np.array([20.0, 20.0, 20.0]), device)
    scratch = Out((int(vol.sum()),), np.uint8, device)
    out = Out(seg.shape, np.int32, device)
    good = dict(seg=_ptr(lab), raw=_ptr(rw), rt=F32, ndim=2, Z=1, Y=6, X=9, ids=_ptr(ids_d), bbox=_ptr(bbox_d), thr=_ptr(thr_d),
                off=_ptr(off_d), scratch=scratch.ptr, n=3, out=out.ptr)
    bad = [dict(seg=NULL), dict(raw=NULL), dict(out=NULL), dict(ids=NULL), dict(bbox=NULL), dict(thr=NULL), dict(off=NULL),
           dict(scratch=NULL), dict(rt=-1), dict(rt=3), dict(Z=0), dict(Y=0), dict(X=0), dict(Y=-6), dict(n=-1),
           dict(ndim=2, Z=2, Y=3), dict(ndim=1), dict(ndim=4),
           dict(n=0, seg=NULL), dict(n=0, raw=NULL), dict(n=0, out=NULL)]      # the first check runs before the n == 0 return
    for change in bad:
        a = dict(good, **change)
        status = lib.clx_inst_refine(a["seg"], a["raw"], a["rt"], a["ndim"], a["Z"], a["Y"], a["X"], a["ids"], a["bbox"], a["thr"],
                                     a["off"], a["scratch"], a["n"], a["out"], st)
        torch.cuda.synchronize(device)
        assert status != 0, change
        assert lib.clx_last_error().decode().startswith("clx_inst_refine"), change
        assert out.untouched() and scratch.untouched(), change
    _set(out, np.zeros(seg.shape, np.int32))
    a = good
    assert lib.clx_inst_refine(a["seg"], a["raw"], a["rt"], a["ndim"], a["Z"], a["Y"], a["X"], a["ids"], a["bbox"], a["thr"], a["off"],
                               a["scratch"], a["n"], a["out"], st) == 0
    torch.cuda.synchronize(device)
    assert np.array_equal(out.get(), ref_refine(seg, raw, 2, ids, [20.0] * 3, np.zeros(seg.shape, np.int32)))


# ================================================================================================== clx_peak_local_max
def run_peaks(img, capacity, device):
    """-> (npeaks, the peaks buffer of `capacity` slots, 0xAB-prefilled)"""
    img = np.ascontiguousarray(img, dtype=np.float64)
    Z, Y, X = _zyx(img)
    img_d = _dev(img, device)
    mm = _dev(np.array([img.min(), img.max()]), device)
    peaks, count = Out((capacity,), np.int32, device), Out((1,), np.int32, device)
    status = _lib().clx_peak_local_max(_ptr(img_d), Z, Y, X, _ptr(mm), peaks.ptr, capacity, count.ptr, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return int(count.get()[0]), peaks.get()


def _lattice():
    img = np.zeros((80, 96))
    n = img[1::2, 1::2].size
    img[1::2, 1::2] = np.random.default_rng(0).permutation(n).reshape(40, 48) + 1.0
    return img


def test_peak_local_max_truncates_at_capacity_and_reports_the_full_count(device):
    from cellulus_amd.detect import peak_local_max

    img = _lattice()
    ref = np.sort(np.ravel_multi_index(peak_local_max(img).T, img.shape))
    assert len(ref) == 1833
    n, peaks = run_peaks(img, 1024, device)                                     # run_peaks checks the guard words after slot 1023
    assert n == 1833
    assert len(np.unique(peaks)) == 1024 and np.isin(peaks, ref).all()
    for capacity in (1833, 1834, 4000):
        n, peaks = run_peaks(img, capacity, device)
        assert n == 1833
        assert np.array_equal(np.sort(peaks[:n]), ref)
        assert (peaks[n:].view(np.uint32) == 0xABABABAB).all()                  # the slots past the count keep their prefill
    n, peaks = run_peaks(img, 1, device)
    assert n == 1833 and peaks[0] in ref


def test_peak_local_max_border_plateau_and_constant_maps(device):
    from cellulus_amd.detect import peak_local_max

    rng = np.random.default_rng(4)
    cases = {}
    b2 = np.zeros((9, 13))
    b2[0, :], b2[-1, :], b2[:, 0], b2[:, -1] = 3.0, 4.0, 5.0, 6.0
    b2[0, 5], b2[4, 12] = 9.0, 8.0
    cases["border_2d"] = b2
    b3 = np.zeros((5, 6, 7))
    b3[0], b3[-1] = 2.0, 3.0
    b3[:, 0], b3[:, -1], b3[:, :, 0], b3[:, :, -1] = 4.0, 5.0, 6.0, 7.0
    cases["border_3d"] = b3
    cases["z2"] = rng.random((2, 9, 11))                                        # every voxel on a z face
    cases["constant_2d"] = np.full((8, 9), 2.5)
    cases["constant_3d"] = np.full((4, 5, 6), -1.0)
    for name, img in cases.items():
        assert len(peak_local_max(img)) == 0, name
        n, peaks = run_peaks(img, 64, device)
        assert n == 0, name
        assert (peaks.view(np.uint32) == 0xABABABAB).all(), name
    # and maps with answers: random 2-D / 3-D, a plateau (every pixel of it is a peak), a peak beside the border
    more = {"random_2d": rng.random((33, 67)), "random_3d": rng.random((6, 17, 19)), "z3": rng.random((3, 9, 11))}
    plateau = np.zeros((12, 14))
    plateau[3:7, 4:9] = 1.0
    plateau[1, 1] = 0.5
    more["plateau"] = plateau
    for name, img in more.items():
        ref = np.sort(np.ravel_multi_index(peak_local_max(img).T, img.shape))
        assert len(ref) > 0, name
        n, peaks = run_peaks(img, 4096, device)
        assert n == len(ref) and np.array_equal(np.sort(peaks[:n]), ref), name


def test_peak_local_max_rejects_bad_arguments(device):
    img = _lattice()
    img_d = _dev(img, device)
    mm = _dev(np.array([0.0, img.max()]), device)
    lib, st = _lib(), _stream(device)
    peaks, count = Out((64,), np.int32, device), Out((1,), np.int32, device)
    good = dict(img=_ptr(img_d), Z=1, Y=80, X=96, mm=_ptr(mm), peaks=peaks.ptr, capacity=64, count=count.ptr)
    bad = [dict(img=NULL), dict(mm=NULL), dict(peaks=NULL), dict(count=NULL), dict(capacity=0), dict(capacity=-1), dict(Z=0),
           dict(Y=0), dict(X=-96), dict(Z=2 ** 15, Y=2 ** 8, X=2 ** 8)]
    for change in bad:
        a = dict(good, **change)
        status = lib.clx_peak_local_max(a["img"], a["Z"], a["Y"], a["X"], a["mm"], a["peaks"], a["capacity"], a["count"], st)
        torch.cuda.synchronize(device)
        assert status != 0, change
        assert peaks.untouched(), change
        c = count.get()[0]                                                      # (guard words checked)
        assert c == 0 or count.untouched(), change


# ================================================================================ clx_cc_label_filter, unaligned `out`
def _snake():
    seg = np.zeros((64, 65), dtype=np.int32)
    seg[::2, :] = 7
    for r in range(1, 63, 2):
        seg[r, 64 if (r // 2) % 2 == 0 else 0] = 7
    return seg


def _cc_maps():
    maps = {}
    for shape in ((37, 61), (200, 260)):
        rng = np.random.default_rng(sum(shape))
        maps["x".join(map(str, shape))] = (rng.random(shape) < 0.55).astype(np.int32) * rng.integers(1, 4, size=shape).astype(np.int32)
    maps["snake_64x65"] = _snake()
    return maps


CC_MAPS = _cc_maps()


def run_cc(seg, min_size, lead, device):
    """clx_cc_label_filter with `out` starting `lead` bytes past a 16-byte boundary, between guard words"""
    lib = _lib()
    Y, X = seg.shape
    nbytes = seg.size * 4
    buf = torch.full((GUARD + lead + nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    out_ptr = buf.data_ptr() + GUARD + lead
    assert out_ptr % 16 == lead
    ws = torch.empty(int(lib.clx_cc_workspace(seg.size)), dtype=torch.uint8, device=device)
    lab = _dev(seg, device)
    ncomp = Out((1,), np.int32, device)
    status = lib.clx_cc_label_filter(_ptr(lab), ctypes.c_void_p(out_ptr), 1, Y, X, min_size, ncomp.ptr, _ptr(ws), _stream(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    host = buf.cpu().numpy()
    assert (host[:GUARD + lead] == 0xAB).all() and (host[GUARD + lead + nbytes:] == 0xAB).all(), "guard words overwritten"
    return host[GUARD + lead:GUARD + lead + nbytes].copy().view(np.int32).reshape(seg.shape), int(ncomp.get()[0])


@pytest.mark.parametrize("min_size", [1, 9])
@pytest.mark.parametrize("name", list(CC_MAPS))
def test_cc_label_filter_unaligned_out_takes_the_pixel_list_path(name, min_size, device):
    """`out` 4 bytes past a 16-byte boundary: the label-list path (16-byte accesses to `out`) is not taken; labels and the
    component count equal the aligned call's and the oracle's"""
    from oracle import infer_oracle as IO

    seg = CC_MAPS[name]
    want = IO.size_filter(seg.copy(), min_size)
    aligned, n_aligned = run_cc(seg, min_size, 0, device)
    assert np.array_equal(aligned, want) and n_aligned == want.max()
    for lead in (4, 8, 12):
        got, n = run_cc(seg, min_size, lead, device)
        assert np.array_equal(got, want), lead
        assert n == n_aligned, lead
