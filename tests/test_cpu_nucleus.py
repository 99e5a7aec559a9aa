"""CPU tier of the nucleus-refinement and seed tests (no kernel is launched): the key encoding against
segment._decode_keys, the NumPy restatement of clx_inst_refine against the oracle's nucleus_refine, the properties the
flood, histogram and peak fixtures of the GPU tier claim, and the C-ABI symbols."""

import ctypes
import os
import re

import numpy as np
import pytest

from nucleus_ref import (BIG, F32, F64, GRID_CAP, HIST_RANGES, I32, NBINS, THRESHOLD, big_label_map, cavity_3d, corner_link,
                         edge_values, encode_keys, histogram_case, histogram_case_int, nested, raw_of, ref_histogram, ref_refine,
                         ref_stats, serpentine, special_values, thin_3d, thin_boxes, wide_box)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- keys
def _edge_floats(dtype):
    fi = np.finfo(dtype)
    tiny = np.nextafter(dtype(0), dtype(1))
    v = [0.0, -0.0, tiny, -tiny, 2 * tiny, -2 * tiny, fi.tiny, -fi.tiny, np.nextafter(fi.tiny, dtype(0)), 1.0, -1.0,
         np.nextafter(dtype(1), dtype(2)), fi.max, -fi.max, np.inf, -np.inf]
    return np.array(v, dtype=dtype)


@pytest.mark.parametrize("raw_type", [F32, F64, I32])
def test_key_round_trip_and_order(raw_type):
    from cellulus_amd.segment import _decode_keys

    rng = np.random.default_rng(raw_type)
    if raw_type == I32:
        edge = np.array([0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 2, -2 ** 31 + 1], dtype=np.int32)
        rand = rng.integers(-2 ** 31, 2 ** 31, size=4000).astype(np.int32)
        bits = np.uint32
    else:
        dtype = np.float32 if raw_type == F32 else np.float64
        bits = np.uint32 if raw_type == F32 else np.uint64
        edge = _edge_floats(dtype)
        assert np.signbit(edge[1]) and edge[2] > 0 and edge[2] / dtype(2) == 0       # -0.0 and the smallest denormal are real
        rand = np.concatenate([rng.normal(size=2000), rng.normal(size=2000) * 1e-40, rng.normal(size=500) * 1e30]).astype(dtype)
    for v in (edge, rand):
        keys = encode_keys(v)
        assert keys.dtype == np.uint64
        if raw_type != F64:
            assert (keys >> np.uint64(32)).max() == 0
        back = _decode_keys(keys, raw_type)
        assert back.dtype == v.dtype
        assert np.array_equal(back.view(bits), v.view(bits))                        # bit for bit: -0.0 stays -0.0
    # key order = value order, with -0.0 strictly below +0.0 and the infinities at the ends
    allv = np.concatenate([edge, rand])
    keys = encode_keys(allv)
    order = np.argsort(keys, kind="stable")
    sv = allv[order]
    assert np.array_equal(sv, np.sort(allv, kind="stable"))                          # as numbers (-0.0 == 0.0 there) ...
    assert len(np.unique(keys)) == len(np.unique(allv.view(bits)))                   # ... and injective on bit patterns
    if raw_type != I32:
        neg0, pos0 = encode_keys(np.array([-0.0, 0.0], dtype=allv.dtype))
        assert neg0 + np.uint64(1) == pos0                                           # ... and adjacent, in this order, as keys
        assert keys.min() == encode_keys(np.array([-np.inf], dtype=allv.dtype))[0]
        assert keys.max() == encode_keys(np.array([np.inf], dtype=allv.dtype))[0]


def test_absent_rows_hold_the_identity_elements():
    """the rows clx_inst_stats leaves for absent ids: (INT_MAX x3, -1 x3) and (~0, 0)"""
    bbox, vkey = ref_stats(np.zeros((3, 4), np.int32), np.zeros((3, 4), np.float32), 5)
    assert (bbox[:, :3] == 0x7FFFFFFF).all() and (bbox[:, 3:] == -1).all()
    assert (vkey[:, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (vkey[:, 1] == 0).all()


# ------------------------------------------------------------------------------------------------- ref_refine vs oracle
def _random_map(shape, dtype, rng):
    blocks = rng.integers(0, 6, size=tuple(-(-s // 6) for s in shape))
    seg = np.kron(blocks, np.ones((6,) * len(shape), dtype=np.int64))[tuple(slice(0, s) for s in shape)]
    seg[rng.random(shape) < 0.05] = 0
    seg = seg.astype(np.int32)
    raw = rng.random(shape)
    raw[rng.random(shape) < 0.3] *= 0.2
    raw[seg == 3] = 0.5                                                              # a constant instance
    if np.issubdtype(dtype, np.integer):
        return seg, (raw * 200).astype(dtype) - 50
    return seg, (raw - 0.4).astype(dtype)                                            # negative values too


@pytest.mark.parametrize("shape", [(30, 41), (25, 25), (7, 20, 19), (2, 18, 18)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_ref_refine_equals_oracle(shape, dtype):
    from oracle import infer_oracle as IO

    rng = np.random.default_rng(sum(shape) + np.dtype(dtype).itemsize)
    seg, raw = _random_map(shape, dtype, rng)
    ids = [int(i) for i in np.unique(seg) if i != 0]
    thr = [float(IO.threshold_otsu(raw[seg == i])) for i in ids]
    got = ref_refine(seg, raw, seg.ndim, ids, thr, np.zeros(seg.shape, np.int32))
    want = IO.nucleus_refine(seg, raw)
    assert np.array_equal(got, want)
    assert len(ids) >= 3 and (want != seg).any() and ((want != 0) & (want == seg)).any()
    # the listing order of ids does not matter, and a prefilled output is only ever raised
    rev = ref_refine(seg, raw, seg.ndim, ids[::-1], thr[::-1], np.zeros(seg.shape, np.int32))
    assert np.array_equal(rev, want)
    pre = ref_refine(seg, raw, seg.ndim, ids, thr, np.full(seg.shape, 3, np.int32))
    assert np.array_equal(pre, np.maximum(want, 3))


# ------------------------------------------------------------------------------------------------------- flood fixtures
@pytest.mark.parametrize("transpose", [False, True])
def test_serpentine_fixture(transpose):
    from scipy.ndimage import binary_fill_holes, label

    for closed in (True, False):
        seg, bright, corridor = serpentine(closed, transpose)
        assert seg.shape == ((40, 41) if transpose else (41, 40)) and (seg == 1).all()
        assert np.array_equal(corridor, ~bright)
        _, ncomp = label(corridor)                                                  # face connectivity
        assert ncomp == 1
        lines = corridor.sum(axis=0 if transpose else 1)
        assert (lines >= 38).sum() == 10                                            # ten corridor rows
        edge = np.ones_like(corridor)
        edge[1:-1, 1:-1] = False
        filled = binary_fill_holes(bright)
        if closed:
            assert not (corridor & edge).any()
            assert filled.all()
        else:
            assert (corridor & edge).sum() == 1
            assert np.array_equal(filled, bright)
            # the opening is on the last corridor row (38): a flood from it reaches row 2 only through all ten rows
            start = np.argwhere(corridor & edge)[0]
            assert (start[1] if transpose else start[0]) == 38
        for rt in (F32, F64, I32):
            out = ref_refine(seg, raw_of(bright, rt), 2, [1], [THRESHOLD[rt]], np.zeros(seg.shape, np.int32))
            assert np.array_equal(out != 0, filled)


def test_wide_thin_and_corner_fixtures():
    from scipy.ndimage import binary_fill_holes

    seg, bright = wide_box()
    filled = binary_fill_holes(bright)
    assert seg.shape == (300, 300) and min(seg.shape) > 256
    assert filled[5, 7] and filled[270:281, 262:290].all() and filled[100:200, 130].all() and filled[199, 130:280].all()
    assert not filled[150, 290:300].any() and not filled[0:4, 20].any()
    seg, bright = thin_boxes()
    out = ref_refine(seg, raw_of(bright, F32), 2, [1, 2], [0.5, 0.5], np.zeros(seg.shape, np.int32))
    assert np.array_equal(out, np.where(bright, seg, 0)) and (out != seg).sum() == 6
    seg, bright, hole = corner_link()
    out = ref_refine(seg, raw_of(bright, F32), 2, [1], [0.5], np.zeros(seg.shape, np.int32))
    assert out[hole] == 1 and out[1, 1] == 0 and not bright[hole]
    # with full (corner) connectivity the hole would be open
    assert not binary_fill_holes(bright[1:8, 1:8], structure=np.ones((3, 3)))[1, 1]


def test_3d_fixtures():
    for capped in (False, True):
        seg, bright, cavity = cavity_3d(capped)
        out = ref_refine(seg, raw_of(bright, F64), 3, [1], [0.5], np.zeros(seg.shape, np.int32))
        assert (out[bright] == 1).all()
        assert (out[cavity] == (1 if capped else 0)).all()
        # sealed in every plane: slice by slice the column is a hole even where it is open along z
        for z in range(seg.shape[0]):
            out2 = ref_refine(seg[z], raw_of(bright[z], F64), 2, [1], [0.5], np.zeros(seg.shape[1:], np.int32))
            assert (out2 == 1).all()
    for Z in (1, 2):
        seg, bright = thin_3d(Z)
        out = ref_refine(seg, raw_of(bright, I32), 3, [1], [0.0], np.zeros(seg.shape, np.int32))
        assert np.array_equal(out != 0, bright) and not bright.all()
        out2 = ref_refine(seg[0], raw_of(bright[0], I32), 2, [1], [0.0], np.zeros(seg.shape[1:], np.int32))
        assert (out2 == 1).all()


def test_nested_fixture_is_the_per_pixel_maximum():
    from oracle import infer_oracle as IO

    for ring, blob in ((2, 5), (5, 2)):
        seg, bright = nested(ring, blob)
        raw = raw_of(bright, F32)
        ids = [2, 5, 7, 8]
        out = ref_refine(seg, raw, 2, ids, [0.5] * 4, np.zeros(seg.shape, np.int32))
        assert np.array_equal(out, IO.nucleus_refine(seg, raw))                     # Otsu separates the two values as well
        assert out[8, 8] == max(ring, blob) and not bright[8, 8]                    # the blob's own hole: filled by both
        assert out[6, 6] == ring and seg[6, 6] == 0                                 # the ring's hole is filled with the ring
        assert out[9, 9] == max(ring, blob)                                         # over the blob: the later (larger) id
        assert out[3, 6] == ring and not bright[3, 6]
        singles = [ref_refine(seg, raw, 2, [i], [0.5], np.zeros(seg.shape, np.int32)) for i in ids]
        assert np.array_equal(out, np.maximum.reduce(singles))


# ----------------------------------------------------------------------------------------------- stats / histogram data
def test_big_map_puts_extremes_on_the_second_trip():
    lab = big_label_map()
    npix = lab.size
    assert lab.shape == BIG and npix == 1061930 and npix - GRID_CAP == 13354
    assert 20 <= len(np.unique(lab[lab > 0])) <= 24
    flat = lab.reshape(-1)
    for rt in (F32, F64, I32):
        raw = special_values(lab, rt, 1)
        full_b, full_k = ref_stats(lab, raw, 24)
        head = flat.copy()
        head[GRID_CAP:] = 0                                                          # what the first trip alone sees
        head_b, head_k = ref_stats(head.reshape(BIG), raw, 24)
        assert (full_b[21] != head_b[21]).any() and (full_b[23] != head_b[23]).any()
        assert head_b[22, 3] == -1 and full_b[22].tolist() == [0, 1029, 1030, 0, 1029, 1030]
        assert (full_k[21] != head_k[21]).all() and full_k[23, 1] != head_k[23, 1]   # id 21: min and max; id 23: max


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_histogram_fixture_has_distinct_edges_and_hits_them(dtype):
    rng = np.random.default_rng(0)
    for lo, hi in HIST_RANGES:
        values, edges = edge_values(lo, hi, dtype, 2000, rng)
        assert values.dtype == dtype and edges.dtype == dtype
        assert len(np.unique(edges)) == NBINS + 1, (lo, hi)                          # or np.histogram raises
        assert values.min() == edges[0] and values.max() == edges[-1]
        assert np.isin(edges, values).all()
        counts, e = np.histogram(values, bins=NBINS)
        assert np.array_equal(e, edges) and counts.sum() == len(values)
        # a value on an inner edge belongs to the bin on its right, one ulp below it to the bin on its left
        k = 100
        assert np.histogram(edges[k:k + 1], bins=edges)[0][k] == 1
        assert np.histogram(np.nextafter(edges[k:k + 1], dtype(-np.inf)), bins=edges)[0][k - 1] == 1
    seg, raw, slot, nid, edges = histogram_case((150, 131), dtype, 2000, 3)
    zero = np.zeros((6, NBINS), np.uint32)
    counts = ref_histogram(seg, raw, slot, nid, edges, NBINS, zero)
    assert counts.sum() == sum(int((seg == i).sum()) for i in range(1, 7))
    assert (seg == 7).any() and (seg == 9).any() and (seg == -4).any() and slot[7] == -1
    pre = ref_histogram(seg, raw, slot, nid, edges, NBINS, zero + np.uint32(5))
    assert np.array_equal(pre, counts + np.uint32(5))


def test_int_histogram_fixture():
    seg, raw, slot, nid, vmin, nbins, widths = histogram_case_int((40, 53), 2)
    assert nbins == widths.max() and len(set(widths.tolist())) == 4
    counts = ref_histogram(seg, raw, slot, nid, vmin, nbins, np.zeros((4, nbins), np.uint32))
    for s in range(4):
        assert (counts[s, widths[s]:] == 0).all() and counts[s, :widths[s]].sum() > 0
    inside = sum(int((seg == i).sum()) for i in range(1, 5))
    assert 0 < inside - int(counts.sum()) <= 12                                     # the out-of-window values are dropped


def test_seed_rerun_fixture_exceeds_the_first_capacity():
    """the plateau the seeds_on_device rerun test relies on"""
    from scipy.ndimage import gaussian_filter

    from cellulus_amd.detect import peak_local_max

    mag = np.full((100, 100), 5.0)
    mag[18:82, 18:82] = 1.0
    smooth = gaussian_filter(mag, sigma=2)
    assert int((smooth == smooth.min()).sum()) == 2304
    peaks = peak_local_max(-smooth)
    assert len(peaks) == 2304 > max(1024, mag.size // 9 + 16) == 1127


def test_peak_lattice_fixture():
    from cellulus_amd.detect import peak_local_max

    img = np.zeros((80, 96))
    rng = np.random.default_rng(0)
    n = img[1::2, 1::2].size
    img[1::2, 1::2] = rng.permutation(n).reshape(40, 48) + 1.0
    assert len(peak_local_max(img)) == 1833 > 1024


# -------------------------------------------------------------------------------------------------------------- symbols
def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    nargs = {"clx_inst_stats": 10, "clx_inst_histogram": 10, "clx_inst_refine": 15, "clx_peak_local_max": 9,
             "clx_cc_label_filter": 9}
    for name, n in nargs.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, f"{name} is not declared in include/clx.h"
        assert len(m.group(1).split(",")) == n, f"{name}: include/clx.h declares {m.group(1)!r}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_clx.PROTOTYPES[name][1]) == n and _clx.PROTOTYPES[name][0] is ctypes.c_int
    # the wide arguments are declared wide: npix of clx_inst_histogram
    assert _clx.PROTOTYPES["clx_inst_histogram"][1][3] is ctypes.c_longlong
