"""NumPy / SciPy restatement of the instance post-processing entry points of csrc/nucleus.hip (clx_inst_stats,
clx_inst_histogram, clx_inst_refine) and the label maps their tests share.  No device, no libclx: np.minimum.at /
np.maximum.at on the order-preserving keys, np.histogram / np.bincount per instance, scipy.ndimage.binary_fill_holes per
instance.  Everything here is integer or bit-exact work."""

import numpy as np

F32, F64, I32 = 0, 1, 2         # clx_raw_type
INT_MAX = 0x7FFFFFFF
KEY_ABSENT_MIN = np.uint64(0xFFFFFFFFFFFFFFFF)
DTYPES = {F32: np.float32, F64: np.float64, I32: np.int32}


def raw_type_of(raw):
    return {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}[np.asarray(raw).dtype]


def encode_keys(values):
    """uint64 keys of a float32 / float64 / int32 array: key(a) < key(b) as unsigned integers  <=>  a sorts below b, with
    -0.0 below +0.0.  Negative floats: all bits flipped; other floats: sign bit set; integers: sign bit flipped.  float32 and
    int32 keys lie in the low 32 bits.  This is the inverse of cellulus_amd.segment._decode_keys."""
    v = np.ascontiguousarray(values)
    if v.dtype == np.int32:
        return (v.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    if v.dtype == np.float32:
        b = v.view(np.uint32)
        return np.where(b >> np.uint32(31) == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint32).astype(np.uint64)
    assert v.dtype == np.float64, v.dtype
    b = v.view(np.uint64)
    return np.where(b >> np.uint64(63) == 1, ~b, b | np.uint64(1 << 63)).astype(np.uint64)


def _zyx(a):
    a = np.asarray(a)
    assert a.ndim in (2, 3), a.shape
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def ref_stats(seg, raw, nid):
    """clx_inst_stats: bbox (nid, 6) int32 = (zmin, ymin, xmin, zmax, ymax, xmax), vkey (nid, 2) uint64 = keys of the smallest
    and the largest raw value, for every id in (0, nid); absent ids (and row 0) keep (INT_MAX x3, -1 x3) and (~0, 0)"""
    seg3 = _zyx(seg).astype(np.int64)
    lab = seg3.reshape(-1)
    keys = encode_keys(np.ascontiguousarray(raw).reshape(-1))
    ok = (lab > 0) & (lab < nid)
    ids = lab[ok]
    bbox = np.empty((nid, 6), dtype=np.int32)
    bbox[:, :3] = INT_MAX
    bbox[:, 3:] = -1
    coords = np.indices(seg3.shape).reshape(3, -1)[:, ok].astype(np.int32)
    for k in range(3):
        np.minimum.at(bbox[:, k], ids, coords[k])
        np.maximum.at(bbox[:, 3 + k], ids, coords[k])
    vkey = np.empty((nid, 2), dtype=np.uint64)
    vkey[:, 0] = KEY_ABSENT_MIN
    vkey[:, 1] = 0
    np.minimum.at(vkey[:, 0], ids, keys[ok])
    np.maximum.at(vkey[:, 1], ids, keys[ok])
    return bbox, vkey


def ref_histogram(seg, raw, slot, nid, edges_or_min, nbins, counts_in):
    """clx_inst_histogram: counts_in (n, nbins) uint32 plus, for every id in (0, nid) with slot[id] >= 0, the histogram of
    its raw values in row slot[id].  Floats: np.histogram(values, bins=nbins) in the raw dtype, whose edges must be the row
    of `edges_or_min` (n, nbins + 1) -- the entry point is handed numpy's own edges.  int32: one bin per value from
    edges_or_min[slot], values outside [vmin, vmin + nbins) dropped."""
    lab = np.asarray(seg).reshape(-1).astype(np.int64)
    raw = np.ascontiguousarray(raw).reshape(-1)
    slot = np.asarray(slot)
    counts = np.array(counts_in, dtype=np.uint32, copy=True)
    for id_ in range(1, nid):
        s = int(slot[id_])
        if s < 0:
            continue
        values = raw[lab == id_]
        if values.size == 0:
            continue
        if raw.dtype == np.int32:
            idx = values.astype(np.int64) - int(edges_or_min[s])
            idx = idx[(idx >= 0) & (idx < nbins)]
            counts[s] += np.bincount(idx, minlength=nbins).astype(np.uint32)
        else:
            c, e = np.histogram(values, bins=nbins)
            assert e.dtype == raw.dtype and np.array_equal(e, edges_or_min[s]), f"instance {id_}: not numpy's edges"
            counts[s] += c.astype(np.uint32)
    return counts


def ref_refine(seg, raw, ndim, ids, thr, out_in):
    """clx_inst_refine: for each listed id in ascending order, mask = (seg == id) & (float64(raw) > thr), holes filled
    inside the id's bounding box (of all its pixels) with scipy's default (face-connected) structure, out = max(out, id)
    on the mask.  ndim 2 takes a (Y, X) map; ndim 3 a (Z, Y, X) map, whose z faces are border like the others."""
    from scipy.ndimage import binary_fill_holes

    seg = np.asarray(seg)
    raw = np.asarray(raw)
    assert seg.ndim == ndim and raw.shape == seg.shape
    out = np.array(out_in, dtype=np.int32, copy=True).reshape(seg.shape)
    order = np.argsort(np.asarray(ids), kind="stable")
    for k in order:
        id_ = int(ids[k])
        m = seg == id_
        assert m.any(), f"id {id_} is listed but absent"
        box = tuple(slice(int(w.min()), int(w.max()) + 1) for w in np.where(m))
        mask = m & (raw.astype(np.float64) > float(thr[k]))
        mask[box] = binary_fill_holes(mask[box])
        out[mask] = np.maximum(out[mask], id_)
    return out


# ---------------------------------------------------------------------------------------------------------- raw values
BRIGHT = {F32: np.float32(0.75), F64: np.float64(0.75), I32: np.int32(7)}
DARK = {F32: np.float32(0.25), F64: np.float64(0.25), I32: np.int32(-2)}
THRESHOLD = {F32: 0.5, F64: 0.5, I32: 0.0}


def raw_of(bright, raw_type):
    """two-valued raw image of a boolean map: BRIGHT where it is set, DARK elsewhere; THRESHOLD separates the two"""
    return np.where(np.asarray(bright, dtype=bool), BRIGHT[raw_type], DARK[raw_type]).astype(DTYPES[raw_type])


# ------------------------------------------------------------------------------------------------------ flood fixtures
def serpentine(closed, transpose=False):
    """(seg, bright, corridor) on (41, 40): one instance (id 1) over the whole map; a one-pixel dark corridor runs along
    rows 2, 6, ..., 38 between columns 1 and 38 and turns at alternate ends, so it is ONE face-connected background
    component of 10 rows.  closed: it touches the border nowhere.  open: its far end (row 38) is extended to the border
    column, so a flood from the border has to walk the whole corridor back to row 2."""
    seg = np.ones((41, 40), dtype=np.int32)
    corridor = np.zeros((41, 40), dtype=bool)
    rows = list(range(2, 39, 4))
    for n, y in enumerate(rows):
        corridor[y, 1:39] = True
        if y != rows[-1]:
            corridor[y:y + 4, 38 if n % 2 == 0 else 1] = True
    if not closed:
        # row 38 is the tenth row (n = 9): it was entered at column 38, so its far end is column 1 -> open towards column 0
        corridor[rows[-1], 0] = True
    bright = ~corridor
    if transpose:
        seg, bright, corridor = seg.T.copy(), bright.T.copy(), corridor.T.copy()
    return seg, bright, corridor


def wide_box():
    """(seg, bright) on (300, 300): one instance over the whole map (more than 256 x-lines and y-lines) with an interior
    one-pixel hole, a block hole beyond line 256 in both axes, an L-shaped hole, and a dark notch that reaches the border"""
    seg = np.ones((300, 300), dtype=np.int32)
    bright = np.ones((300, 300), dtype=bool)
    bright[5, 7] = False
    bright[270:281, 262:290] = False
    bright[100:200, 130] = False
    bright[199, 130:280] = False
    bright[150, 290:300] = False                    # open: reaches column 299
    bright[0:4, 20] = False                         # open: reaches row 0
    return seg, bright


def thin_boxes():
    """(seg, bright) on (12, 30): id 1 is a 1 x 19 line, id 2 a 9 x 1 line, both with dark pixels inside.  Every pixel of
    a one-pixel-thick box is a border pixel, so nothing is filled."""
    seg = np.zeros((12, 30), dtype=np.int32)
    seg[3, 2:21] = 1
    seg[2:11, 25] = 2
    bright = np.ones((12, 30), dtype=bool)
    bright[3, 5:8] = False
    bright[3, 12] = False
    bright[5:7, 25] = False
    return seg, bright


def corner_link():
    """(seg, bright, hole) on (9, 9): id 1 on [1:8, 1:8]; the dark pixel `hole` = (2, 2) touches the dark border pixel (1, 1)
    only through a corner: under face connectivity it is enclosed, and filled"""
    seg = np.zeros((9, 9), dtype=np.int32)
    seg[1:8, 1:8] = 1
    bright = np.ones((9, 9), dtype=bool)
    bright[1, 1] = False
    bright[2, 2] = False
    return seg, bright, (2, 2)


def cavity_3d(capped):
    """(seg, bright, cavity) on (5, 7, 8): id 1 over the whole volume with a dark column at (y, x) = (3, 4), sealed in y and
    x.  capped: the column spans z = 1..3 only and is enclosed.  Not capped: it runs through z = 0 and z = 4, the z faces of
    the box, and is open."""
    seg = np.ones((5, 7, 8), dtype=np.int32)
    cavity = np.zeros((5, 7, 8), dtype=bool)
    cavity[(slice(1, 4) if capped else slice(None)), 3, 4] = True
    return seg, ~cavity, cavity


def thin_3d(Z):
    """(seg, bright) on (Z, 9, 10), Z = 1 or 2: one instance with interior dark pixels in every slice.  As a 3-D input every
    voxel lies on a z face; the same (Y, X) slice as a 2-D input has its holes filled."""
    seg = np.ones((Z, 9, 10), dtype=np.int32)
    bright = np.ones((Z, 9, 10), dtype=bool)
    bright[:, 3:5, 4:7] = False
    bright[:, 7, 2] = False
    return seg, bright


def nested(ring_id, blob_id):
    """(seg, bright) on (24, 26): a square ring `ring_id` with a dark notch, a blob `blob_id` inside its hole (with a dark
    hole of its own), and two L-shaped instances 7 and 8 whose bounding boxes overlap each other and the ring's"""
    seg = np.zeros((24, 26), dtype=np.int32)
    seg[2:16, 2:16] = ring_id
    seg[5:13, 5:13] = 0
    seg[7:11, 7:11] = blob_id
    bright = np.ones((24, 26), dtype=bool)
    bright[8, 8] = False                            # the blob's own hole
    bright[3, 4:9] = False                          # a dark stripe inside the ring's rim: enclosed by the rim
    # two interlocking L shapes
    seg[10:22, 18:20] = 7
    seg[20:22, 12:20] = 7
    seg[12:14, 14:25] = 8
    seg[12:23, 23:25] = 8
    seg[12:14, 18:20] = 8                           # where they cross, 8 owns the pixels
    bright[15, 18] = False
    bright[13, 21] = False
    return seg, bright


# ------------------------------------------------------------------------------------------------------ stats fixtures
def blobs(shape, n, seed):
    """seeded label map of n box-shaped objects separated by background"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.int32)
    for i in range(1, n + 1):
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [min(s, a + int(rng.integers(1, max(2, s // 3)))) for s, a in zip(shape, lo)]
        lab[tuple(slice(a, b) for a, b in zip(lo, hi))] = i
    return lab


GRID_CAP = 4096 * 256           # threads of the capped grid of stats_kernel / inst_hist*_kernel: one trip covers this many pixels
BIG = (1030, 1031)              # 1 061 930 pixels: the last 13 354 are reached on the second trip only


def big_label_map():
    """(1030, 1031) map of about 20 labels; labels 21-23 have their extreme pixels in the last 13 354 pixels only"""
    lab = blobs(BIG, 20, 11)
    lab[1000:1030, 500:520] = 21                    # ymax = 1029 on the second trip
    lab[1029, 1030] = 22                            # a single pixel, the very last
    lab[200:210, 300:310] = 23
    lab[1029, 0] = 23                               # xmin and ymax on the second trip only
    return lab


def special_values(seg, raw_type, seed):
    """raw image for a stats test: mixed-sign values everywhere; then id 1 all negative, id 2 only -0.0 / +0.0, id 3
    denormals of both signs, id 4 with -inf and +inf (int32: INT_MIN and INT_MAX), as far as those ids have pixels.  On
    the BIG map ids 21 and 23 get their minimum and their maximum in the last 13 354 pixels."""
    rng = np.random.default_rng(seed)
    seg = np.asarray(seg)
    dtype = DTYPES[raw_type]
    if raw_type == I32:
        raw = rng.integers(-1000, 1000, size=seg.shape).astype(np.int32)
        raw[seg == 1] = -np.abs(raw[seg == 1]) - 1
        raw[seg == 2] = rng.integers(-1, 1, size=int((seg == 2).sum())).astype(np.int32)
        where = np.argwhere(seg == 4)
        if len(where) >= 2:
            raw[tuple(where[0])] = np.iinfo(np.int32).max
            raw[tuple(where[-1])] = np.iinfo(np.int32).min
        elif len(where) == 1:
            raw[tuple(where[0])] = np.iinfo(np.int32).min
        lo, hi = np.int32(-5000), np.int32(5000)
    else:
        raw = rng.normal(size=seg.shape).astype(dtype)
        raw[seg == 1] = -np.abs(raw[seg == 1]) - dtype(1)
        n2 = int((seg == 2).sum())
        raw[seg == 2] = np.where(np.arange(n2) % 2 == 0, dtype(-0.0), dtype(0.0))
        tiny = np.nextafter(dtype(0), dtype(1))
        n3 = int((seg == 3).sum())
        raw[seg == 3] = (rng.integers(-3, 4, size=n3) * tiny).astype(dtype)
        where = np.argwhere(seg == 4)
        if len(where) >= 2:
            raw[tuple(where[0])] = np.inf
            raw[tuple(where[-1])] = -np.inf
        elif len(where) == 1:
            raw[tuple(where[0])] = -np.inf
        lo, hi = dtype(-50), dtype(50)
    if seg.shape == BIG:
        assert seg[1027, 510] == 21 and seg[1028, 510] == 21 and seg[1029, 0] == 23
        raw[1027, 510] = lo
        raw[1028, 510] = hi
        raw[1029, 0] = hi
    return raw


# -------------------------------------------------------------------------------------------------- histogram fixtures
HIST_RANGES = [(0.0, 1.0), (-3.5, 7.25), (30000.0, 30000.75), (-1e-9, 1e-9), (-2.0, -1.0), (1e6, 1e6 + 40)]
NBINS = 256


def edge_values(lo, hi, dtype, n_uniform, rng):
    """values of one float instance: the 257 np.linspace edges of [lo, hi] in `dtype`, the representable neighbours of
    every edge on both sides (clipped to the range) and n_uniform uniform values; min and max are lo and hi themselves.
    Returns (values, edges)."""
    dtype = np.dtype(dtype).type
    lo, hi = dtype(lo), dtype(hi)
    edges = np.linspace(lo, hi, NBINS + 1, endpoint=True, dtype=dtype)
    below = np.clip(np.nextafter(edges, dtype(-np.inf)), lo, hi)
    above = np.clip(np.nextafter(edges, dtype(np.inf)), lo, hi)
    uniform = np.clip((lo + (hi - lo) * rng.random(n_uniform)).astype(dtype), lo, hi)
    values = np.concatenate([edges, below, above, uniform]).astype(dtype)
    return values, edges


def histogram_case(shape, dtype, n_uniform, seed):
    """label map + raw image for a float histogram launch: ids 1..6 carry the values of HIST_RANGES scattered over the map
    in random positions, id 7 has slot -1, ids 9 and -4 lie outside (0, nid) with nid = 9, id 8 is absent.
    -> (seg, raw, slot, nid, edges (6, 257))"""
    rng = np.random.default_rng(seed)
    npix = int(np.prod(shape))
    nid = 9
    seg = rng.choice(np.array([0, 7, 9, -4], dtype=np.int32), size=npix)
    raw = rng.normal(size=npix).astype(dtype)
    per = [edge_values(lo, hi, dtype, n_uniform, rng) for lo, hi in HIST_RANGES]
    total = sum(len(v) for v, _ in per)
    assert total <= npix, (total, npix)
    where = rng.permutation(npix)[:total]
    at = 0
    for k, (values, _) in enumerate(per):
        pos = where[at:at + len(values)]
        seg[pos] = k + 1
        raw[pos] = values
        at += len(values)
    slot = np.full(nid, -1, dtype=np.int32)
    slot[1:7] = [3, 0, 5, 1, 4, 2]                  # slots are not in id order
    edges = np.empty((6, NBINS + 1), dtype=dtype)
    for k, (_, e) in enumerate(per):
        edges[slot[k + 1]] = e
    return seg.reshape(shape), raw.reshape(shape), slot, nid, edges


def histogram_case_int(shape, seed):
    """int32 histogram launch: ids 1..4 with different vmin and widths, nbins = the widest (300); id 5 has slot -1, ids 6 and
    -1 lie outside (0, nid) with nid = 6.  Every instance's values fill [vmin, vmin + width); on top of that the widest
    one (id 2) gets values one below and one past its window and INT_MIN / INT_MAX (raw - vmin does not fit 32 bits), the
    narrower ones values below their window, and id 4's window ends at INT_MAX (vmin + nbins does not fit 32 bits).
    -> (seg, raw, slot, nid, vmin (4,), nbins, widths (4,)), vmin and widths by slot"""
    rng = np.random.default_rng(seed)
    nid = 6
    seg = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, -1], dtype=np.int32), size=shape)
    raw = np.zeros(shape, dtype=np.int32)
    vmin = np.array([-40, 2 ** 31 - 10, -7, 1000], dtype=np.int32)
    widths = np.array([300, 10, 120, 3], dtype=np.int64)
    slot = np.full(nid, -1, dtype=np.int32)
    slot[1:5] = [2, 0, 3, 1]
    for id_ in (1, 2, 3, 4):
        s = slot[id_]
        m = seg == id_
        v = int(vmin[s]) + rng.integers(0, widths[s], size=int(m.sum()))
        raw[m] = v.astype(np.int32)
    raw[seg == 5] = 3
    outliers = {2: (-41, 260, 2 ** 31 - 1, -2 ** 31, -40, 259), 1: (-8, -2 ** 31, -7, 112), 3: (999, 1002),
                4: (-2 ** 31, 2 ** 31 - 11, 2 ** 31 - 1, 0)}
    for id_, values in outliers.items():
        where = np.argwhere(seg == id_)
        for k, v in enumerate(values):
            raw[tuple(where[-1 - k])] = v                   # the last pixels: on the BIG map the second trip's
    return seg, raw, slot, nid, vmin, 300, widths
