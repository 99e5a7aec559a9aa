"""Restatement the radial distribution (clx_region_radial) is compared with; none of the kernel's code.

Ring: the two inequalities of include/clx.h, tried for every k from the last ring down in int64 (the bounds of the products
are asserted), so the smallest k that satisfies them stays; ring_relative / ring_absolute are the same in Python integers,
one pixel at a time.  Wedge: the eight sectors spelled out one by one as masks over (dy, dx).  q: np.rint(np.ldexp(float64(v),
shift)).  Sums: np.add.at.  The maps come from tests/inscribed_ref.py (ref_distance_sq, ref_inscribed)."""

import numpy as np

from inscribed_ref import DIST_INF, ref_distance_sq, ref_inscribed  # noqa: F401  (re-exported for the tests)

BAD_LABEL, BAD_VALUE, BAD_MAP, BAD_ROW = 1, 2, 4, 8


def ring_relative(d2, D2, rings):
    """smallest k in [0, rings) with d2 * rings^2 <= (k + 1)^2 * D2, in Python integers; needs 1 <= d2 <= D2"""
    d2, D2, rings = int(d2), int(D2), int(rings)
    assert 1 <= d2 <= D2 and rings >= 1
    for k in range(rings):
        if d2 * rings * rings <= (k + 1) * (k + 1) * D2:
            return k
    raise AssertionError("unreachable: k = rings - 1 satisfies the inequality")


def ring_absolute(d2, width, rings):
    """smallest k with d2 <= ((k + 1) * width)^2, clamped to rings - 1, in Python integers"""
    d2, width, rings = int(d2), int(width), int(rings)
    assert d2 >= 1 and width >= 1 and rings >= 1
    for k in range(rings):
        if d2 <= ((k + 1) * width) ** 2:
            return k
    return rings - 1


def ref_rings(d2, D2, rings, width):
    """vectorised over pixels: d2 and D2 int64 arrays of one shape (D2 is ignored with width > 0) -> int64 rings"""
    d2 = np.asarray(d2, dtype=np.int64)
    if width == 0:
        D2 = np.asarray(D2, dtype=np.int64)
        assert d2.size == 0 or (d2.min() >= 1 and (d2 <= D2).all() and int(D2.max()) <= 2 ** 50)
        lhs, scale = d2 * (rings * rings), D2                  # < 2^31 * 2^10; (k + 1)^2 * D2 <= 2^10 * 2^50
    else:
        assert d2.size == 0 or (d2.min() >= 1 and int(d2.max()) <= DIST_INF)
        lhs, scale = d2, np.full(d2.shape, width * width, dtype=np.int64)          # (32 * 2^15)^2 = 2^40
    ring = np.full(d2.shape, rings - 1, dtype=np.int64)        # absolute mode: what lies deeper; relative: k = rings - 1 holds
    for k in range(rings - 1, -1, -1):                         # descending: the smallest k that holds is written last
        ring = np.where(lhs <= (k + 1) * (k + 1) * scale, k, ring)
    return ring


def ref_wedge(dy, dx):
    """floor(atan2(dy, dx) / 45 degrees) with the angle in [0, 360), the eight sectors one by one; (0, 0) is in sector 0"""
    dy, dx = np.asarray(dy, dtype=np.int64), np.asarray(dx, dtype=np.int64)
    o = np.full(np.broadcast(dy, dx).shape, -1, dtype=np.int64)
    o[(dy == 0) & (dx == 0)] = 0
    o[(dx > 0) & (dy >= 0) & (dy < dx)] = 0                     # [0, 45): from the ray +x up to the diagonal
    o[(dx > 0) & (dy > 0) & (dy >= dx)] = 1                     # [45, 90): from the diagonal dy = dx up to the ray +y
    o[(dy > 0) & (dx <= 0) & (-dx < dy)] = 2                    # [90, 135): from the ray +y
    o[(dy > 0) & (dx < 0) & (-dx >= dy)] = 3                    # [135, 180): from the diagonal dy = -dx
    o[(dx < 0) & (dy <= 0) & (-dy < -dx)] = 4                   # [180, 225): from the ray -x
    o[(dx < 0) & (dy < 0) & (-dy >= -dx)] = 5                   # [225, 270): from the diagonal
    o[(dy < 0) & (dx >= 0) & (dx < -dy)] = 6                    # [270, 315): from the ray -y
    o[(dy < 0) & (dx > 0) & (dx >= -dy)] = 7                    # [315, 360): from the diagonal dy = -dx
    assert (o >= 0).all()
    return o


def ref_radial(labels, dist_sq, raw, nid, inscribed, row, nrows, rings, width, wedges, shift=0):
    """-> (count int64 (nrows, rings, wedges), isum int64 of the same shape (zeros without raw), bad).  labels: the map in its
    2-D / 3-D shape (the last axis is X); dist_sq, raw: npix values; inscribed (nid, 3); row (nid)"""
    labels = np.asarray(labels)
    X = labels.shape[-1]
    lab = labels.astype(np.int64).reshape(-1)
    npix = lab.size
    d = np.asarray(dist_sq).astype(np.int64).reshape(-1)
    inscribed = np.asarray(inscribed).astype(np.int64).reshape(nid, 3)
    row = np.asarray(row).astype(np.int64).reshape(nid)
    bad_label = (lab < 0) | (lab >= nid)
    idx = np.where(bad_label, 0, lab)
    obj = ~bad_label & (lab > 0)
    r = row[idx]
    bad_row = obj & (r >= nrows)
    taken = obj & (r >= 0) & (r < nrows)
    bad_value = np.zeros(npix, dtype=bool)
    q = np.zeros(npix, dtype=np.int64)
    if raw is not None:
        raw = np.ascontiguousarray(raw).reshape(-1)
        if raw.dtype == np.int32:
            q = raw.astype(np.int64)
        else:
            bound = float(2 ** 62 >> int(npix).bit_length())
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                t = np.rint(np.ldexp(raw.astype(np.float64), shift))
                fits = np.abs(t) <= bound                      # False for NaN
            bad_value = taken & ~fits
            q = np.where(fits, t, 0.0).astype(np.int64)
    D2, centre = inscribed[idx, 0], inscribed[idx, 1]
    bad_map = taken & ((d < 1) | (d > (D2 if width == 0 else DIST_INF)))
    if wedges == 8:
        bad_map |= taken & ((centre < 0) | (centre >= npix))
    keep = np.flatnonzero(taken & ~bad_value & ~bad_map)
    ring = ref_rings(d[keep], D2[keep], rings, width)
    wedge = np.zeros(len(keep), dtype=np.int64)
    if wedges == 8:
        assert labels.ndim == 2 or labels.shape[0] == 1
        wedge = ref_wedge(keep // X - centre[keep] // X, keep % X - centre[keep] % X)
    cell = (r[keep] * rings + ring) * wedges + wedge
    count = np.zeros(nrows * rings * wedges, dtype=np.int64)
    isum = np.zeros(nrows * rings * wedges, dtype=np.int64)
    np.add.at(count, cell, 1)
    np.add.at(isum, cell, q[keep])
    bad = BAD_LABEL * int(bad_label.any()) | BAD_VALUE * int(bad_value.any()) | BAD_MAP * int(bad_map.any()) | BAD_ROW * int(bad_row.any())
    shape = (nrows, rings, wedges)
    return count.reshape(shape), isum.reshape(shape), bad


def rows_of_all(nid):
    """row[id] = id - 1: every id in [1, nid) gets a row, nrows = nid - 1"""
    return np.arange(-1, nid - 1, dtype=np.int32), nid - 1
