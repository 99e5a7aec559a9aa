"""The convex hull integers of clx_region_hull restated for the tests, without the kernel's row-span shortcut: per object
ALL corner points of its pixels (np.unique), a lexicographic monotone chain in Python ints that drops collinear points,
then A2 by the shoelace formula, F2 by brute force over the hull vertices and (C, L2) by exact integer
cross-multiplication with the tie rule (the smaller l_e).  In 3-D F2 is the largest squared distance over all
voxel-corner points of the object.  Also the hand-made shapes both test tiers use."""

import numpy as np
from scipy import ndimage


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def strict_hull(points):
    """vertices of the convex hull of 2-D integer points, in order around it, no collinear point"""
    pts = sorted(set((int(p[0]), int(p[1])) for p in points))
    if len(pts) <= 2:
        return pts
    halves = []
    for seq in (pts, pts[::-1]):
        chain = []
        for p in seq:
            while len(chain) >= 2 and _cross(chain[-2], chain[-1], p) <= 0:
                chain.pop()
            chain.append(p)
        halves.append(chain[:-1])
    return halves[0] + halves[1]


def corner_points(coords):
    """coords (n, nd) pixel coordinates -> (m, nd) the distinct corner lattice points of those pixels"""
    coords = np.asarray(coords, dtype=np.int64)
    nd = coords.shape[1]
    offsets = np.array(list(np.ndindex((2,) * nd)), dtype=np.int64)
    return np.unique((coords[:, None, :] + offsets[None, :, :]).reshape(-1, nd), axis=0)


def width_pair(vertices):
    """(C, L2) over the edges of a polygon given by its vertices in order: the smallest c_e^2 / l_e, compared exactly,
    ties towards the smaller l_e"""
    best = None
    n = len(vertices)
    for i in range(n):
        a, b = vertices[i], vertices[(i + 1) % n]
        e = (b[0] - a[0], b[1] - a[1])
        c = max(abs(e[0] * (v[1] - a[1]) - e[1] * (v[0] - a[0])) for v in vertices)
        l = e[0] * e[0] + e[1] * e[1]
        if best is None or c * c * best[1] < best[0] * best[0] * l or (c * c * best[1] == best[0] * best[0] * l and l < best[1]):
            best = (c, l)
    return best


def hull_integers_2d(points):
    """[A2, NV, F2, C, L2] of 2-D integer points (Python ints)"""
    v = strict_hull(points)
    a2 = abs(sum(v[i][0] * v[(i + 1) % len(v)][1] - v[i][1] * v[(i + 1) % len(v)][0] for i in range(len(v))))
    f2 = max((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for p in v for q in v)
    c, l = width_pair(v)
    return [a2, len(v), f2, c, l]


def max_sq_distance(points, chunk=256):
    """largest squared distance between two of the integer points (m, nd), by brute force"""
    p = np.asarray(points, dtype=np.int64)
    best = 0
    for i in range(0, len(p), chunk):
        d = p[i:i + chunk, None, :] - p[None, :, :]
        best = max(best, int((d * d).sum(axis=2).max()))
    return best


def ref_hull(labels, nd, nid=None):
    """int64 (nid, 5): A2 NV F2 C L2 per id (3-D: F2 only); ids outside [0, nid) are background; absent ids and row 0: 0"""
    labels = np.asarray(labels)
    assert labels.ndim == nd
    nid = int(labels.max()) + 1 if nid is None else nid
    out = np.zeros((nid, 5), dtype=np.int64)
    clean = np.where((labels > 0) & (labels < nid), labels, 0)
    for i, box in enumerate(ndimage.find_objects(clean, max_label=nid - 1), 1):      # the boxes only say where to look
        if box is None:
            continue
        at = np.argwhere(clean[box] == i) + np.array([s.start for s in box])
        corners = corner_points(at)
        out[i] = hull_integers_2d(corners) if nd == 2 else [0, 0, max_sq_distance(corners), 0, 0]
    return out


def boxes_and_rows(labels, nid):
    """what the caller hands clx_region_hull, from NumPy: bbox int32 (nid, 6) in clx_region_moments' convention (absent:
    min 0x7fffffff, max -1), row_base int64 (nid) and the row count"""
    labels = np.asarray(labels)
    lab3 = labels.reshape((1,) * (3 - labels.ndim) + labels.shape)
    bbox = np.empty((nid, 6), dtype=np.int32)
    bbox[:, :3] = 0x7FFFFFFF
    bbox[:, 3:] = -1
    for i in np.unique(lab3):
        if i <= 0 or i >= nid:
            continue
        at = np.argwhere(lab3 == i)
        bbox[i, :3] = at.min(axis=0)
        bbox[i, 3:] = at.max(axis=0)
    return (bbox,) + rows_of(bbox)


def rows_of(bbox):
    """-> (row_base int64 (nid), rows): the exclusive prefix sum of the rows of every box, none for an absent id"""
    b = bbox.astype(np.int64)
    n = np.where(b[:, 3] >= 0, (b[:, 3] - b[:, 0] + 1) * (b[:, 4] - b[:, 1] + 1), 0)
    n[0] = 0
    return np.cumsum(n) - n, int(n.sum())


def shapes():
    """name -> (labels, nid): the hand-made 2-D shapes"""
    s = {}
    s["one_pixel"] = (np.ones((1, 1), np.int32), 2)
    row = np.zeros((5, 13), np.int32)
    row[2, 3:11] = 1
    s["one_row"] = (row, 2)
    s["one_column"] = (row.T.copy(), 2)
    s["fills_the_image_13x21"] = (np.full((13, 21), 3, np.int32), 4)
    ell = np.zeros((12, 14), np.int32)
    ell[1:11, 2:5] = 1
    ell[8:11, 2:12] = 1
    cee = np.zeros((12, 14), np.int32)
    cee[1:11, 2:12] = 2
    cee[4:8, 5:12] = 0                                   # open to the right
    ring = np.zeros((12, 14), np.int32)
    ring[1:11, 2:12] = 3
    ring[4:8, 5:9] = 0
    s["L"], s["C"], s["ring"] = (ell, 2), (cee, 3), (ring, 4)
    s["C_open_left"] = (cee[:, ::-1].copy(), 3)
    yy, xx = np.indices((16, 16))
    # two opposite corner pixels of the even board are 0: its hull is the box less two triangles of half a pixel; on the odd
    # board all four corner pixels are set and the hull is the box
    s["checkerboard_one_id_16x16"] = (((yy + xx) % 2).astype(np.int32), 2)
    s["checkerboard_one_id_15x15"] = (((yy + xx + 1) % 2).astype(np.int32)[:15, :15].copy(), 2)
    s["staircase_triangle_12"] = ((xx <= yy).astype(np.int32)[:12, :12].copy(), 2)     # a right triangle: collinear corners on the diagonal
    stairs = np.zeros((14, 30), np.int32)
    for k in range(12):
        stairs[1 + k, 2 + 2 * k:5 + 2 * k] = 1                              # a diagonal band, slope 2
    s["diagonal_staircase"] = (stairs, 2)
    combs = np.zeros((12, 20), np.int32)
    combs[0::2, 1:15] = 1
    combs[1::2, 4:19] = 2                                # rows alternate ids: every second row of either box is empty
    s["interleaved_combs"] = (combs, 3)
    y2, x2 = np.indices((27, 29))
    s["disc_12"] = (((y2 - 13) ** 2 + (x2 - 14) ** 2 <= 144).astype(np.int32), 2)
    bar = np.zeros((3, 44), np.int32)
    bar[1, 2:42] = 1
    s["bar_1x40"] = (bar, 2)
    trap = np.zeros((4, 14), np.int32)
    trap[1, 5:9] = 1
    trap[2, 1:13] = 1                                    # parallel edges of length 4 and 12 at the same width: the tie
    s["trapezoid_tie"] = (trap, 2)
    gaps = np.zeros((9, 30), np.int32)
    gaps[1:4, 2:9] = 3
    gaps[5:8, 4:6] = 9
    gaps[2:7, 20:28] = 17
    gaps[3, 22] = 0
    s["gaps_in_the_ids"] = (gaps, 20)
    return s
