"""Restatements the label-aware distance map and the inscribed circle / ball are compared with; none of the kernels' passes.

ref_distance_sq: per object value, scipy.ndimage.distance_transform_edt of the object's mask on its bounding box grown by one
pixel and clipped to the map; d^2 = rint(d * d) (d is the float64 root of an integer below 2^30: d * d is off by far less
than 0.5).  The crop is exact: a candidate outside the grown box, moved coordinate by coordinate onto the box's nearest face,
lands on a pixel that is not the object's (every pixel of the grown layer is outside the object's own box) and is no farther
from any pixel of the object.  With `edge` the whole map is first padded with one layer of 0.  A map of one non-zero value has
no candidate without `edge`: DIST_INF.

brute_distance_sq: all pixel pairs in NumPy integers, for maps of up to about 200 pixels; no scipy."""

import numpy as np
from scipy import ndimage

DIST_INF = 1 << 30


def ref_distance_sq(labels, edge):
    """labels: 2-D or 3-D integers, every axis counted -> int64 map of the same shape"""
    labels = np.asarray(labels).astype(np.int64)
    lab = np.pad(labels, 1) if edge else labels
    out = np.zeros(lab.shape, dtype=np.int64)
    values = np.unique(lab)
    boxes = ndimage.find_objects(np.searchsorted(values, lab).astype(np.int32) + 1)     # slot v + 1: works for negative values
    for value, box in zip(values, boxes):
        if value == 0:
            continue
        grown = tuple(slice(max(0, s.start - 1), min(n, s.stop + 1)) for s, n in zip(box, lab.shape))
        mask = lab[grown] == value
        if mask.all():                                                  # the whole map is this object
            assert mask.shape == lab.shape and not edge
            out[grown] = DIST_INF
            continue
        d = ndimage.distance_transform_edt(mask)
        d2 = np.rint(d * d).astype(np.int64)
        out[grown][mask] = d2[mask]
    return out[(slice(1, -1),) * lab.ndim] if edge else out


def brute_distance_sq(labels, edge):
    labels = np.asarray(labels).astype(np.int64)
    lab = np.pad(labels, 1) if edge else labels
    assert lab.size <= 600
    coords = np.indices(lab.shape).reshape(lab.ndim, -1).T.astype(np.int64)
    flat = lab.reshape(-1)
    diff = coords[:, None, :] - coords[None, :, :]
    d2 = (diff * diff).sum(axis=2)
    other = flat[:, None] != flat[None, :]
    best = np.where(other, d2, DIST_INF).min(axis=1)
    best[flat == 0] = 0
    out = best.reshape(lab.shape)
    return out[(slice(1, -1),) * lab.ndim] if edge else out


def ref_inscribed(labels, dist_sq, nid):
    """-> (out int64 (nid, 3): max d^2, smallest flat index that attains it, Σ d^2; bad) over the pixels with a label in
    [1, nid) and a distance in [0, DIST_INF]: a sort by (label, distance descending, index), first entry of every label"""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    d = np.asarray(dist_sq).astype(np.int64).reshape(-1)
    bad_label = (lab < 0) | (lab >= nid)
    bad_dist = ~bad_label & (lab > 0) & ((d < 0) | (d > DIST_INF))
    keep = np.flatnonzero(~bad_label & ~bad_dist & (lab > 0))
    out = np.zeros((nid, 3), dtype=np.int64)
    order = keep[np.lexsort((keep, -d[keep], lab[keep]))]
    first = order[np.r_[True, lab[order][1:] != lab[order][:-1]]] if len(order) else order
    out[lab[first], 0] = d[first]
    out[lab[first], 1] = first
    np.add.at(out[:, 2], lab[keep], d[keep])
    return out, int(bad_label.any()) | 2 * int(bad_dist.any())
