"""NumPy / scipy.ndimage restatements of what clx_region_contacts and clx_region_perimeter count, shared by
test_cpu_contacts.py, test_gpu_contacts.py and test_gpu_contacts_stage.py.  Neither follows the kernels' formulation:
the contacts are shifted comparisons of the zero-padded map and np.unique, the perimeter is scikit-image's own recipe
(mask minus its erosion, a 3 x 3 convolution, a histogram of the codes) per object."""

import math

import numpy as np
from scipy import ndimage as ndi

CROSS = ndi.generate_binary_structure(2, 1)
KERNEL = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
CODES = ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))            # weight 1, sqrt 2, (1 + sqrt 2) / 2
WEIGHTS = np.zeros(50, dtype=np.float64)
WEIGHTS[list(CODES[0])] = 1.0
WEIGHTS[list(CODES[1])] = math.sqrt(2.0)
WEIGHTS[list(CODES[2])] = (1.0 + math.sqrt(2.0)) / 2.0


def clean(labels, nid):
    """ids outside [0, nid) become 0"""
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab < 0) | (lab >= nid), 0, lab)


def ref_contacts(labels, nd, nid=None):
    """-> (keys uint64 ascending, counts int64): faces between different ids, the outside of the image being id 0 along
    the counted axes (the last `nd` of the map seen as [Z][Y][X])"""
    lab = np.asarray(labels).astype(np.int64)
    lab = lab.reshape((1,) * (3 - lab.ndim) + lab.shape)
    if nid is not None:
        lab = clean(lab, nid)
    axes = range(3 - nd, 3)
    pad = np.pad(lab, [(1, 1) if ax in axes else (0, 0) for ax in range(3)])
    found = []
    for ax in axes:
        n = pad.shape[ax]
        lo, hi = np.take(pad, range(0, n - 1), axis=ax), np.take(pad, range(1, n), axis=ax)
        differ = lo != hi
        a, b = np.minimum(lo, hi)[differ], np.maximum(lo, hi)[differ]
        found.append((a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64))
    keys, counts = np.unique(np.concatenate(found), return_counts=True)
    return keys.astype(np.uint64), counts.astype(np.int64)


def ref_perimeter(labels, nid):
    """-> (classes int64 (nid, 4), perimeter float64 (nid)) of a 2-D map; row 0 stays 0"""
    lab = clean(labels, nid)
    classes = np.zeros((nid, 4), dtype=np.int64)
    perimeter = np.zeros(nid, dtype=np.float64)
    for i, box in enumerate(ndi.find_objects(lab.astype(np.int32), max_label=nid - 1), 1):
        if box is None:
            continue
        mask = np.pad(lab[box] == i, 2)                           # zeros around it: other ids and the outside alike
        border = mask & ~ndi.binary_erosion(mask, CROSS, border_value=0)
        codes = ndi.convolve(border.astype(np.int64), KERNEL, mode="constant", cval=0)
        hist = np.bincount(codes.ravel(), minlength=50)
        classes[i] = [int(border.sum())] + [int(hist[list(c)].sum()) for c in CODES]
        perimeter[i] = hist @ WEIGHTS
    return classes, perimeter


def ref_boundary_columns(labels):
    """the boundary columns of region_table(boundary=True) per id present, ascending, from the two restatements"""
    labels = np.asarray(labels)
    nd = labels.ndim
    ids = np.unique(labels)
    ids = ids[ids > 0].astype(np.int64)
    keys, counts = ref_contacts(labels, nd)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    cols = {k: np.zeros(len(ids), dtype=np.int64) for k in ("boundary_faces", "contact_faces", "num_neighbours", "touches_border")}
    for r, i in enumerate(ids):
        mine = (a == i) | (b == i)
        cols["boundary_faces"][r] = counts[mine].sum()
        cols["contact_faces"][r] = counts[mine & (a > 0)].sum()
        cols["num_neighbours"][r] = int((mine & (a > 0)).sum())
        where = np.argwhere(labels == i)
        cols["touches_border"][r] = int(any(where[:, k].min() == 0 or where[:, k].max() == labels.shape[k] - 1 for k in range(nd)))
    if nd == 2:
        classes, perimeter = ref_perimeter(labels, int(labels.max()) + 1)
        cols["border_pixels"] = classes[ids, 0]
        cols["perimeter"] = perimeter[ids]
    return cols, (a, b, counts)
