"""NumPy / scipy restatements of what clx_region_topology counts and of the columns formed from it, shared by
test_cpu_topology.py, test_gpu_topology.py and test_gpu_topology_stage.py.  None follows the kernel's formulation (a
walk over windows, a mask per id, a table): the window sums are comparisons of shifted views of the zero-padded map with
np.bincount per id, the Euler numbers are counted cell by cell on the doubled (Khalimsky) grid and, in 2-D, from
scipy.ndimage.label on the mask and its padded complement."""

import itertools
import math

import numpy as np
from scipy import ndimage as ndi

from contacts_ref import clean

NT = 5                                                  # T1 T2 T3 E_hi E_lo


def _counted(labels, nd):
    """the map as an array of its `nd` counted axes"""
    lab = np.asarray(labels)
    if nd == 2:
        assert lab.ndim == 2 or lab.shape[0] == 1, "nd == 2 needs Z == 1"
        return lab.reshape(lab.shape[-2:])
    return lab.reshape((1,) * (3 - lab.ndim) + lab.shape)


def _views(padded, nd):
    """view v (bit nd-1-k of v: the offset along axis k) of the padded map: voxel v of every window"""
    shape = [s - 1 for s in padded.shape]
    out = []
    for off in itertools.product((0, 1), repeat=nd):
        out.append(padded[tuple(slice(o, o + s) for o, s in zip(off, shape))])
    return out


def _cells(nd):
    """the d-cells through a vertex as (d, voxel numbers): d chosen axes and a side along each"""
    voxels = list(itertools.product((0, 1), repeat=nd))
    for axes in itertools.product((False, True), repeat=nd):
        chosen = [k for k in range(nd) if axes[k]]
        for side in itertools.product((0, 1), repeat=len(chosen)):
            yield len(chosen), [n for n, v in enumerate(voxels) if all(v[k] == s for k, s in zip(chosen, side))]


def ref_window_sums(labels, nd, nid=None):
    """-> int64 (nid, 5): T1 T2 T3 E_hi E_lo of every id, row 0 left at 0.  All ids at once: a pair of voxels with
    different values adds to both values' ids; a cell adds to every distinct id among its voxels (E_hi) or to the one id
    that all its voxels carry (E_lo)."""
    lab = _counted(labels, nd).astype(np.int64)
    nid = int(lab.max()) + 1 if nid is None else nid
    lab = clean(lab, nid)
    views = _views(np.pad(lab, 1), nd)
    voxels = list(itertools.product((0, 1), repeat=nd))
    counts = np.zeros((nid, NT), dtype=np.int64)

    def add(column, ids, weight=1):
        counts[:, column] += weight * np.bincount(ids[ids > 0], minlength=nid)

    for a, b in itertools.combinations(range(len(voxels)), 2):
        k = sum(p != q for p, q in zip(voxels[a], voxels[b]))
        differ = views[a] != views[b]
        add(k - 1, views[a][differ])
        add(k - 1, views[b][differ])
    for d, members in _cells(nd):
        w = 1 << (nd - d)
        s = np.sort(np.stack([views[n] for n in members], axis=-1), axis=-1)
        add(3, s[..., 0].ravel(), (-1) ** d * w)
        for j in range(1, len(members)):
            add(3, s[..., j][s[..., j] != s[..., j - 1]], (-1) ** d * w)
        add(4, s[..., 0][s[..., 0] == s[..., -1]], (-1) ** (nd - d) * w)
    counts[0] = 0
    return counts


def mask_window_sums(mask):
    """-> [T1, T2, T3, E_hi, E_lo] of one boolean mask (its own number of axes is nd), by the definitions"""
    mask = np.asarray(mask, dtype=bool)
    nd = mask.ndim
    views = _views(np.pad(mask, 1), nd)
    voxels = list(itertools.product((0, 1), repeat=nd))
    out = [0] * NT
    for a, b in itertools.combinations(range(len(voxels)), 2):
        out[sum(p != q for p, q in zip(voxels[a], voxels[b])) - 1] += int((views[a] != views[b]).sum())
    for d, members in _cells(nd):
        w = 1 << (nd - d)
        stack = np.stack([views[n] for n in members])
        out[3] += (-1) ** d * w * int(stack.any(axis=0).sum())
        out[4] += (-1) ** (nd - d) * w * int(stack.all(axis=0).sum())
    return out


def euler_by_cells(mask):
    """-> (chi_hi, chi_lo) of a boolean mask: the cells of the doubled grid (odd index: the open extent of a voxel along
    that axis, even index: a lattice plane), a cell's dimension being its number of odd indices.  The closed complex has
    a cell if ANY voxel around it is set, the open one if ALL are (the outside is not set); chi_hi = sum (-1)^dim over
    the closed complex, chi_lo = sum (-1)^(nd - dim) over the open one."""
    mask = np.pad(np.asarray(mask, dtype=bool), 1)
    nd = mask.ndim
    odd = tuple(slice(1, None, 2) for _ in range(nd))
    grid = tuple(2 * s + 1 for s in mask.shape)
    is_set, not_set = np.zeros(grid, dtype=bool), np.zeros(grid, dtype=bool)
    is_set[odd] = mask
    not_set[odd] = ~mask
    around = np.ones((3,) * nd, dtype=bool)
    closed = ndi.binary_dilation(is_set, around)
    opened = ~ndi.binary_dilation(not_set, around)
    dim = sum(np.arange(g).reshape([-1 if k == a else 1 for k in range(nd)]) % 2 for a, g in enumerate(grid))
    sign = np.where(dim % 2 == 0, 1, -1)
    return int((sign * closed).sum()), int(((-1) ** nd * sign * opened).sum())


def euler_by_label_2d(mask):
    """-> (components_8 - holes_4, components_4 - holes_8) of a 2-D mask"""
    mask = np.asarray(mask, dtype=bool)
    outside = np.pad(~mask, 1, constant_values=True)      # one component of it is the outside, the others are holes
    full, cross = np.ones((3, 3), dtype=bool), ndi.generate_binary_structure(2, 1)
    return (ndi.label(mask, full)[1] - (ndi.label(outside, cross)[1] - 1),
            ndi.label(mask, cross)[1] - (ndi.label(outside, full)[1] - 1))


def direction_weights():
    """(w1, w2, w3): the spherical Voronoi cell areas of the 26 lattice directions over 4 pi, antipodes pooled, for the
    axial, face-diagonal and space-diagonal directions"""
    from scipy.spatial import SphericalVoronoi

    d = np.array([v for v in itertools.product((-1, 0, 1), repeat=3) if any(v)], dtype=np.float64)
    kind = (d != 0).sum(axis=1)
    areas = SphericalVoronoi(d / np.linalg.norm(d, axis=1)[:, None]).calculate_areas() / (4.0 * np.pi)
    return tuple(2.0 * float(areas[kind == k].mean()) for k in (1, 2, 3))


def ref_topology_columns(area, counts, nd, weights=None):
    """the columns of region_table(topology=True) from areas (n) and window sums (n, 5), in plain float64 arithmetic"""
    area = np.asarray(area, dtype=np.int64).reshape(-1)
    c = np.asarray(counts, dtype=np.int64).reshape(-1, NT)
    assert (c[:, 3] % (1 << nd) == 0).all() and (c[:, 4] % (1 << nd) == 0).all()
    cols = {"euler_number": c[:, 3] // (1 << nd), "euler_number_conn1": c[:, 4] // (1 << nd)}
    t = c[:, :3].astype(np.float64)
    if nd == 2:
        cols["perimeter_crofton"] = (math.pi / 8.0) * (t[:, 0] / 2.0 + t[:, 1] / math.sqrt(2.0))
    else:
        w1, w2, w3 = weights or direction_weights()
        n1, n2, n3 = t[:, 0] / 4.0, t[:, 1] / 2.0, t[:, 2]
        surface = 4.0 * (w1 * n1 / 2.0 + w2 * n2 / (2.0 * math.sqrt(2.0)) + w3 * n3 / (2.0 * math.sqrt(3.0)))
        cols["surface_area"] = surface
        with np.errstate(divide="ignore", invalid="ignore"):
            cols["sphericity"] = math.pi ** (1.0 / 3.0) * (6.0 * area.astype(np.float64)) ** (2.0 / 3.0) / surface
    return cols


def ref_topology_table(labels, weights=None):
    """the topology columns per id present in `labels` (2-D or 3-D), ascending"""
    labels = np.asarray(labels)
    nd = labels.ndim
    ids = np.unique(labels)
    ids = ids[ids > 0].astype(np.int64)
    counts = ref_window_sums(labels, nd)
    area = np.bincount(labels.ravel().astype(np.int64), minlength=counts.shape[0])
    return ref_topology_columns(area[ids], counts[ids], nd, weights), counts[ids]
