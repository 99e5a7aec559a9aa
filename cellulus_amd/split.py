"""``split`` stage: what REPAIRS the label map a segmentation handed over -- objects that touch come out of connected components as
one clump, and every column of ``region_table`` then describes the clump as one cell.  CellProfiler's "declumping by shape"
and the textbook ``skimage.segmentation.watershed(-edt, markers)`` cut a clump along the necks of its distance transform with
a priority-queue flood on the host, whose result depends on the queue's order among equal values.  Here the result is a
function of the map alone, from exact integers, for every object in one call on the device (``csrc/label_basins.hip``:
``clx_label_basins``, ``clx_basin_passes``, ``clx_basin_relabel``); the one decision that needs a square root is taken on the
host, exactly, from one small table (``merge_basins``).

Definitions.  ``D = label_distance_sq(labels, edge)``; ``idx(p)`` is the raster index of pixel ``p``.  NEIGHBOURS are the 8
(2-D) or 26 (3-D) pixels around ``p`` inside the map that carry ``p``'s label; rows and slices never wrap.
HEIGHT: ``key(p) = (D[p] << 32) | (2^32 - 1 - idx(p))``: a larger ``D`` is higher, among equal ``D`` the smaller raster index; no
two pixels share a key, so there are no plateaus.  ASCENT: ``up(p)`` is the neighbour with the largest key if that exceeds
``key(p)``, else ``p`` itself, a SUMMIT.  ``root(p)`` is the summit the chain ``p, up(p), ...`` ends at; the BASIN of a summit is
the set of pixels rooted at it.  PASS: for two basins ``A != B``, ``pass(A, B)`` is the largest ``min(D[p], D[q])`` over
neighbouring ``p`` in ``A``, ``q`` in ``B``.  MERGE (``merge_basins``): the passes, sorted by ``(-pass, rootA, rootB)``, are walked
with a union-find in which every cluster keeps its TOP, the summit with the largest key; for a pass between two clusters the
one whose top is lower, ``lo``, joins the other iff ``sqrt(D[top(lo)]) - sqrt(pass) < depth`` -- its peak stands less than
``depth`` pixels above the neck.  ``depth = 0`` merges nothing; a refused pass is never looked at again.  PIECES: the surviving
clusters, sorted by (label of the object, raster index of the top) and numbered 1 .. n.  Parts of one label that are not
8- / 26-connected share no pass and are separate pieces at any depth.

    python -m cellulus_amd.split experiment.toml --source NAME --output NAME [--depth 1] [--edge]

writes ``split_labels`` of every sample and bandwidth of ``NAME`` into a new dataset of the segmentation container and
``split_bandwidth-<b>.csv``, one row per piece, next to the measure stage's files.
"""

import math

import numpy as np
import torch

from . import _stage
from .measure import (FLAGS, _call, _check_map, _distance_map, _in_type_of, _pair_capacity, _pair_slots, _scene, _Scene,
                      _workspace)
from .measure_columns import DIST_INF, _extents, _raster_columns, _real_fraction, _sqrt_ratio

MAX_SUMMITS = 1 << 30                   # clx_label_basins: capacity of the summit list; clx_basin_relabel: n
BASIN_NONE = -1                         # CLX_BASIN_NONE: root of a pixel of no basin
_DISTANCE_OUT_OF_RANGE = f"{{who}}: the distance map must lie in [0, {DIST_INF}] under the objects"
_ROOTS_CHANGED = "{who}: the roots changed under the relabelling"


def _depth(depth, who):
    """``depth`` as an exact Fraction: a real number >= 0"""
    return _real_fraction(depth, who, "depth")


def shallower(top_d2, pass_d2, depth):
    """``sqrt(top_d2) - sqrt(pass_d2) < depth`` for integers ``top_d2 >= pass_d2 >= 0`` and a Fraction ``depth >= 0``, decided
    exactly: with ``c = top_d2 - pass_d2 - depth²`` it is ``c < 2 depth sqrt(pass_d2)``, that is ``c < 0`` or ``c² < 4 depth²
    pass_d2``.  Equality does not merge"""
    top_d2, pass_d2 = int(top_d2), int(pass_d2)
    if not top_d2 >= pass_d2 >= 0:
        raise ValueError(f"shallower: needs top_d2 >= pass_d2 >= 0, got {top_d2} and {pass_d2}")
    if depth == 0:
        return False
    c = top_d2 - pass_d2 - depth * depth
    return c < 0 or c * c < 4 * depth * depth * pass_d2


def merge_basins(summit_labels, summit_d2, summits, passes, depth=1):
    """The merge of the basins of one map, on the host in Python integers and Fractions (no rounded square root).
    ``summits`` (n): the raster indices of the summits, ascending; ``summit_labels`` and ``summit_d2`` (n): the label and the
    squared distance under each; ``passes`` (m, 3): rows ``rootA, rootB, pass`` with ``rootA < rootB``, both among the summits
    and under one label; ``depth``: a real number >= 0 in pixels, taken exactly.  The module's docstring has the rule.
    Returns ``(piece, pieces)``: ``piece`` int64 (n), the piece 1 .. k of every summit, and ``pieces``, a dict of int64 arrays
    with one row per piece in the order of the ids: ``parent`` (the label), ``top`` (the raster index of its highest summit),
    ``top_d2``, and ``pass_d2``, the highest pass to another piece, -1 where it borders none."""
    who = "merge_basins"
    depth = _depth(depth, who)
    summits, labels, d2 = (np.asarray(v).astype(np.int64).reshape(-1) for v in (summits, summit_labels, summit_d2))
    passes = np.asarray(passes).astype(np.int64).reshape(-1, 3)
    n = len(summits)
    if not len(labels) == len(d2) == n:
        raise ValueError(f"{who}: summit_labels, summit_d2 and summits must have one length")
    if n and (np.any(np.diff(summits) <= 0) or summits[0] < 0 or d2.min() < 0 or d2.max() > DIST_INF):
        raise ValueError(f"{who}: needs increasing summits >= 0 and squared distances in [0, {DIST_INF}]")
    a, b = np.searchsorted(summits, passes[:, 0]), np.searchsorted(summits, passes[:, 1])
    if len(passes) and (np.any(passes[:, 0] >= passes[:, 1]) or b.max() >= n or np.any(summits[a] != passes[:, 0])
                        or np.any(summits[b] != passes[:, 1]) or np.any(labels[a] != labels[b])
                        or np.any(passes[:, 2] > np.minimum(d2[a], d2[b])) or passes[:, 2].min() < 0):
        raise ValueError(f"{who}: a pass needs rootA < rootB among the summits of one label and 0 <= pass <= both summits' distances")
    rows = sorted(zip((-passes[:, 2]).tolist(), passes[:, 0].tolist(), passes[:, 1].tolist(), a.tolist(), b.tolist()))
    d2_list, summit_list = d2.tolist(), summits.tolist()

    def higher(i, j):
        return (d2_list[i], -summit_list[i]) > (d2_list[j], -summit_list[j])

    parent = list(range(n))                                   # union-find over the summits' rows; a cluster's root is its top

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for minus_pass, _, _, i, j in rows:
        ci, cj = find(i), find(j)
        if ci == cj:
            continue
        lo, hi = (cj, ci) if higher(ci, cj) else (ci, cj)
        if shallower(d2_list[lo], -minus_pass, depth):
            parent[lo] = hi                                   # the higher top stays the root
    cluster = np.array([find(i) for i in range(n)], dtype=np.int64)
    roots = np.unique(cluster)                                # the surviving clusters, by the row of their top
    roots = roots[np.lexsort((summits[roots], labels[roots]))]
    piece_of_root = np.zeros(n, dtype=np.int64)
    piece_of_root[roots] = np.arange(1, len(roots) + 1)
    piece = piece_of_root[cluster]
    pass_d2 = np.full(len(roots), -1, dtype=np.int64)
    for minus_pass, _, _, i, j in rows:
        pi, pj = piece[i] - 1, piece[j] - 1
        if pi != pj:
            pass_d2[pi], pass_d2[pj] = max(pass_d2[pi], -minus_pass), max(pass_d2[pj], -minus_pass)
    return piece, {"parent": labels[roots], "top": summits[roots], "top_d2": d2[roots], "pass_d2": pass_d2}


def split_columns(parent, top, top_d2, pass_d2, area, shape):
    """The table of ``split_table`` from integers, one row per piece in the order of the ids: ``parent``, ``top``, ``top_d2``
    and ``pass_d2`` are ``merge_basins``' ``pieces``, ``area`` (n) the pieces' pixels, ``shape`` the map's 2 or 3 extents.
    Columns: ``label`` (1 .. n), ``parent`` (the label the piece was cut from), ``summit_z/_y/_x`` (2-D: y and x; the piece's
    highest pixel), ``summit_radius = sqrt(top_d2)`` (the radius of its largest inscribed ball), ``pass_radius = sqrt(pass_d2)``,
    the half-width of the widest neck to another piece of the same object (NaN: none), ``pieces_of_parent`` and ``area``; int64
    but the two radii, each of which is one correctly rounded root of an exact integer.  Host only."""
    who = "split_columns"
    _extents(shape, who)
    parent, top, top_d2, pass_d2, area = (np.asarray(v).astype(np.int64).reshape(-1) for v in (parent, top, top_d2, pass_d2, area))
    n = len(parent)
    if not len(top) == len(top_d2) == len(pass_d2) == len(area) == n:
        raise ValueError(f"{who}: parent, top, top_d2, pass_d2 and area must have one row per piece")
    if n and (top.min() < 0 or top.max() >= int(np.prod(shape)) or top_d2.min() < 0 or np.any(pass_d2 > top_d2) or area.min() < 1):
        raise ValueError(f"{who}: needs tops inside a map of shape {tuple(shape)}, pass_d2 <= top_d2 and area >= 1")
    table = {"label": np.arange(1, n + 1, dtype=np.int64), "parent": parent, **_raster_columns("summit", top, shape, who)}
    table["summit_radius"] = np.array([_sqrt_ratio(v, 1) for v in top_d2.tolist()], dtype=np.float64)
    table["pass_radius"] = np.array([_sqrt_ratio(v, 1) if v >= 0 else math.nan for v in pass_d2.tolist()], dtype=np.float64)
    _, inverse, counts = np.unique(parent, return_inverse=True, return_counts=True)
    table["pieces_of_parent"] = counts[inverse].astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    table["area"] = area
    return table


def _as_roots(values):
    """raster indices as the int32 words the library takes for uint32"""
    return torch.from_numpy(np.asarray(values, dtype=np.int64).astype(np.uint32).view(np.int32))


def _basins(scene, dist):
    """one clx_label_basins call (a second one where the first list was too short) -> (root, flat int32 on the device; the
    summits' raster indices, int64 ascending on the host)"""
    npix = scene.lab.numel()
    workspace, nbytes = _workspace(scene, "clx_label_basins_workspace", scene.lab.numel())
    root = torch.empty(npix, dtype=torch.int32, device=scene.device)
    capacity = min(npix, max(1024, npix // 64))
    while True:
        if capacity > MAX_SUMMITS:
            raise ValueError(f"{scene.who}: more summits than a list of {MAX_SUMMITS} holds")
        summits = torch.empty(capacity, dtype=torch.int32, device=scene.device)
        flags, count = _call(scene.device, scene.who, "clx_label_basins", {2: _DISTANCE_OUT_OF_RANGE}, scene.lab, dist, scene.nd, scene.Z,
                             scene.Y, scene.X, capacity, root, summits, FLAGS, workspace, nbytes, words=2)
        count &= 0xFFFFFFFF
        if not flags & 4:
            break
        capacity = count                                      # the count is exact: the second list fits
    return root, np.sort(summits[:count].cpu().numpy().view(np.uint32).astype(np.int64))


def _passes(scene, dist, root, nsummits):
    """clx_basin_passes -> (rootA, rootB, pass) int64, sorted by (rootA, rootB); no call where fewer than two summits are"""
    if nsummits < 2:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    keys, values = _pair_slots(scene.device, scene.who, "clx_basin_passes", {}, _pair_capacity(nsummits), scene.lab, dist, root, scene.nd,
                               scene.Z, scene.Y, scene.X)
    order = np.argsort(keys, kind="stable")                   # unsigned: (rootA << 32) | rootB is the (rootA, rootB) order
    keys = keys[order]
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), values[order]


def _front(labels, device, who):
    """the host checks on the map, then its scene"""
    _check_map(labels, who)
    return _scene(labels, device, who)


def basins(labels, edge=False, device=None):
    """The basins of the distance map of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as
    ``region_table``): ``(root, summits)``.  ``root``: an int32 DEVICE tensor in the shape of ``labels``, for every object pixel
    the raster index of the summit its steepest ascent ends at (to be read as uint32 on maps of 2^31 pixels and more), ``-1`` on
    background.  ``summits``: the raster indices of the summits, int64 ascending, on the host.  ``edge`` is
    ``label_distance_sq``'s.  The module's docstring has the definitions.  Runs on a HIP device; there is no CPU path."""
    scene = _front(labels, device, "basins")
    if scene.lab.numel() == 0 or scene.nid == 1:
        return torch.full(scene.spatial, BASIN_NONE, dtype=torch.int32, device=scene.device), np.zeros(0, dtype=np.int64)
    root, summits = _basins(scene, _distance_map(scene, edge))
    return root.reshape(scene.spatial), summits


def basin_passes(labels, edge=False, device=None):
    """The passes between the basins of ``labels`` (``basins``' arguments): ``(rootA, rootB, pass)``, int64 arrays on the host
    with one row per pair of basins of one object that have neighbouring pixels, ``rootA < rootB`` the raster indices of their
    summits and ``pass`` the largest ``min(D[p], D[q])`` over their neighbouring pixels; sorted by ``(rootA, rootB)``.  A table
    that proves too small is doubled and filled again inside.  Runs on a HIP device; there is no CPU path."""
    scene = _front(labels, device, "basin_passes")
    if scene.lab.numel() == 0 or scene.nid == 1:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    dist = _distance_map(scene, edge)
    root, summits = _basins(scene, dist)
    return _passes(scene, dist, root, len(summits))


def _split(labels, depth, edge, device, who, table=False, fits=None):
    """-> (scene, the new map as a flat int32 device tensor or None for a map without objects, the piece table or None).
    ``fits(n)``: called with the number of pieces before the map is written"""
    depth = _depth(depth, who)
    scene = _front(labels, device, who)
    if scene.lab.numel() == 0 or scene.nid == 1:
        none = np.zeros(0, dtype=np.int64)
        return scene, None, split_columns(none, none, none, none, none, scene.spatial) if table else None
    dist = _distance_map(scene, edge)
    root, summits = _basins(scene, dist)
    a, b, height = _passes(scene, dist, root, len(summits))
    at = torch.from_numpy(summits).to(scene.device)
    piece, pieces = merge_basins(scene.lab[at].cpu().numpy(), dist[at].cpu().numpy(), summits, np.stack([a, b, height], axis=1), depth)
    if fits is not None:
        fits(len(pieces["top"]))
    out = torch.empty_like(scene.lab)
    workspace, nbytes = _workspace(scene, "clx_label_basins_workspace", scene.lab.numel())
    scene.call("clx_basin_relabel", {1 | 2: _ROOTS_CHANGED}, root, scene.lab.numel(), _as_roots(summits).to(scene.device),
               torch.from_numpy(piece.astype(np.int32)).to(scene.device), len(summits), out, FLAGS, workspace, nbytes)
    if not table:
        return scene, out, None
    n = len(pieces["top"])
    new = _Scene(who, out, scene.device, scene.nd, scene.spatial, n + 1).measured()
    return scene, out, split_columns(pieces["parent"], pieces["top"], pieces["top_d2"], pieces["pass_d2"], new.area[1:], scene.spatial)


def _dtype_max(labels):
    return torch.iinfo(labels.dtype).max if torch.is_tensor(labels) else np.iinfo(labels.dtype).max


def split_labels(labels, depth=1, edge=False, device=None):
    """``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as ``region_table``) with every object
    cut into its pieces: the basins of its distance map, merged where a peak stands less than ``depth`` pixels (a real number
    >= 0, taken exactly; 0 keeps every basin) above the neck to a higher one.  The pieces are numbered 1 .. n by (old label,
    raster index of the piece's highest pixel); background stays 0; parts of one label that do not touch get ids of their own.
    The result has the type, dtype and device of ``labels``; ValueError if n does not fit the dtype.  ``edge`` is
    ``label_distance_sq``'s.  A function of the map alone: the same bits in every run.  Runs on a HIP device; there is no CPU
    path."""
    who = "split_labels"

    def fits(n):
        if n > _dtype_max(labels):
            raise ValueError(f"{who}: {n} pieces do not fit {labels.dtype}")

    scene, out, _ = _split(labels, depth, edge, device, who, fits=fits)
    return _in_type_of(labels, scene, out)


def split_table(labels, depth=1, edge=False, device=None):
    """The table of the pieces ``split_labels`` cuts ``labels`` into, one row per piece: ``split_columns`` lists the columns.  A
    map without objects gives an empty table with these columns.  Runs on a HIP device; there is no CPU path."""
    return _split(labels, depth, edge, device, "split_table", table=True)[2]


def split_stage(inference_config, source, output, depth=1, edge=False) -> None:
    """For every sample and bandwidth of ``source``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (``segment()``'s, say): ``split_labels(labels, depth, edge)`` into a new
    uint16 dataset ``output`` of that container and ``split_table``'s rows of all samples as ``split_bandwidth-<b>.csv`` in the
    working directory -- a header line, then ``sample`` and the table's columns, floats as ``%.17g``.  Rank 0 works alone under
    torch.distributed."""
    who = "split_stage"
    if not isinstance(source, str) or not source:
        raise ValueError(f"{who}: source must be the name of a dataset, got {source!r}")
    if not isinstance(output, str) or not output or output == source:
        raise ValueError(f"{who}: output must name a new dataset other than source, got {output!r}")
    _depth(depth, who)
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    stage.open("a", source)
    stage.refuse_existing(output)
    ds_source, ds_output = stage.f[source], stage.create(output)

    def fits(n):
        if n > np.iinfo(np.uint16).max:
            raise ValueError(f"{who}: {n} pieces do not fit uint16")

    def per_sample(sample, bandwidth):
        labels = ds_source[sample, bandwidth].astype(np.int32)
        scene, out, table = _split(labels, depth, edge, stage.device, who, table=True, fits=fits)
        ds_output[sample, bandwidth] = _in_type_of(labels, scene, out).astype(np.uint16)
        return (table,)

    stage.run(per_sample, ("split",))


if __name__ == "__main__":
    from .cli import split as _command

    _command()
