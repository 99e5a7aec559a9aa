"""``skeleton`` stage: what THINS the objects of a label map to their centre lines and measures the lines -- how long an
elongated or branching object (a neurite, a filament, a hypha, a clump with necks) is along itself, how often it branches, how
many free ends it has and how wide it is along its axis.  CellProfiler's MorphologicalSkeleton / MeasureObjectSkeleton, MATLAB's
``bwmorph('thin')`` and ``skimage.morphology.thin`` work on one mask on the host; here all objects are thinned in one pass on
the device (``csrc/label_thin.hip``: ``clx_label_thin``, ``clx_skeleton_census``), label-aware.  ``fill -> skeleton`` is a
chain: a pinhole becomes a loop of the skeleton.

Definitions.  The input is one map.  Every non-zero value is an OBJECT pixel.  A 3-D map is thinned slice by slice
(``planewise=True``; 3-D curve skeletons are not done); rows and slices never wrap.  The NEIGHBOURS of a pixel p are
``P2 .. P9`` = N, NE, E, SE, S, SW, W, NW, N at ``y - 1``; ``Pk = 1`` iff that pixel lies inside the slice, is still alive and
carries p's label, so touching objects thin independently.  With

    C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
    N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),   N = min(N1, N2)

a SUB-ITERATION deletes every alive pixel with ``C == 1``, ``2 <= N <= 3`` and ``m == 0``, all at once from the state before
it; odd sub-iterations have ``m = (P2 | P3 | !P5) & P4``, even ones ``m = (P6 | P7 | !P9) & P8`` (Guo & Hall 1989, algorithm
A1).  An ITERATION is an odd, then an even sub-iteration; the SKELETON is the state after the first iteration that deletes
nothing, or after ``max_iter`` iterations.  Thinning keeps every object's 8-connected components and holes.

On the thinned map, per label: a FACE LINK is a pair of face neighbours, a DIAGONAL LINK a pair of diagonal neighbours neither
of whose two common face neighbours carries the label, a BLOCK a 2 x 2 window full of the label; the DEGREE of a pixel is the
number of its links, an END has degree 1, a BRANCH POINT (junction pixel) degree >= 3, an ISOLATED pixel degree 0.
``pixels - face_links - diag_links + blocks`` is the label's Euler number with 8-connectivity.

The BRANCH GRAPH (``branch_graph``, ``csrc/skeleton_graph.hip``: ``clx_skeleton_graph``; skan's ``summarize``, CellProfiler's
MeasureObjectSkeleton, ImageJ's AnalyzeSkeleton) contracts these links, on any map.  A PATH pixel has degree 2.  A NODE is a
maximal set of junction pixels connected by links between two junction pixels (kind 3), an end pixel alone (kind 1) or an
isolated pixel alone (kind 0); its id is its smallest raster index.  A BRANCH is a maximal set of path pixels connected by links
between two path pixels together with every link from one of them to a pixel that is no path pixel, or a DIRECT branch: a
single link between an end pixel and a junction pixel or between two end pixels.  Links between two junction pixels belong to
their node.  A branch has two terminals or none; its kind is 0 end-end, 1 end-junction (a SPUR), 2 junction-junction, 3 CYCLE (a
full 2 x 2 block on its own is a cycle of 4 pixels).  ``prune_spurs`` removes the spurs shorter than a length, the junction
staying, one round per library call.  Trunk / branch classification against a second object set, 3-D curve skeletons and
loop-aware pruning are not done.

    python -m cellulus_amd.skeleton infer.toml --source NAME --output NAME [--max-iter N] [--planewise] [--radius] [--prune L]
                                    [--graph]

writes ``thin_labels`` of every sample and bandwidth of ``NAME`` (with ``--prune`` after one round of ``prune_spurs``) into a
new dataset of the segmentation container and ``skeleton_bandwidth-<b>.csv``, one row per label, next to the measure stage's
files; with ``--graph`` that file has the ``graph_columns`` too and ``skeleton_branches_bandwidth-<b>.csv`` one row per branch.
"""

import heapq
import math
import numbers

import numpy as np
import torch

from . import _clx, _stage
from .measure import FLAGS, LABELS_OUT_OF_RANGE, _check_map, _distance_map, _in_type_of, _scene, _Scene, _workspace

CALL_ITERATIONS = 64                    # clx_label_thin: the iterations a call queues at most
CENSUS_WORDS = 10                       # clx_skeleton_census: words per label
REFUSE_3D = "{who}: 3-D thinning is not implemented; planewise=True thins every slice on its own"
REFUSE_3D_GRAPH = "{who}: 3-D curve skeletons are not implemented; planewise=True takes every slice as a map of its own"
BRANCH_WORDS = ("first", "label", "kind", "path_pixels", "face_links", "diag_links", "pixel_a", "pixel_b", "node_a", "node_b",
                "d2_sum", "d2_min", "d2_max")                   # clx_skeleton_graph: a branch row
NODE_WORDS = ("first", "label", "kind", "pixels", "links_out", "inner_face", "inner_diag")     # ... and a node row
END_END, SPUR, JUNCTION_JUNCTION, CYCLE = 0, 1, 2, 3           # a branch's kind
JUNCTION = 3                                                    # a node's kind: a cluster of junction pixels (1: end, 0: isolated)
GRAPH_CAPACITY = 1 << 14                # rows of each kind the first clx_skeleton_graph call of branch_graph has room for
LIMIT_Q10_END = 1 << 30                 # clx_skeleton_graph: limit_q10 lies below it


def _max_iter(max_iter, who):
    if max_iter is None:
        return None
    if isinstance(max_iter, bool) or not isinstance(max_iter, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: max_iter must be an integer or None, got {type(max_iter).__name__}")
    if not 0 <= int(max_iter) < 1 << 31:
        raise ValueError(f"{who}: max_iter must lie in [0, 2^31), got {max_iter!r}")
    return int(max_iter)


def _flag(value, name, who):
    if not isinstance(value, (bool, np.bool_)):
        raise TypeError(f"{who}: {name} must be a bool, got {type(value).__name__}")
    return bool(value)


def _planewise(planewise, nd, who, refuse=REFUSE_3D):
    planewise = _flag(planewise, "planewise", who)
    if planewise and nd == 2:
        raise ValueError(f"{who}: planewise needs a 3-D map")
    if nd == 3 and not planewise:
        raise ValueError(refuse.format(who=who))
    return planewise


def _limit_q10(min_length, who, name="min_length"):
    """a length in pixels -> clx_skeleton_graph's limit in units of 1/1024 pixel, rounded UP: ``ceil(min_length * 1024)``, so
    that a spur is pruned iff its length is below the smallest multiple of 1/1024 that is >= min_length"""
    if isinstance(min_length, (bool, np.bool_)) or not isinstance(min_length, (numbers.Real, np.integer, np.floating)):
        raise TypeError(f"{who}: {name} must be a number, got {type(min_length).__name__}")
    if not math.isfinite(min_length) or min_length < 0 or math.ceil(float(min_length) * 1024) >= LIMIT_Q10_END:
        raise ValueError(f"{who}: {name} must lie in [0, 2^20), got {min_length!r}")
    return math.ceil(float(min_length) * 1024)


def skeleton_columns(label, area, words, radius=False):
    """The table of ``skeleton_table`` from integers.  ``label`` (n): the labels present, ascending; ``area`` (n): their pixels
    in the input map; ``words`` (n, 10): their rows of ``clx_skeleton_census`` on the thinned map -- pixels, face_links,
    diag_links, blocks, ends, junctions, isolated, d2_sum, d2_min, d2_max.  Columns: ``label``, ``area``, ``skeleton_pixels``,
    ``skeleton_length = face_links + sqrt(2) * diag_links`` (float64), ``skeleton_end_points``, ``skeleton_branch_points``,
    ``skeleton_isolated``, ``skeleton_euler_number = pixels - face_links - diag_links + blocks``, and with ``radius``
    ``skeleton_radius_min`` and ``skeleton_radius_max`` (the square roots of d2_min and d2_max) and ``skeleton_dist_sq_mean``
    (d2_sum / pixels), float64; a label none of whose skeleton pixels has a finite distance (``d2_max < 0``: the map is one
    object everywhere) has ``inf`` in the three.  Integers are int64.  Host only."""
    who = "skeleton_columns"
    label, area = (np.asarray(v).astype(np.int64).reshape(-1) for v in (label, area))
    words = np.asarray(words).astype(np.int64).reshape(-1, CENSUS_WORDS)
    n = len(label)
    if len(area) != n or len(words) != n:
        raise ValueError(f"{who}: label, area and words must have one row per label")
    if n and (np.any(np.diff(label) <= 0) or np.any(label == 0) or area.min() < 1 or words[:, :7].min() < 0 or np.any(words[:, 0] > area)):
        raise ValueError(f"{who}: needs increasing labels != 0 with area >= 1 and 0 <= pixels <= area")
    pixels, face, diag, blocks = words[:, 0], words[:, 1], words[:, 2], words[:, 3]
    table = {"label": label, "area": area, "skeleton_pixels": pixels,
             "skeleton_length": face.astype(np.float64) + np.sqrt(2.0) * diag.astype(np.float64),
             "skeleton_end_points": words[:, 4], "skeleton_branch_points": words[:, 5], "skeleton_isolated": words[:, 6],
             "skeleton_euler_number": pixels - face - diag + blocks}
    if _flag(radius, "radius", who):
        finite = words[:, 9] >= 0
        inf = np.full(n, np.inf)
        table["skeleton_radius_min"] = np.where(finite, np.sqrt(np.where(finite, words[:, 8], 0).astype(np.float64)), inf)
        table["skeleton_radius_max"] = np.where(finite, np.sqrt(np.where(finite, words[:, 9], 0).astype(np.float64)), inf)
        table["skeleton_dist_sq_mean"] = np.where(finite, words[:, 7].astype(np.float64) / np.maximum(pixels, 1), inf)
    return table


def _coordinates(table, name, index, shape):
    """adds ``name_z`` (3-D), ``name_y``, ``name_x`` of the raster indices ``index`` of a map of ``shape``; -1 where index < 0"""
    inside = index >= 0
    at = np.unravel_index(np.where(inside, index, 0), shape)
    for axis, v in zip("zyx"[-len(shape):], at):
        table[f"{name}_{axis}"] = np.where(inside, v, -1).astype(np.int64)
    return at


def branch_columns(rows, shape, radius=False):
    """The branch table of ``branch_graph`` from integers.  ``rows`` (n, 13): rows of ``clx_skeleton_graph``'s ``branches`` --
    first, label, kind, path_pixels, face_links, diag_links, pixel_a, pixel_b, node_a, node_b, d2_sum, d2_min, d2_max -- of a
    map of ``shape`` (2-D or 3-D).  Columns: the first ten words (int64), the coordinates ``first_y, first_x``, ``pixel_a_y,
    ..., pixel_b_x`` (with ``_z`` in front for a 3-D map; -1 for a cycle's pixels), ``length = face_links + sqrt(2) *
    diag_links``, ``euclidean``, the distance between pixel_a and pixel_b (NaN for a cycle), ``tortuosity = length /
    euclidean`` (NaN where the two coincide and for a cycle), float64; with ``radius`` ``radius_min`` and ``radius_max`` (the
    square roots of d2_min and d2_max) and ``dist_sq_mean`` (d2_sum / path_pixels), with ``inf`` in the three for a branch
    none of whose path pixels has a finite distance (``d2_max < 0``: a direct branch has none).  The rows are sorted by first.
    Host only."""
    who = "branch_columns"
    rows = np.asarray(rows).astype(np.int64).reshape(-1, len(BRANCH_WORDS))
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"{who}: shape must be 2 or 3 positive extents, got {shape!r}")
    npix = int(np.prod(shape, dtype=np.int64))
    cycle = rows[:, 2] == CYCLE
    if len(rows) and (rows[:, 0].min() < 0 or rows[:, 0].max() >= npix or rows[:, 6:10].max() >= npix or rows[:, 3:6].min() < 0
                      or np.any((rows[:, 6:10] < 0) != cycle[:, None]) or np.any(rows[:, 6] > rows[:, 7])):
        raise ValueError(f"{who}: needs rows of a map of {npix} pixels with pixel_a <= pixel_b, and -1 for a cycle's alone")
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    cycle = rows[:, 2] == CYCLE
    table = {name: rows[:, k] for k, name in enumerate(BRANCH_WORDS[:10])}
    _coordinates(table, "first", rows[:, 0], shape)
    a, b = (_coordinates(table, name, rows[:, k], shape) for name, k in (("pixel_a", 6), ("pixel_b", 7)))
    length = rows[:, 4].astype(np.float64) + np.sqrt(2.0) * rows[:, 5].astype(np.float64)
    euclidean = np.sqrt(sum(((u - v) ** 2 for u, v in zip(a, b)), np.zeros(len(rows), dtype=np.int64)).astype(np.float64))
    apart = ~cycle & (euclidean > 0)
    table["length"] = length
    table["euclidean"] = np.where(cycle, np.nan, euclidean)
    table["tortuosity"] = np.where(apart, length / np.where(apart, euclidean, 1.0), np.nan)
    if _flag(radius, "radius", who):
        finite = rows[:, 12] >= 0
        inf = np.full(len(rows), np.inf)
        table["radius_min"] = np.where(finite, np.sqrt(np.where(finite, rows[:, 11], 0).astype(np.float64)), inf)
        table["radius_max"] = np.where(finite, np.sqrt(np.where(finite, rows[:, 12], 0).astype(np.float64)), inf)
        table["dist_sq_mean"] = np.where(finite, rows[:, 10].astype(np.float64) / np.maximum(rows[:, 3], 1), inf)
    return table


def node_columns(rows, shape):
    """The node table of ``branch_graph``: the seven words of ``clx_skeleton_graph``'s ``nodes`` (first, label, kind, pixels,
    links_out, inner_face, inner_diag; int64) and ``first``'s coordinates as in ``branch_columns``, sorted by first.  Host
    only."""
    rows = np.asarray(rows).astype(np.int64).reshape(-1, len(NODE_WORDS))
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    table = {name: rows[:, k] for k, name in enumerate(NODE_WORDS)}
    _coordinates(table, "first", rows[:, 0], tuple(int(v) for v in shape))
    return table


def _sweep(adjacency, source):
    """heap Dijkstra -> (the farthest node reached from ``source``, its distance)"""
    dist, heap = {source: 0.0}, [(0.0, source)]
    far, reach = source, 0.0
    while heap:
        d, a = heapq.heappop(heap)
        if d > dist[a]:
            continue
        if d > reach:
            far, reach = a, d
        for b, w in adjacency[a]:
            if d + w < dist.get(b, math.inf):
                dist[b] = d + w
                heapq.heappush(heap, (d + w, b))
    return far, reach


def _longest_path(adjacency, members, tree):
    """the largest shortest path between two of the nodes ``members`` of one component: two sweeps where it is a tree (the
    farthest node from any node is an end of a longest path), a sweep from every node otherwise"""
    if tree:
        return _sweep(adjacency, _sweep(adjacency, members[0])[0])[1]
    return max(_sweep(adjacency, a)[1] for a in members)


def graph_columns(label, branches, nodes):
    """The per-label columns of ``skeleton_table(graph=True)`` from integers.  ``label`` (n): the labels, ascending;
    ``branches`` (b, 13) and ``nodes`` (m, 7): the rows of ``clx_skeleton_graph`` on the (thinned) map.  Columns, one row per
    label: ``skeleton_branches``, ``skeleton_junctions`` (nodes of kind 3), ``skeleton_cycles``, ``skeleton_spurs``,
    ``skeleton_components`` (of the graph: the 8-connected components of the label's pixels; a cycle is one of its own), int64;
    ``skeleton_branch_length_mean`` and ``skeleton_branch_length_max`` over the label's branches (0 without one) and
    ``skeleton_longest_path``, float64: the largest, over the pairs of nodes of one component, of the shortest path in the graph
    whose edges are the branches weighted by ``length``, nodes contracted to points; 0 for a label whose components have no
    nodes.  Host only: heap Dijkstra in plain Python."""
    who = "graph_columns"
    label = np.asarray(label).astype(np.int64).reshape(-1)
    branches = np.asarray(branches).astype(np.int64).reshape(-1, len(BRANCH_WORDS))
    nodes = np.asarray(nodes).astype(np.int64).reshape(-1, len(NODE_WORDS))
    # (the device appends its rows in any order: sorted by first, the float sums below are a function of the map)
    branches, nodes = (rows[np.argsort(rows[:, 0], kind="stable")] for rows in (branches, nodes))
    if len(label) and (np.any(np.diff(label) <= 0) or np.any(label == 0)):
        raise ValueError(f"{who}: needs increasing labels != 0")
    if not (np.isin(branches[:, 1], label).all() and np.isin(nodes[:, 1], label).all()):
        raise ValueError(f"{who}: a row carries a label that is not listed")
    n = len(label)
    row_of = {int(v): k for k, v in enumerate(label)}
    length = branches[:, 4].astype(np.float64) + np.sqrt(2.0) * branches[:, 5].astype(np.float64)
    cycle = branches[:, 2] == CYCLE
    at_b, at_n = (np.array([row_of[int(v)] for v in rows[:, 1]], dtype=np.int64) for rows in (branches, nodes))

    def count(at, mask):
        return np.bincount(at[mask], minlength=n).astype(np.int64)

    every = np.ones(len(branches), dtype=bool)
    total = np.bincount(at_b, weights=length, minlength=n)
    longest = np.zeros(n)
    np.maximum.at(longest, at_b, length)
    table = {"skeleton_branches": count(at_b, every), "skeleton_junctions": count(at_n, nodes[:, 2] == JUNCTION),
             "skeleton_cycles": count(at_b, cycle), "skeleton_spurs": count(at_b, branches[:, 2] == SPUR)}
    # the components of the contracted graph: nodes joined by the branches that are no cycles
    ids = {int(f): k for k, f in enumerate(nodes[:, 0])}
    if len(ids) != len(nodes):
        raise ValueError(f"{who}: two node rows have one id")
    adjacency = [[] for _ in nodes]
    for k in np.flatnonzero(~cycle):
        a, b = ids.get(int(branches[k, 8])), ids.get(int(branches[k, 9]))
        if a is None or b is None:
            raise ValueError(f"{who}: a branch ends on a node that has no row")
        adjacency[a].append((b, float(length[k])))
        adjacency[b].append((a, float(length[k])))
    component = np.full(len(nodes), -1, dtype=np.int64)
    components, path = count(at_b, cycle), np.zeros(n)
    for start in range(len(nodes)):
        if component[start] >= 0:
            continue
        component[start] = start
        members, stack = [], [start]
        while stack:
            a = stack.pop()
            members.append(a)
            for b, _ in adjacency[a]:
                if component[b] < 0:
                    component[b] = start
                    stack.append(b)
        edges = sum(len(adjacency[a]) for a in members) // 2
        row = at_n[start]
        components[row] += 1
        path[row] = max(path[row], _longest_path(adjacency, members, edges == len(members) - 1))
    has = table["skeleton_branches"] > 0
    table["skeleton_components"] = components
    table["skeleton_branch_length_mean"] = np.where(has, total / np.maximum(table["skeleton_branches"], 1), 0.0)
    table["skeleton_branch_length_max"] = longest
    table["skeleton_longest_path"] = path
    return table


def _graph_call(scene, lab, dist, limit_q10, rows, want_map, want_out):
    """clx_skeleton_graph on ``lab`` (flat int32 on the device, the scene's shape), once, or twice where the rows asked for
    (``rows``) did not fit the first call's capacity -> (branches int64 (b, 13), nodes int64 (m, 7), both on the host and
    unsorted, branch_map and out as flat int32 device tensors or None, info as a list)"""
    npix = lab.numel()
    workspace, nbytes = _workspace(scene, "clx_skeleton_graph_workspace", scene.nd, scene.Z, scene.Y, scene.X, below="2^31")
    branch_map = torch.empty(npix, dtype=torch.int32, device=scene.device) if want_map else None
    out = torch.empty(npix, dtype=torch.int32, device=scene.device) if want_out else None
    info = torch.empty(6, dtype=torch.int32, device=scene.device)
    capacity_b = capacity_n = GRAPH_CAPACITY if rows else 0
    while True:
        branches = torch.empty((capacity_b, len(BRANCH_WORDS)), dtype=torch.int64, device=scene.device) if rows else None
        nodes = torch.empty((capacity_n, len(NODE_WORDS)), dtype=torch.int64, device=scene.device) if rows else None
        _clx.call("clx_skeleton_graph", _clx.ptr(lab), _clx.ptr(dist), scene.nd, scene.Z, scene.Y, scene.X, limit_q10, capacity_b, capacity_n,
                  _clx.ptr(branch_map), _clx.ptr(out), _clx.ptr(branches), _clx.ptr(nodes), _clx.ptr(info), _clx.ptr(workspace), nbytes,
                  _clx.stream_ptr(scene.device))
        found = info.tolist()
        if not rows:
            return None, None, branch_map, out, found
        if found[0] <= capacity_b and found[1] <= capacity_n:
            return branches[:found[0]].cpu().numpy(), nodes[:found[1]].cpu().numpy(), branch_map, out, found
        capacity_b, capacity_n = found[0], found[1]          # the counts are complete whatever the capacity: the second call fits


def branch_graph(labels, planewise=False, radius=False, device=None):
    """The branch graph of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as
    ``region_table``; thinned, by ``thin_labels`` say, or not: the definitions need no thinning) -> a dict: ``branches``, the
    ``branch_columns``, and ``nodes``, the ``node_columns``, both sorted by first, and ``branch_map``, int32 in the type and on the
    device of ``labels``: first + 1 of its branch on a path pixel,
    -(node id + 1) on a node pixel, 0 on background.  A 3-D map needs ``planewise=True``: every slice is a map of its own.  With
    ``radius`` the distance map is ``label_distance_sq`` of THIS map (of every slice on its own when planewise).  The module's
    docstring has the definitions.  Runs on a HIP device; there is no CPU path."""
    who = "branch_graph"
    _check_map(labels, who)
    _planewise(planewise, labels.ndim, who, REFUSE_3D_GRAPH)
    radius = _flag(radius, "radius", who)
    scene = _scene(labels, device, who)
    if scene.lab.numel() == 0:
        branches, nodes = np.zeros((0, len(BRANCH_WORDS)), np.int64), np.zeros((0, len(NODE_WORDS)), np.int64)
        branch_map = torch.zeros(0, dtype=torch.int32, device=scene.device)
    else:
        dist = _distance_slices(scene) if radius and scene.nid > 1 else None
        branches, nodes, branch_map, _, _ = _graph_call(scene, scene.lab, dist, 0, True, True, False)
    branch_map = branch_map.reshape(scene.spatial)
    if torch.is_tensor(labels):
        branch_map = branch_map.to(labels.device)
    else:
        branch_map = branch_map.cpu().numpy()
    shape = scene.spatial if scene.lab.numel() else tuple(max(v, 1) for v in scene.spatial)
    return {"branches": branch_columns(branches, shape, radius), "nodes": node_columns(nodes, shape), "branch_map": branch_map}


def prune_spurs(labels, min_length, rounds=1, planewise=False, device=None):
    """``labels`` (``branch_graph``'s arguments; a thinned map, usually) with its short spurs removed.  A spur -- a branch
    between an end pixel and a junction -- is pruned iff its ``length = face_links + sqrt(2) * diag_links`` is below
    ``ceil(min_length * 1024) / 1024``: ``min_length`` is rounded UP to a multiple of 1/1024 pixel, the unit in which the
    library compares, exactly, in integers; ``min_length=0`` prunes nothing.  The spur's path pixels and its end pixel are set to
    0 and the junction stays; end-end branches and cycles are never pruned.  A ROUND decides all spurs from one state of the
    map; after it a junction may have become a path pixel and two branches one, so ``rounds`` (an integer >= 1) rounds are made,
    or fewer where a round prunes nothing.  The result has the type, dtype and device of ``labels``.  Runs on a HIP device;
    there is no CPU path."""
    who = "prune_spurs"
    limit = _limit_q10(min_length, who)
    if isinstance(rounds, bool) or not isinstance(rounds, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: rounds must be an integer, got {type(rounds).__name__}")
    if not 1 <= int(rounds) < 1 << 31:
        raise ValueError(f"{who}: rounds must lie in [1, 2^31), got {rounds!r}")
    _check_map(labels, who)
    _planewise(planewise, labels.ndim, who, REFUSE_3D_GRAPH)
    scene = _scene(labels, device, who)
    return _in_type_of(labels, scene, _prune(scene, scene.lab, limit, int(rounds)))


def _prune(scene, lab, limit_q10, rounds):
    """up to ``rounds`` clx_skeleton_graph calls with ``limit_q10``, each on the map the one before left -> the pruned map, flat
    int32 on the device; None where nothing was pruned (no call for an empty map or a limit of 0)"""
    if lab.numel() == 0 or limit_q10 == 0:
        return None
    out = None
    for _ in range(rounds):
        _, _, _, pruned, info = _graph_call(scene, lab if out is None else out, None, limit_q10, False, False, True)
        if info[3] == 0:
            break
        out = pruned
    return out


def _thin_map(scene, max_iter):
    """clx_label_thin calls, the first with resume = 0, until an iteration deletes nothing or ``max_iter`` iterations have run
    -> the thinned map, flat int32 on the device; None for a map the library was not called for"""
    npix = scene.lab.numel()
    if npix == 0 or max_iter == 0:
        return None
    workspace, nbytes = _workspace(scene, "clx_label_thin_workspace", scene.nd, scene.Z, scene.Y, scene.X, below="2^31")
    out = torch.empty(npix, dtype=torch.int32, device=scene.device)
    info = torch.empty(3, dtype=torch.int32, device=scene.device)
    done = 0
    while True:
        iterations = CALL_ITERATIONS if max_iter is None else min(CALL_ITERATIONS, max_iter - done)
        _clx.call("clx_label_thin", _clx.ptr(scene.lab), scene.nd, scene.Z, scene.Y, scene.X, iterations, int(done > 0), _clx.ptr(out),
                  _clx.ptr(info), _clx.ptr(workspace), nbytes, _clx.stream_ptr(scene.device))
        done += iterations
        if info.tolist()[1] == 0 or (max_iter is not None and done >= max_iter):
            return out


def _distance_slices(scene):
    """``label_distance_sq`` of the scene's map with the default edge convention, every slice on its own -> flat int32 on the
    device"""
    if scene.nd == 2:
        return _distance_map(scene, False)
    plane = scene.Y * scene.X
    return torch.cat([_distance_map(_Scene(scene.who, scene.lab[z * plane:(z + 1) * plane], scene.device, 2, scene.spatial[1:], scene.nid),
                                    False) for z in range(scene.Z)])


def _skeleton(labels, max_iter, planewise, radius, device, who, table=False, graph=False, prune=None):
    """-> (scene, the thinned map -- with ``prune`` after one round of pruning -- as a flat int32 device tensor or None for a map
    that came through unchanged, with ``table`` the ``skeleton_columns`` of it -- with ``graph`` and the ``graph_columns`` --, and
    with ``table`` and ``graph`` the ``branch_columns`` of it)"""
    max_iter = _max_iter(max_iter, who)
    _check_map(labels, who)
    _planewise(planewise, labels.ndim, who)
    radius = _flag(radius, "radius", who)
    graph = _flag(graph, "graph", who)
    limit = 0 if prune is None else _limit_q10(prune, who, "prune")
    scene = _scene(labels, device, who)
    out = _thin_map(scene, max_iter)
    if limit:
        pruned = _prune(scene, scene.lab if out is None else out, limit, 1)
        out = out if pruned is None else pruned
    if not table:
        return scene, out, None, None
    scene.measured()
    shape = scene.spatial if scene.lab.numel() else tuple(max(v, 1) for v in scene.spatial)
    if scene.empty:
        none = np.zeros(0, dtype=np.int64)
        columns = skeleton_columns(none, none, np.zeros((0, CENSUS_WORDS), dtype=np.int64), radius)
        if graph:
            columns.update(graph_columns(none, none, none))
        return scene, out, columns, branch_columns(none, shape, radius) if graph else None
    words = scene.ids(CENSUS_WORDS)
    skeleton = scene.lab if out is None else out
    dist = _distance_slices(scene) if radius else None
    # (bit 1, a pixel without a finite distance, is no error: skeleton_columns reports inf)
    scene.call("clx_skeleton_census", {1: LABELS_OUT_OF_RANGE}, skeleton, dist, scene.nd, scene.Z, scene.Y, scene.X, scene.nid, words, FLAGS)
    present = scene.present
    columns = skeleton_columns(present, scene.area[present], words.cpu().numpy()[present], radius)
    if not graph:
        return scene, out, columns, None
    branches, nodes, _, _, _ = _graph_call(scene, skeleton, dist, 0, True, False, False)
    columns.update(graph_columns(present, branches, nodes))
    return scene, out, columns, branch_columns(branches, shape, radius)


def thin_labels(labels, max_iter=None, planewise=False, device=None):
    """``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as ``region_table``) with every object
    thinned to its centre lines: the state after the first iteration that deletes nothing, or after ``max_iter`` iterations (an
    integer >= 0, or None: to the end; 0 changes nothing).  A 3-D map needs ``planewise=True``: every slice is thinned as a 2-D
    map of its own.  Objects that touch thin independently.  The result has the type, dtype and device of ``labels``.  The
    module's docstring has the definitions.  A function of the map alone: the same bits in every run.  Runs on a HIP device;
    there is no CPU path."""
    scene, out, _, _ = _skeleton(labels, max_iter, planewise, False, device, "thin_labels")
    return _in_type_of(labels, scene, out)


def skeleton_table(labels, max_iter=None, planewise=False, radius=False, device=None, graph=False, prune=None):
    """The skeleton of every object of ``labels`` (``thin_labels``' arguments) measured, one row per label present:
    ``skeleton_columns`` lists the columns.  ``area`` is ``clx_region_moments`` of the input map.  With ``radius`` the distance
    map is ``label_distance_sq`` of the INPUT map (of every slice on its own when planewise) with the edge convention
    ``region_table(inscribed=True)`` has by default.  With ``prune`` (a length in pixels, ``prune_spurs``' ``min_length``) the
    thinned map loses its spurs shorter than that, in one round, before it is measured.  With ``graph`` the ``graph_columns``
    of the (pruned) skeleton's branch graph follow.  A map without objects gives an empty table with these columns.  Runs on a
    HIP device; there is no CPU path."""
    return _skeleton(labels, max_iter, planewise, radius, device, "skeleton_table", table=True, graph=graph, prune=prune)[2]


def skeleton_stage(inference_config, source, output, max_iter=None, planewise=False, radius=False, graph=False, prune=None) -> None:
    """For every sample and bandwidth of ``source``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (``segment()``'s, say): ``thin_labels(labels, max_iter, planewise)`` -- with
    ``prune`` after one round of ``prune_spurs(..., prune)`` -- into a new uint16 dataset ``output`` of that container and
    ``skeleton_table``'s rows of all samples as ``skeleton_bandwidth-<b>.csv`` in the working directory -- a header line, then
    ``sample`` and the table's columns, floats as ``%.17g``.  With ``graph`` the table has the ``graph_columns`` and a second
    file, ``skeleton_branches_bandwidth-<b>.csv``, has ``sample`` and the ``branch_columns``, one row per branch.  Rank 0 works
    alone under torch.distributed."""
    who = "skeleton_stage"
    if not isinstance(source, str) or not source:
        raise ValueError(f"{who}: source must be the name of a dataset, got {source!r}")
    if not isinstance(output, str) or not output or output == source:
        raise ValueError(f"{who}: output must name a new dataset other than source, got {output!r}")
    _max_iter(max_iter, who)
    _flag(planewise, "planewise", who)
    _flag(radius, "radius", who)
    _flag(graph, "graph", who)
    if prune is not None:
        _limit_q10(prune, who, "prune")
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    _planewise(planewise, stage.nd, who)
    stage.open("a", source)
    stage.refuse_existing(output)
    ds_source, ds_output = stage.f[source], stage.create(output)

    def per_sample(sample, bandwidth):
        labels = ds_source[sample, bandwidth].astype(np.int32)
        scene, out, table, branches = _skeleton(labels, max_iter, planewise, radius, stage.device, who, table=True, graph=graph, prune=prune)
        ds_output[sample, bandwidth] = _in_type_of(labels, scene, out).astype(np.uint16)
        return (table, branches) if graph else (table,)

    stage.run(per_sample, ("skeleton", "skeleton_branches") if graph else ("skeleton",))


if __name__ == "__main__":
    from .cli import skeleton as _command

    _command()
