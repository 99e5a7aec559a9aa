"""The branch graph of the skeleton stage (include/clx.h, clx_skeleton_graph) restated in NumPy on whole maps: the reference
of tests/test_cpu_skeleton_graph.py, tests/test_gpu_skeleton_graph.py and tests/test_gpu_skeleton_graph_stage.py.  No device,
no cellulus_amd.

Links and degree are the census's (tests/skeleton_ref.py).  A PATH pixel has degree 2, an END pixel degree 1, a JUNCTION pixel
degree >= 3, an ISOLATED pixel degree 0.  A NODE is a maximal set of junction pixels connected by links between two junction
pixels (kind 3), an end pixel alone (kind 1) or an isolated pixel alone (kind 0); its id is its smallest raster index.  A BRANCH
is (a) a maximal set of path pixels connected by links between two path pixels, with every link from one of them to a pixel
that is no path pixel (a terminal link), `first` its smallest path pixel, or (b) a DIRECT branch, a single link between an end
pixel and a junction pixel or between two end pixels, `first` the end pixel (the smaller of two).  Links between two junction
pixels belong to their node.  A branch of kind (a) has two terminal links or none (a CYCLE).  Branch kinds: 0 end-end, 1
end-junction (a SPUR), 2 junction-junction, 3 cycle."""

import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from skeleton_ref import DIST_INF, _slices, shifted

ISOLATED, END, PATH, JUNCTION = 0, 1, 2, 3
END_END, SPUR, JUNCTION_JUNCTION, CYCLE = 0, 1, 2, 3
BRANCH_WORDS = ("first", "label", "kind", "path_pixels", "face_links", "diag_links", "pixel_a", "pixel_b", "node_a", "node_b",
                "d2_sum", "d2_min", "d2_max")
NODE_WORDS = ("first", "label", "kind", "pixels", "links_out", "inner_face", "inner_diag")
SQRT2 = math.sqrt(2.0)


def pixel_graph(labels):
    """-> (the flat map as int64, the kind of every pixel (-1: background), the links as arrays i, j, face: every link once,
    i the pixel that has it towards E, S, SE or SW)"""
    lab = _slices(labels).astype(np.int64)
    X = lab.shape[2]
    obj = lab != 0

    def same(dy, dx):
        return obj & (shifted(lab, dy, dx) == lab)

    e, s, w, n = same(0, 1), same(1, 0), same(0, -1), same(-1, 0)
    se, sw, nw, ne = same(1, 1) & ~s & ~e, same(1, -1) & ~s & ~w, same(-1, -1) & ~n & ~w, same(-1, 1) & ~n & ~e
    degree = sum(v.astype(np.int64) for v in (e, s, w, n, se, sw, nw, ne))
    kind = np.where(obj, np.minimum(degree, JUNCTION), -1).ravel()
    index = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    i = [index[m] for m in (e, s, se, sw)]
    j = [i[0] + 1, i[1] + X, i[2] + X + 1, i[3] + X - 1]
    face = [np.full(len(v), k < 2) for k, v in enumerate(i)]
    return lab.ravel(), kind, np.concatenate(i), np.concatenate(j), np.concatenate(face)


def _roots(n, i, j):
    """the smallest pixel of every pixel's component under the links (i, j)"""
    comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)), directed=False)[1]
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n, dtype=np.int64))
    return smallest[comp]


def prune_q10(min_length):
    """the limit of ``prune_spurs``: the smallest multiple of 1/1024 that is >= min_length"""
    return math.ceil(min_length * 1024)


def spur_pruned(face, diag, limit_q10):
    """face + sqrt(2) diag < limit_q10 / 1024 in Python integers"""
    F, D, T = 1024 * int(face), 1024 * int(diag), int(limit_q10)
    if F >= T or D >= T:
        return False
    return 2 * D * D < (T - F) * (T - F)


def graph(labels, dist_sq=None, limit_q10=0):
    """-> dict: ``branches`` int64 (n, 13) and ``nodes`` int64 (m, 7), both sorted by first; ``branch_map`` and ``out`` in the
    shape of ``labels``, int32; ``info`` (6 integers); ``terminals``: the terminal links of every branch of kind (a), in the
    order of the rows of that kind."""
    labels = np.asarray(labels)
    lab, kind, li, lj, lface = pixel_graph(labels)
    n = lab.size
    both = lambda k: (kind[li] == k) & (kind[lj] == k)
    root = np.arange(n, dtype=np.int64)
    for k in (PATH, JUNCTION):
        m = both(k)
        r = _roots(n, li[m], lj[m])
        root = np.where(kind == k, r, root)

    def node_of(p):
        return int(root[p])                              # an end or isolated pixel is its own root

    branch = {int(r): {"pixels": 0, "face": 0, "diag": 0, "ends": [], "d2": []} for r in np.unique(root[kind == PATH])}
    node = {int(r): {"kind": int(kind[r]), "pixels": 0, "out": 0, "face": 0, "diag": 0} for r in np.unique(root[(kind >= 0) & (kind != PATH)])}
    for p in np.flatnonzero(kind == PATH):
        branch[int(root[p])]["pixels"] += 1
    for p in np.flatnonzero((kind >= 0) & (kind != PATH)):
        node[int(root[p])]["pixels"] += 1
    direct = []
    for a, b, face in zip(li.tolist(), lj.tolist(), lface.tolist()):
        ka, kb = int(kind[a]), int(kind[b])
        word = "face" if face else "diag"
        if ka == PATH and kb == PATH:
            assert root[a] == root[b]
            branch[int(root[a])][word] += 1
        elif ka == PATH or kb == PATH:
            p, q = (a, b) if ka == PATH else (b, a)
            branch[int(root[p])][word] += 1
            branch[int(root[p])]["ends"].append(q)
            node[node_of(q)]["out"] += 1
        elif ka == JUNCTION and kb == JUNCTION:
            assert root[a] == root[b]
            node[int(root[a])][word] += 1
        else:                                            # end - junction or end - end: a direct branch
            assert END in (ka, kb) and ISOLATED not in (ka, kb)
            first = min(p for p, k in ((a, ka), (b, kb)) if k == END)
            direct.append((first, a, b, face))
            node[node_of(a)]["out"] += 1
            node[node_of(b)]["out"] += 1

    bad = 0
    if dist_sq is not None:
        d = np.asarray(dist_sq).astype(np.int64).ravel()
        for p in np.flatnonzero(kind == PATH):
            if 0 <= d[p] < DIST_INF:
                branch[int(root[p])]["d2"].append(int(d[p]))
            else:
                bad |= 2

    rows, terminals, pruned = [], [], {}
    for first, b in branch.items():
        ends = sorted(b["ends"])
        terminals.append(len(ends))
        if len(ends) == 2:
            k = {2: END_END, 1: SPUR, 0: JUNCTION_JUNCTION}[sum(int(kind[q] == END) for q in ends)]
            a = ends + [node_of(q) for q in ends]
        else:
            k, a = CYCLE, [-1, -1, -1, -1]
        d2 = b["d2"]
        rows.append([first, int(lab[first]), k, b["pixels"], b["face"], b["diag"], *a, sum(d2), min(d2, default=DIST_INF), max(d2, default=-1)])
        pruned[first] = k == SPUR and spur_pruned(b["face"], b["diag"], limit_q10)
    for first, a, b, face in direct:
        k = END_END if kind[a] == END and kind[b] == END else SPUR
        lo, hi = min(a, b), max(a, b)
        rows.append([first, int(lab[first]), k, 0, int(face), int(not face), lo, hi, node_of(lo), node_of(hi), 0, DIST_INF, -1])
        pruned[first] = k == SPUR and spur_pruned(int(face), int(not face), limit_q10)
    branches = np.array(sorted(rows), dtype=np.int64).reshape(-1, 13)
    nodes = np.array(sorted([first, int(lab[first]), v["kind"], v["pixels"], v["out"], v["face"], v["diag"]] for first, v in node.items()),
                     dtype=np.int64).reshape(-1, 7)

    branch_map = np.where(kind == PATH, root + 1, np.where(kind >= 0, -(root + 1), 0))
    out = lab.copy()
    pixels = spurs = 0
    for row in branches:
        if pruned[int(row[0])]:
            end = row[6] if kind[row[6]] == END else row[7]
            gone = (branch_map == row[0] + 1) if row[3] else np.zeros(n, bool)
            gone[end] = True
            out[gone] = 0
            pixels += int(gone.sum())
            spurs += 1
    return {"branches": branches, "nodes": nodes, "branch_map": branch_map.astype(np.int32).reshape(labels.shape),
            "out": out.astype(np.int32).reshape(labels.shape), "info": [len(branches), len(nodes), pixels, spurs, bad, 0],
            "terminals": terminals}


def lengths(branches):
    return branches[:, 4].astype(np.float64) + SQRT2 * branches[:, 5].astype(np.float64)


def components(branches, nodes):
    """-> (the component of every node row, of every branch row, the number of components) of the contracted graph: a cycle is
    a component of its own"""
    ids = {int(f): k for k, f in enumerate(nodes[:, 0])}
    parent = list(range(len(nodes)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for row in branches:
        if row[2] != CYCLE:
            a, b = find(ids[int(row[8])]), find(ids[int(row[9])])
            parent[max(a, b)] = min(a, b)
    of_node = [find(k) for k in range(len(nodes))]
    cycles = iter(range(len(nodes), len(nodes) + len(branches)))
    of_branch = [next(cycles) if row[2] == CYCLE else of_node[ids[int(row[8])]] for row in branches]
    return of_node, of_branch, len(set(of_node)) + int((branches[:, 2] == CYCLE).sum())


def longest_path_brute(branches, nodes):
    """the largest, over the pairs of nodes of one component, of the shortest path along the branches weighted by length:
    Floyd-Warshall on the whole graph"""
    m = len(nodes)
    if m == 0:
        return 0.0
    ids = {int(f): k for k, f in enumerate(nodes[:, 0])}
    dist = np.full((m, m), np.inf)
    dist[np.arange(m), np.arange(m)] = 0.0
    for row, length in zip(branches, lengths(branches)):
        if row[2] != CYCLE:
            a, b = ids[int(row[8])], ids[int(row[9])]
            dist[a, b] = dist[b, a] = min(dist[a, b], length)
    for k in range(m):
        dist = np.minimum(dist, dist[:, k:k + 1] + dist[k:k + 1, :])
    return float(dist[np.isfinite(dist)].max())


def summary(branches, nodes):
    """-> {label: dict of the graph_columns' values}, the longest path by brute force"""
    out = {}
    for label in sorted(set(branches[:, 1].tolist()) | set(nodes[:, 1].tolist())):
        b, v = branches[branches[:, 1] == label], nodes[nodes[:, 1] == label]
        length = lengths(b)
        out[int(label)] = {"skeleton_branches": len(b), "skeleton_junctions": int((v[:, 2] == JUNCTION).sum()),
                           "skeleton_cycles": int((b[:, 2] == CYCLE).sum()), "skeleton_spurs": int((b[:, 2] == SPUR).sum()),
                           "skeleton_components": components(b, v)[2],
                           "skeleton_branch_length_mean": float(length.mean()) if len(b) else 0.0,
                           "skeleton_branch_length_max": float(length.max()) if len(b) else 0.0,
                           "skeleton_longest_path": longest_path_brute(b, v)}
    return out
