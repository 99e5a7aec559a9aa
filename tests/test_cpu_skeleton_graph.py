"""CPU tier of the skeleton stage's branch graph: the restatement of the definitions (tests/skeleton_graph_ref.py) against
maps worked by hand, against the census of tests/skeleton_ref.py (every link and every pixel lies in exactly one branch or
node) and against scipy.ndimage.label on thinned noise; graph_columns against a brute-force longest path; branch_columns by
hand; the prune rule against integer square roots; the refusals that need no device; the declarations in include/clx.h."""

import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy import ndimage

import skeleton_graph_ref as gref
from skeleton_graph_ref import CYCLE, END_END, JUNCTION, JUNCTION_JUNCTION, SPUR, graph, spur_pruned, summary
from skeleton_ref import DIST_INF, census, noise_map, skeleton

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT2 = math.sqrt(2.0)
_NOISE = {}


def grid(text, label=1):
    return np.array([[label if c == "#" else 0 for c in line] for line in text.split()], np.int32)


BAR = grid("""......
              .####.
              ......""")
TEE = grid(""".......
              .#####.
              ...#...
              ...#...
              ...#...""")
WYE = grid("""#...#
              .#.#.
              ..#..
              ..#..
              ..#..""")
RING = grid(""".###.
               .#.#.
               .###.""")
RING_WITH_TAIL = grid(""".###...
                         .#.###.
                         .###...""")
BLOCK = grid("""....
                .##.
                .##.
                ....""", 5)
PLUS = grid(""".#.
               ###
               .#.""")


def noise(seed):
    """the graph of a thinned noise map, computed once per seed and left unchanged -> (the thinned map, graph())"""
    if seed not in _NOISE:
        skel = skeleton(noise_map((60, 75), seed, block=13, sigma=1.5))
        _NOISE[seed] = skel, graph(skel)
    return _NOISE[seed]


def rows(result):
    return result["branches"][:, :10].tolist(), result["nodes"].tolist()


def end(p, label=1):
    return [p, label, 1, 1, 1, 0, 0]


def test_maps_worked_by_hand():
    assert rows(graph(BAR)) == ([[8, 1, END_END, 2, 3, 0, 7, 10, 7, 10]], [end(7), end(10)])
    assert graph(BAR)["branch_map"].tolist() == [[0] * 6, [0, -8, 9, 9, -11, 0], [0] * 6]
    assert rows(graph(TEE)) == ([[9, 1, SPUR, 1, 2, 0, 8, 10, 8, 10], [11, 1, SPUR, 1, 2, 0, 10, 12, 10, 12], [17, 1, SPUR, 2, 3, 0, 10, 31, 10, 31]],
                                [end(8), [10, 1, JUNCTION, 1, 3, 0, 0], end(12), end(31)])
    assert rows(graph(WYE)) == ([[6, 1, SPUR, 1, 0, 2, 0, 12, 0, 12], [8, 1, SPUR, 1, 0, 2, 4, 12, 4, 12], [17, 1, SPUR, 1, 2, 0, 12, 22, 12, 22]],
                                [end(0), end(4), [12, 1, JUNCTION, 1, 3, 0, 0], end(22)])
    assert rows(graph(RING)) == ([[1, 1, CYCLE, 8, 8, 0, -1, -1, -1, -1]], [])
    # the ring's pixel (1, 3) has the tail as its third link: the ring is a branch with both ends on that node
    assert rows(graph(RING_WITH_TAIL)) == ([[1, 1, JUNCTION_JUNCTION, 7, 8, 0, 10, 10, 10, 10], [11, 1, SPUR, 1, 2, 0, 10, 12, 10, 12]],
                                           [[10, 1, JUNCTION, 1, 3, 0, 0], end(12)])
    # a full 2 x 2 block: every pixel has two face links and no diagonal one, a cycle of 4 pixels
    assert rows(graph(BLOCK)) == ([[5, 5, CYCLE, 4, 4, 0, -1, -1, -1, -1]], [])
    assert graph(BLOCK)["branch_map"][1:3, 1:3].tolist() == [[6, 6], [6, 6]]
    # the plus: four direct branches, first = the end pixel
    assert rows(graph(PLUS)) == ([[1, 1, SPUR, 0, 1, 0, 1, 4, 1, 4], [3, 1, SPUR, 0, 1, 0, 3, 4, 3, 4], [5, 1, SPUR, 0, 1, 0, 4, 5, 4, 5],
                                  [7, 1, SPUR, 0, 1, 0, 4, 7, 4, 7]], [end(1), end(3), [4, 1, JUNCTION, 1, 4, 0, 0], end(5), end(7)])
    assert rows(graph(np.array([[3, 3]], np.int32))) == ([[0, 3, END_END, 0, 1, 0, 0, 1, 0, 1]], [end(0, 3), end(1, 3)])
    assert rows(graph(np.array([[3, 0], [0, 3]], np.int32))) == ([[0, 3, END_END, 0, 0, 1, 0, 3, 0, 3]], [end(0, 3), end(3, 3)])
    assert rows(graph(np.array([[0, 0], [0, -7]], np.int32))) == ([], [[3, -7, 0, 1, 0, 0, 0]])
    assert rows(graph(np.zeros((2, 3), np.int32))) == ([], [])
    for r in (graph(m) for m in (BAR, TEE, WYE, RING, RING_WITH_TAIL, BLOCK, PLUS)):
        assert r["info"] == [len(r["branches"]), len(r["nodes"]), 0, 0, 0, 0] and (r["branches"][:, 10:] == [0, DIST_INF, -1]).all()


def test_a_cluster_of_junction_pixels_by_hand():
    steps = grid("""..#...
                    ######
                    ...#..""")
    # (1, 2) and (1, 3) have degree 3 and a face link between them: one node of two pixels with four links out
    branches, nodes = rows(graph(steps))
    assert nodes == [end(2), end(6), [8, 1, JUNCTION, 2, 4, 1, 0], end(11), end(15)]
    assert branches == [[2, 1, SPUR, 0, 1, 0, 2, 8, 2, 8], [7, 1, SPUR, 1, 2, 0, 6, 8, 6, 8], [10, 1, SPUR, 1, 2, 0, 9, 11, 8, 11],
                        [15, 1, SPUR, 0, 1, 0, 9, 15, 8, 15]]
    assert graph(steps)["branch_map"].tolist() == [[0, 0, -3, 0, 0, 0], [-7, 8, -9, -9, 11, -12], [0, 0, 0, -16, 0, 0]]
    assert sum(b[4] + b[5] for b in branches) + 1 == int(census(steps)[0][1, 1:3].sum())


def test_touching_labels_in_both_orders():
    for lo, hi in ((1, 2), (2, 1), (-3, 2 ** 31 - 1)):
        labels = np.zeros((4, 7), np.int32)
        labels[1, 1:6], labels[2, 1:6] = lo, hi
        branches, nodes = rows(graph(labels))
        assert branches == [[9, lo, END_END, 3, 4, 0, 8, 12, 8, 12], [16, hi, END_END, 3, 4, 0, 15, 19, 15, 19]]
        assert nodes == [end(8, lo), end(12, lo), end(15, hi), end(19, hi)]
        for label in (lo, hi):
            alone = graph(np.where(labels == label, label, 0).astype(np.int32))
            assert [b for b in branches if b[1] == label] == rows(alone)[0]


def test_3d_is_slice_by_slice_and_rows_do_not_wrap():
    stack = np.zeros((2, 4, 4), np.int32)
    stack[0, 3, :], stack[1, 0, :] = 1, 1                 # the last row of a slice and the first of the next
    stack[0, 0, 3], stack[0, 1, 0] = 1, 1                 # the end of a row and the start of the next
    r = graph(stack)
    assert rows(r)[0] == [[13, 1, END_END, 2, 3, 0, 12, 15, 12, 15], [17, 1, END_END, 2, 3, 0, 16, 19, 16, 19]]
    assert [n[:3] for n in rows(r)[1]] == [[3, 1, 0], [4, 1, 0], [12, 1, 1], [15, 1, 1], [16, 1, 1], [19, 1, 1]]
    for z in range(2):
        m = r["branch_map"][z]
        assert np.array_equal(graph(stack[z])["branch_map"], m - 16 * z * np.sign(m))


def test_noise_maps_conserve_links_and_pixels_and_cover_every_case():
    kinds, direct, clusters, loops, isolated = set(), 0, 0, 0, 0
    for seed in range(12):
        skel, r = noise(seed)
        b, v = r["branches"], r["nodes"]
        assert set(r["terminals"]) <= {0, 2}
        words = census(skel)[0]
        for label in range(1, len(words)):
            bl, vl = b[b[:, 1] == label], v[v[:, 1] == label]
            assert bl[:, 4].sum() + vl[:, 5].sum() == words[label, 1] and bl[:, 5].sum() + vl[:, 6].sum() == words[label, 2]
            assert bl[:, 3].sum() + vl[:, 3].sum() == words[label, 0]
            assert (vl[:, 2] == 1).sum() == words[label, 4] and (vl[:, 2] == 0).sum() == words[label, 6]
            assert vl[vl[:, 2] == JUNCTION, 3].sum() == words[label, 5]
            assert gref.components(bl, vl)[2] == ndimage.label(skel == label, np.ones((3, 3), int))[1]
        # a terminal of a branch is a link out of a node
        assert v[:, 4].sum() == 2 * (b[:, 2] != CYCLE).sum()
        assert np.array_equal(r["branch_map"] > 0, np.isin(r["branch_map"] - 1, b[:, 0]) & (skel != 0))
        assert np.array_equal(r["out"], skel)
        kinds |= set(b[:, 2].tolist())
        direct += int((b[:, 3] == 0).sum())
        clusters += int((v[:, 3] > 1).sum())
        loops += int(((b[:, 2] == JUNCTION_JUNCTION) & (b[:, 8] == b[:, 9])).sum())
        isolated += int((v[:, 2] == 0).sum())
    assert kinds == {END_END, SPUR, JUNCTION_JUNCTION, CYCLE} and direct > 100 and clusters > 10 and loops >= 5 and isolated > 30


def test_unthinned_maps_conserve_too():
    for seed in range(3):
        labels = noise_map((40, 52), seed, block=13, sigma=1.5)
        r = graph(labels)
        assert set(r["terminals"]) <= {0, 2}
        words = census(labels)[0]
        for label in range(1, len(words)):
            bl, vl = r["branches"][r["branches"][:, 1] == label], r["nodes"][r["nodes"][:, 1] == label]
            assert bl[:, 4].sum() + vl[:, 5].sum() == words[label, 1] and bl[:, 5].sum() + vl[:, 6].sum() == words[label, 2]
            assert bl[:, 3].sum() + vl[:, 3].sum() == words[label, 0]
            assert gref.components(bl, vl)[2] == ndimage.label(labels == label, np.ones((3, 3), int))[1]


def test_dist_sq_words():
    dist = np.arange(TEE.size, dtype=np.int64).reshape(TEE.shape)
    r = graph(TEE, dist)
    assert r["branches"][:, 10:].tolist() == [[9, 9, 9], [11, 11, 11], [17 + 24, 17, 24]] and r["info"][4] == 0
    dist[2, 3], dist[1, 2] = -1, DIST_INF
    r = graph(TEE, dist)
    assert r["branches"][:, 10:].tolist() == [[0, DIST_INF, -1], [11, 11, 11], [24, 24, 24]] and r["info"][4] == 2
    dist[1, 1] = dist[1, 3] = -5                          # under an end and a junction pixel: not looked at
    assert graph(TEE, dist)["info"][4] == 2 and graph(BAR, np.full(BAR.shape, -1))["info"][4] == 2
    assert graph(PLUS, np.full(PLUS.shape, -1))["info"][4] == 0


def test_graph_columns_by_hand_and_against_brute_force(monkeypatch):
    from cellulus_amd import skeleton as sk

    def columns(r, label=None):
        present = sorted(set(r["branches"][:, 1].tolist()) | set(r["nodes"][:, 1].tolist())) if label is None else label
        return sk.graph_columns(present, r["branches"], r["nodes"])

    names = ["skeleton_branches", "skeleton_junctions", "skeleton_cycles", "skeleton_spurs", "skeleton_components",
             "skeleton_branch_length_mean", "skeleton_branch_length_max", "skeleton_longest_path"]
    tee = columns(graph(TEE))
    assert list(tee) == names and [tee[c].tolist() for c in names] == [[3], [1], [0], [3], [1], [7 / 3], [3.0], [5.0]]
    wye = columns(graph(WYE))
    assert wye["skeleton_longest_path"].tolist() == [pytest.approx(4 * SQRT2)] and wye["skeleton_branch_length_max"].tolist() == [2 * SQRT2]
    tail = columns(graph(RING_WITH_TAIL))                 # the loop on the junction adds nothing to a shortest path
    assert [tail[c].tolist() for c in names] == [[2], [1], [0], [1], [1], [5.0], [8.0], [2.0]]
    ring = columns(graph(RING))
    assert [ring[c].tolist() for c in names] == [[1], [0], [1], [0], [1], [8.0], [8.0], [0.0]]
    lone = columns(graph(np.array([[4]], np.int32)), [2, 4])                       # a listed label without a skeleton pixel
    assert [lone[c].tolist() for c in names] == [[0, 0], [0, 0], [0, 0], [0, 0], [0, 1], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
    assert all(tee[c].dtype == (np.float64 if c in names[5:] else np.int64) for c in names)
    empty = sk.graph_columns([], np.zeros((0, 13)), np.zeros((0, 7)))
    assert list(empty) == names and all(len(c) == 0 for c in empty.values())
    with pytest.raises(ValueError, match="^graph_columns: needs increasing labels"):
        sk.graph_columns([2, 1], np.zeros((0, 13)), np.zeros((0, 7)))
    with pytest.raises(ValueError, match="^graph_columns: a row carries a label that is not listed"):
        sk.graph_columns([2], graph(TEE)["branches"], graph(TEE)["nodes"])
    with pytest.raises(ValueError, match="^graph_columns: a branch ends on a node that has no row"):
        sk.graph_columns([1], graph(TEE)["branches"], graph(TEE)["nodes"][1:])

    trees = others = 0
    every_source = lambda adjacency, members, tree, inner=sk._longest_path: inner(adjacency, members, False)
    for seed in range(12):
        _, r = noise(seed)
        want = summary(r["branches"], r["nodes"])
        got = columns(r, sorted(want))
        for c in names[:5]:
            assert got[c].tolist() == [want[label][c] for label in sorted(want)], (seed, c)
        for c in names[5:]:
            assert got[c].tolist() == pytest.approx([want[label][c] for label in sorted(want)], rel=1e-12, abs=0), (seed, c)
        rng = np.random.default_rng(seed)                 # the rows come from the device in any order: the same bits whatever it is
        mixed = sk.graph_columns(sorted(want), rng.permutation(r["branches"]), rng.permutation(r["nodes"]))
        assert all(mixed[c].tobytes() == got[c].tobytes() for c in names)
        trees += int((got["skeleton_branches"] == (r["nodes"][:, 1][:, None] == np.array(sorted(want))[None, :]).sum(0) - got["skeleton_components"]).sum())
        others += int((got["skeleton_cycles"] > 0).sum())
        with monkeypatch.context() as m:                  # the two sweeps of a tree against a sweep from every node
            m.setattr(sk, "_longest_path", every_source)
            slow = columns(r, sorted(want))
        assert slow["skeleton_longest_path"].tolist() == pytest.approx(got["skeleton_longest_path"].tolist(), rel=1e-12, abs=0)
    assert trees > 20 and others >= 1


def test_branch_columns_by_hand():
    from cellulus_amd.skeleton import branch_columns, node_columns

    r = graph(RING_WITH_TAIL, np.full(RING_WITH_TAIL.shape, 4))
    extra = np.array([[30, 2, END_END, 2, 1, 2, 22, 40, 22, 40, 13, 4, 9]])       # (3, 1) -> (5, 5) of a 7-wide map, made up
    table = branch_columns(np.concatenate([extra, r["branches"]]), (6, 7), radius=True)
    assert list(table) == ["first", "label", "kind", "path_pixels", "face_links", "diag_links", "pixel_a", "pixel_b", "node_a", "node_b",
                           "first_y", "first_x", "pixel_a_y", "pixel_a_x", "pixel_b_y", "pixel_b_x", "length", "euclidean", "tortuosity",
                           "radius_min", "radius_max", "dist_sq_mean"]
    assert table["first"].tolist() == [1, 11, 30] and table["first_y"].tolist() == [0, 1, 4] and table["first_x"].tolist() == [1, 4, 2]
    assert table["pixel_a_y"].tolist() == [1, 1, 3] and table["pixel_a_x"].tolist() == [3, 3, 1] and table["pixel_b_x"].tolist() == [3, 5, 5]
    assert table["length"].tolist() == [8.0, 2.0, 1 + 2 * SQRT2] and table["euclidean"].tolist() == [0.0, 2.0, math.sqrt(4 + 16)]
    assert np.isnan(table["tortuosity"][0]) and table["tortuosity"].tolist()[1:] == [1.0, (1 + 2 * SQRT2) / math.sqrt(20)]
    assert table["radius_min"].tolist() == [2.0, 2.0, 2.0] and table["radius_max"].tolist() == [2.0, 2.0, 3.0]
    assert table["dist_sq_mean"].tolist() == [4.0, 4.0, 6.5]
    ring = branch_columns(graph(RING)["branches"], RING.shape, radius=True)
    assert ring["pixel_a_y"].tolist() == [-1] and ring["pixel_b_x"].tolist() == [-1] and np.isnan(ring["euclidean"][0]) and np.isnan(ring["tortuosity"][0])
    assert ring["radius_min"].tolist() == [math.inf] and ring["dist_sq_mean"].tolist() == [math.inf] and ring["length"].tolist() == [8.0]
    stack = branch_columns([[41, 1, END_END, 0, 1, 0, 41, 42, 41, 42, 0, DIST_INF, -1]], (3, 4, 5))
    assert [stack[c].tolist() for c in ("first_z", "first_y", "first_x", "pixel_b_z", "pixel_b_y", "pixel_b_x")] == [[2], [0], [1], [2], [0], [2]]
    assert "radius_min" not in stack and all(v.dtype == (np.float64 if c in ("length", "euclidean", "tortuosity") else np.int64) for c, v in stack.items())
    empty = branch_columns(np.zeros((0, 13)), (4, 4))
    assert list(empty) == list(table)[:19] and all(len(c) == 0 for c in empty.values())
    for bad, shape in (([[99, 1, 0, 0, 1, 0, 1, 2, 1, 2, 0, 0, 0]], (4, 4)), ([[1, 1, 0, 0, 1, 0, 3, 2, 3, 2, 0, 0, 0]], (4, 4)),
                       ([[1, 1, 3, 0, 1, 0, 1, 2, 1, 2, 0, 0, 0]], (4, 4)), (np.zeros((0, 13)), (4,))):
        with pytest.raises(ValueError, match="^branch_columns: "):
            branch_columns(bad, shape)
    nodes = node_columns(graph(RING_WITH_TAIL)["nodes"][::-1], RING_WITH_TAIL.shape)
    assert list(nodes) == ["first", "label", "kind", "pixels", "links_out", "inner_face", "inner_diag", "first_y", "first_x"]
    assert nodes["first"].tolist() == [10, 12] and nodes["first_x"].tolist() == [3, 5] and nodes["links_out"].tolist() == [3, 1]


def test_prune_rule_in_integers():
    from cellulus_amd.skeleton import _limit_q10

    for f in range(6):
        for d in range(6):
            F, D = 1024 * f, 1024 * d
            first = F + math.isqrt(2 * D * D) + 1         # the smallest limit above 1024 (f + sqrt(2) d): sqrt(2) D is irrational for d > 0
            assert Fraction(first - 1 - F) ** 2 <= 2 * D * D < Fraction(first - F) ** 2 or d == 0
            for T in (0, 1, F, D, first - 1, first, first + 1, 1 << 29, (1 << 30) - 1):
                if T >= 0:
                    assert spur_pruned(f, d, T) == (T >= first), (f, d, T)
    assert spur_pruned(2 ** 31 - 1, 0, (1 << 30) - 1) is False and spur_pruned(0, 2 ** 20 - 1, (1 << 30) - 1) is False
    assert [_limit_q10(v, "w") for v in (0, 1, 1.0, 1.0005, SQRT2, 2.5, np.float32(3), 1 / 1024, 1 / 1024 + 1e-9)] == [0, 1024, 1024, 1025, 1449,
                                                                                                                   2560, 3072, 1, 2]
    assert [gref.prune_q10(v) for v in (0, 1.0005, SQRT2)] == [0, 1025, 1449]
    for bad in (-1, math.inf, math.nan, 2.0 ** 20):
        with pytest.raises(ValueError, match="^w: min_length must lie in"):
            _limit_q10(bad, "w")
    for bad in (True, "1", None):
        with pytest.raises(TypeError, match="^w: min_length must be a number"):
            _limit_q10(bad, "w")


def test_pruning_by_hand():
    wye = grid("""#.....#
                  .#...#.
                  ..#.#..
                  ...#...
                  ...#...
                  ...#...
                  ...#...""")
    wye[0, 0] = wye[1, 1] = 0                             # the left arm is one diagonal link, the right arm three, the stem three face links
    r = graph(wye, limit_q10=gref.prune_q10(1.5))         # sqrt(2) < 1.5
    assert r["info"][2:4] == [1, 1] and int((r["out"] != wye).sum()) == 1 and r["out"][2, 2] == 0
    assert sorted(r["branches"][:, 2].tolist()) == [SPUR] * 3
    again = graph(r["out"], limit_q10=gref.prune_q10(1.5))
    assert again["info"][2:4] == [0, 0] and np.array_equal(again["out"], r["out"])
    # the junction has become a path pixel: the other two arms are one end-end branch
    assert again["branches"][:, :6].tolist() == [[12, 1, END_END, 5, 3, 3]] and len(again["nodes"]) == 2
    assert gref.prune_q10(3 * SQRT2) == 4345
    for limit, pixels, spurs in ((0, 0, 0), (1024, 0, 0), (1448, 0, 0), (1449, 1, 1), (3072, 1, 1), (3073, 4, 2), (4344, 4, 2), (4345, 7, 3),
                                 ((1 << 30) - 1, 7, 3)):
        r = graph(wye, limit_q10=limit)
        assert r["info"][2:4] == [pixels, spurs], limit
        assert int((r["out"] != wye).sum()) == pixels and r["out"][3, 3] == 1 and ((r["out"] == wye) | (r["out"] == 0)).all()
    for never in (BAR, RING, BLOCK, np.array([[1, 1]], np.int32)):       # end-end branches and cycles stay
        r = graph(never, limit_q10=(1 << 30) - 1)
        assert r["info"][2:4] == [0, 0] and np.array_equal(r["out"], never)
    r = graph(PLUS, limit_q10=1025)                        # direct spurs: only the end pixels go
    assert r["info"][2:4] == [4, 4] and r["out"].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    tail = graph(RING_WITH_TAIL, limit_q10=2049)
    assert tail["info"][2:4] == [2, 1] and np.array_equal(tail["out"][:, :5], RING) and not tail["out"][:, 5:].any()


def test_refusals_without_a_device():
    from cellulus_amd import _clx
    from cellulus_amd.skeleton import branch_graph, prune_spurs, skeleton_stage, skeleton_table

    flat, stack = np.ones((4, 5), np.int32), np.ones((2, 4, 5), np.int32)
    for entry, args in ((branch_graph, ()), (prune_spurs, (2.0,))):
        who = entry.__name__
        with pytest.raises(ValueError, match=f"^{who}: 3-D curve skeletons are not implemented; planewise=True takes every slice as a map of its own$"):
            entry(stack, *args)
        with pytest.raises(ValueError, match=f"^{who}: planewise needs a 3-D map"):
            entry(flat, *args, planewise=True)
        with pytest.raises(TypeError, match=f"^{who}: planewise must be a bool"):
            entry(stack, *args, planewise=1)
        with pytest.raises(TypeError, match=f"^{who}: labels must be integers"):
            entry(flat.astype(np.float32), *args)
        with pytest.raises(ValueError, match=f"^{who}: labels must be 2-D or 3-D"):
            entry(np.ones(5, np.int32), *args)
        with pytest.raises(TypeError, match=f"^{who}: labels must be an array or a tensor"):
            entry([[1, 0]], *args)
        if not torch.cuda.is_available():
            with pytest.raises(_clx.ClxError, match="no CPU path"):
                entry(flat, *args)
    with pytest.raises(TypeError, match="^branch_graph: radius must be a bool"):
        branch_graph(flat, radius=1)
    with pytest.raises(ValueError, match="^prune_spurs: min_length must lie in"):
        prune_spurs(flat, -1.0)
    with pytest.raises(TypeError, match="^prune_spurs: min_length must be a number"):
        prune_spurs(flat, "2")
    with pytest.raises(ValueError, match="^prune_spurs: rounds must lie in"):
        prune_spurs(flat, 2.0, rounds=0)
    with pytest.raises(TypeError, match="^prune_spurs: rounds must be an integer"):
        prune_spurs(flat, 2.0, rounds=1.5)
    with pytest.raises(TypeError, match="^skeleton_table: graph must be a bool"):
        skeleton_table(flat, graph=1)
    with pytest.raises(ValueError, match="^skeleton_table: prune must lie in"):
        skeleton_table(flat, prune=-2)
    with pytest.raises(TypeError, match="^skeleton_stage: graph must be a bool"):
        skeleton_stage(None, "a", "b", graph="yes")
    with pytest.raises(TypeError, match="^skeleton_stage: prune must be a number"):
        skeleton_stage(None, "a", "b", prune="3")

    # the library refuses null pointers before any launch, and sizes its workspace on the host
    lib = _clx.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                              # never dereferenced: every call below is refused before any launch
    assert lib.clx_skeleton_graph(null, null, 2, 1, 4, 4, 0, 0, 0, null, null, null, null, null, null, 0, null) == -1
    assert lib.clx_last_error().startswith(b"clx_skeleton_graph: null pointer")
    for labels, info, workspace in ((null, one, one), (one, null, one), (one, one, null)):
        assert lib.clx_skeleton_graph(labels, null, 2, 1, 4, 4, 0, 0, 0, null, null, null, null, info, workspace, 1 << 20, null) == -1
        assert lib.clx_last_error().startswith(b"clx_skeleton_graph: null pointer")
    assert lib.clx_skeleton_graph(one, null, 2, 1, 4, 4, 0, 1, 0, null, null, null, null, one, one, 1 << 20, null) == -1
    assert lib.clx_last_error().startswith(b"clx_skeleton_graph: null branches with capacity_b > 0")
    assert lib.clx_skeleton_graph(one, null, 2, 1, 4, 4, 0, 0, 1, null, null, null, null, one, one, 1 << 20, null) == -1
    assert lib.clx_last_error().startswith(b"clx_skeleton_graph: null nodes with capacity_n > 0")
    assert lib.clx_skeleton_graph(one, null, 2, 1, 4, 4, 1, 0, 0, null, null, null, null, one, one, 1 << 20, null) == -1
    assert lib.clx_last_error().startswith(b"clx_skeleton_graph: null out with limit_q10 > 0")
    assert lib.clx_skeleton_graph_workspace(2, 1, 7, 9) == 40 * 7 * 9 and lib.clx_skeleton_graph_workspace(3, 3, 130, 67) == 40 * 3 * 130 * 67
    assert lib.clx_skeleton_graph_workspace(2, 2, 4, 4) == 0 and lib.clx_skeleton_graph_workspace(3, 1 << 11, 1 << 10, 1 << 10) == 0
    assert lib.clx_skeleton_graph_workspace(4, 1, 4, 4) == 0 and lib.clx_skeleton_graph_workspace(2, 1, 0, 4) == 0


def test_declared_exported_prototyped_and_on_the_command_line(tmp_path):
    from cellulus_amd import _clx

    text = open(os.path.join(ROOT, "include", "clx.h")).read()
    assert "A full 2 x 2 block of one label on its own is a cycle of 4 pixels" in " ".join(text.replace("*", " ").split())
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name in ("clx_skeleton_graph_workspace", "clx_skeleton_graph"):
        assert re.search(rf"\b{name}\s*\(", text) and hasattr(lib, name) and name in _clx.PROTOTYPES, name
    assert len(_clx.PROTOTYPES["clx_skeleton_graph"][1]) == 17 and _clx.load().clx_abi_version() == 13
    # one copy of the link rule: the census and the graph take it from skeleton_links.h
    csrc = os.path.join(ROOT, "cellulus_amd", "csrc")
    holders = sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".h")) and "Links links_at(" in open(os.path.join(csrc, n)).read())
    users = [n for n in os.listdir(csrc) if n.endswith(".hip") and '#include "skeleton_links.h"' in open(os.path.join(csrc, n)).read()]
    assert holders == ["skeleton_links.h"] and {"label_thin.hip", "skeleton_graph.hip"} <= set(users)
    from click.testing import CliRunner

    from cellulus_amd.cli import skeleton as command

    res = CliRunner().invoke(command, ["--help"])
    assert res.exit_code == 0 and all(o in res.output for o in ("--source", "--output", "--max-iter", "--planewise", "--radius", "--prune", "--graph"))
    # a length the library's limit cannot hold is a usage error, before any file is read
    config = tmp_path / "experiment.toml"
    config.write_text("")
    for bad in ("2e6", "-1", "1048576", "nan"):
        res = CliRunner().invoke(command, [str(config), "--source", "a", "--output", "b", "--prune", bad])
        assert res.exit_code == 2 and "--prune" in res.output, (bad, res.output)
