"""CPU tier of the skeleton stage: the restatement of the definitions (tests/skeleton_ref.py) against thinning every object's
mask alone, against scipy.ndimage.label for the topology and the Euler identity, on maps worked by hand; skeleton_columns by
hand; the entry points' refusals that need no device; the declarations in include/clx.h."""

import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from skeleton_ref import DIST_INF, WORDS, census, noise_map, skeleton, thin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT, FOUR = np.ones((3, 3), int), ndimage.generate_binary_structure(2, 1)


def _topology(mask):
    """(8-connected components, 4-connected holes) of a 2-D mask"""
    padded = np.pad(mask, 1)
    return ndimage.label(padded, EIGHT)[1], ndimage.label(~padded, FOUR)[1] - 1


def test_label_aware_equals_each_mask_alone_and_is_idempotent():
    objects = 0
    for seed in range(12):
        labels = noise_map((31 + seed, 45 - seed), seed, block=9)
        got, deleted = thin(labels)
        assert deleted[-1] == 0 and sum(deleted) == int((labels != 0).sum() - (got != 0).sum())
        for label in np.unique(labels[labels != 0]):
            alone = skeleton((labels == label).astype(np.int32))
            assert np.array_equal(got == label, alone == 1), (seed, label)
            objects += 1
        again, deleted = thin(got)
        assert np.array_equal(again, got) and deleted == [0]
    assert objects > 40


def test_topology_is_kept():
    changed = 0
    for seed in range(10):
        labels = noise_map((40, 52), 100 + seed, block=13, sigma=1.5)
        got = skeleton(labels)
        for label in np.unique(labels[labels != 0]):
            assert _topology(got == label) == _topology(labels == label), (seed, label)
        changed += int((got != labels).sum())
        assert ((got == labels) | (got == 0)).all()
    assert changed > 2000


def test_3d_is_slice_by_slice():
    labels = noise_map((3, 20, 27), 7, block=8)
    got, deleted = thin(labels)
    assert np.array_equal(got, np.stack([skeleton(s) for s in labels]))
    assert thin(labels, 2)[1] == [sum(thin(s, 2)[1][i] for s in labels) for i in range(2)]


def test_maps_worked_by_hand():
    square2 = np.zeros((4, 4), np.int32)
    square2[1:3, 1:3] = 7
    got, deleted = thin(square2)
    assert np.argwhere(got).tolist() == [[2, 1]] and got[2, 1] == 7 and deleted == [3, 0]      # the bottom-left pixel
    square3 = np.ones((3, 3), np.int32)
    assert np.argwhere(skeleton(square3)).tolist() == [[1, 1]] and thin(square3)[1] == [8, 0]
    bar = np.ones((2, 5), np.int32)
    want = np.zeros((2, 5), np.int32)
    want[1, 0:4] = 1
    assert np.array_equal(skeleton(bar), want)
    stairs = (np.eye(6) + np.eye(6, k=1)).astype(np.int32)
    assert np.array_equal(skeleton(stairs), np.eye(6, dtype=np.int32))
    for same in (np.ones((1, 1), np.int32), np.zeros((3, 4), np.int32), np.array([[1, 0, 0], [0, 1, 1], [1, 0, 0]], np.int32)):
        assert np.array_equal(skeleton(same), same) and thin(same)[1] == [0]
    # The 3 x 3 plus does NOT stay under the stated conditions.  Its top arm has P5 = P6 = P7 = 1 and nothing else: C = 1 (only
    # !P4 & (P5|P6)), N1 = N2 = 2, and P4 = 0 makes m = 0, so the first sub-iteration deletes it, and likewise the right arm
    # (P7 = P8 = P9) and the bottom arm (P9 = P2 = P3); the left arm has P3 = P4 = P5 = 1, so m = (P2|P3|!P5) & P4 = 1 keeps it.
    # The centre has C = 0.  In the second sub-iteration the left arm has N = 1.  Centre and left arm remain.
    plus = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.int32)
    assert np.array_equal(skeleton(plus), np.array([[0, 0, 0], [1, 1, 0], [0, 0, 0]], np.int32)) and thin(plus)[1] == [3, 0]
    # touching objects thin independently, in both id orders; the ends of rows do not wrap
    pair = np.zeros((5, 8), np.int32)
    pair[1:4, 1:4], pair[1:4, 4:7] = 1, 2
    for a, b in ((1, 2), (2, 1), (-5, 2 ** 31 - 1)):
        both = np.where(pair == 1, a, np.where(pair == 2, b, 0)).astype(np.int32)
        assert np.argwhere(skeleton(both)).tolist() == [[2, 2], [2, 5]]
    ends = np.zeros((4, 6), np.int32)
    ends[0:2, 4:6], ends[1:3, 0:2] = 1, 1
    assert np.array_equal(skeleton(ends) != 0, (skeleton(np.pad(ends, ((0, 0), (0, 3)))) != 0)[:, :6])


def _words(rows):
    return census(np.array(rows, np.int32))[0][1, :7].tolist()


def test_census_by_hand():
    assert _words([[1, 1, 1], [0, 1, 0], [0, 1, 0]]) == [5, 4, 0, 0, 3, 1, 0]                 # T
    assert _words([[1, 0, 1], [0, 1, 0], [0, 1, 0]]) == [4, 1, 2, 0, 3, 1, 0]                 # Y: two diagonal links
    assert _words([[0, 1, 0], [1, 1, 1], [0, 1, 0]]) == [5, 4, 0, 0, 4, 1, 0]                 # plus
    assert _words([[1, 0], [1, 1]]) == [3, 2, 0, 0, 2, 0, 0]                                  # L: its diagonal is no link
    assert _words([[1, 1], [1, 1]]) == [4, 4, 0, 1, 0, 0, 0]                                  # a block
    assert _words([[1, 0, 0], [0, 0, 0], [0, 0, 1]]) == [2, 0, 0, 0, 0, 0, 2]                 # two isolated pixels
    # another label between two diagonal neighbours is background for them; every label has its own words
    words, bad = census(np.array([[1, 2], [2, 1]], np.int32))
    assert bad == 0 and words[1, :7].tolist() == [2, 0, 1, 0, 2, 0, 0] and words[2, :7].tolist() == [2, 0, 1, 0, 2, 0, 0]
    assert words[0].tolist() == [0] * 8 + [DIST_INF, -1] and words[1, 7:].tolist() == [0, DIST_INF, -1]
    # the d2 words, the bad bits
    skel = np.array([[1, 1, 0], [0, 0, 3]], np.int32)
    words, bad = census(skel, np.array([[4, 9, 5], [0, 0, 2]]), nid=5)
    assert bad == 0 and words[1, 7:].tolist() == [13, 4, 9] and words[3, 7:].tolist() == [2, 2, 2] and words[4, 7:].tolist() == [0, DIST_INF, -1]
    words, bad = census(skel, np.array([[4, DIST_INF, 5], [0, 0, -1]]), nid=4)
    assert bad == 2 and words[1].tolist() == [2, 1, 0, 0, 2, 0, 0, 4, 4, 4] and words[3, 7:].tolist() == [0, DIST_INF, -1]
    words, bad = census(skel, nid=3)
    assert bad == 1 and words.shape == (3, 10) and words[1, 0] == 2
    assert census(np.array([[-1, 1]], np.int32))[1] == 1 and len(WORDS) == 10


def test_euler_identity_on_unthinned_maps():
    blocks = 0
    for seed in range(12):
        labels = noise_map((36, 44), 200 + seed, block=11, sigma=1.2)
        for lab in (labels, skeleton(labels)):
            words = census(lab)[0]
            for label in np.unique(lab[lab != 0]):
                parts, holes = _topology(lab == label)
                assert words[label, 0] - words[label, 1] - words[label, 2] + words[label, 3] == parts - holes, (seed, label)
        blocks += int(census(labels)[0][:, 3].sum())
    assert blocks > 1000                                 # the unthinned maps are full of 2 x 2 blocks and dropped diagonals


def test_skeleton_columns_by_hand():
    from cellulus_amd.skeleton import skeleton_columns

    words = np.array([[5, 3, 2, 1, 2, 1, 0, 30, 1, 16], [1, 0, 0, 0, 0, 0, 1, 0, DIST_INF, -1]])
    table = skeleton_columns([2, 9], [40, 1], words, radius=True)
    assert list(table) == ["label", "area", "skeleton_pixels", "skeleton_length", "skeleton_end_points", "skeleton_branch_points",
                           "skeleton_isolated", "skeleton_euler_number", "skeleton_radius_min", "skeleton_radius_max", "skeleton_dist_sq_mean"]
    assert table["label"].tolist() == [2, 9] and table["area"].tolist() == [40, 1] and table["skeleton_pixels"].tolist() == [5, 1]
    assert table["skeleton_length"].tolist() == [3 + math.sqrt(2.0) * 2, 0.0]
    assert table["skeleton_end_points"].tolist() == [2, 0] and table["skeleton_branch_points"].tolist() == [1, 0]
    assert table["skeleton_isolated"].tolist() == [0, 1] and table["skeleton_euler_number"].tolist() == [1, 1]
    assert table["skeleton_radius_min"].tolist() == [1.0, math.inf] and table["skeleton_radius_max"].tolist() == [4.0, math.inf]
    assert table["skeleton_dist_sq_mean"].tolist() == [6.0, math.inf]
    assert all(table[c].dtype == (np.float64 if c in ("skeleton_length", "skeleton_radius_min", "skeleton_radius_max",
                                                      "skeleton_dist_sq_mean") else np.int64) for c in table)
    plain = skeleton_columns([2, 9], [40, 1], words)
    assert list(plain) == list(table)[:8]
    empty = skeleton_columns([], [], np.zeros((0, 10)), radius=True)
    assert list(empty) == list(table) and all(len(c) == 0 for c in empty.values())
    for label, area, w in (([2, 2], [1, 1], words), ([0, 1], [1, 1], words), ([1, 2], [0, 1], words), ([1, 2], [4, 1], words), ([1], [9], words)):
        with pytest.raises(ValueError, match="^skeleton_columns: "):
            skeleton_columns(label, area, w)
    with pytest.raises(TypeError, match="radius must be a bool"):
        skeleton_columns([2, 9], [40, 1], words, radius=1)


def test_refusals_without_a_device():
    from cellulus_amd import _clx
    from cellulus_amd.skeleton import skeleton_stage, skeleton_table, thin_labels

    flat, stack = np.ones((4, 5), np.int32), np.ones((2, 4, 5), np.int32)
    for entry in (thin_labels, skeleton_table):
        who = entry.__name__
        with pytest.raises(ValueError, match=f"^{who}: 3-D thinning is not implemented; planewise=True thins every slice on its own$"):
            entry(stack)
        with pytest.raises(ValueError, match=f"^{who}: planewise needs a 3-D map"):
            entry(flat, planewise=True)
        with pytest.raises(TypeError, match=f"^{who}: planewise must be a bool"):
            entry(stack, planewise=1)
        with pytest.raises(ValueError, match=f"^{who}: max_iter must lie in"):
            entry(flat, max_iter=-1)
        for bad in (1.5, True, "3"):
            with pytest.raises(TypeError, match=f"^{who}: max_iter must be an integer or None"):
                entry(flat, max_iter=bad)
        with pytest.raises(TypeError, match=f"^{who}: labels must be integers"):
            entry(flat.astype(np.float32))
        with pytest.raises(ValueError, match=f"^{who}: labels must be 2-D or 3-D"):
            entry(np.ones(5, np.int32))
        with pytest.raises(TypeError, match=f"^{who}: labels must be an array or a tensor"):
            entry([[1, 0]])
    with pytest.raises(TypeError, match="^skeleton_table: radius must be a bool"):
        skeleton_table(flat, radius=1)
    if not torch.cuda.is_available():
        with pytest.raises(_clx.ClxError, match="no CPU path"):
            thin_labels(flat)
    for source, output in ((None, "a"), ("", "a"), ("a", ""), ("a", "a"), ("a", 3)):
        with pytest.raises(ValueError, match="^skeleton_stage: (source|output) must"):
            skeleton_stage(None, source, output)
    with pytest.raises(ValueError, match="^skeleton_stage: max_iter must lie in"):
        skeleton_stage(None, "a", "b", max_iter=-2)
    with pytest.raises(TypeError, match="^skeleton_stage: planewise must be a bool"):
        skeleton_stage(None, "a", "b", planewise="yes")
    with pytest.raises(TypeError, match="^skeleton_stage: radius must be a bool"):
        skeleton_stage(None, "a", "b", radius=0)
    # the library refuses null pointers before any launch, and sizes its workspace on the host
    lib = _clx.load()
    assert lib.clx_label_thin(None, 2, 1, 4, 4, 1, 0, None, None, None, 0, None) == -1 and b"null pointer" in lib.clx_last_error()
    assert lib.clx_skeleton_census(None, None, 2, 1, 4, 4, 2, None, None, None) == -1 and b"null pointer" in lib.clx_last_error()
    assert lib.clx_label_thin_workspace(2, 1, 96, 384) == 128 + 10 * 8 * 96 * 6 + 2 * 8          # one tile
    assert lib.clx_label_thin_workspace(3, 2, 97, 385) == 128 + 10 * 8 * 2 * 97 * 7 + 2 * 8      # 2 x 2 x 2 tiles
    assert lib.clx_label_thin_workspace(2, 2, 4, 4) == 0 and lib.clx_label_thin_workspace(3, 1 << 11, 1 << 10, 1 << 10) == 0
    assert lib.clx_label_thin_workspace(4, 1, 4, 4) == 0 and lib.clx_label_thin_workspace(2, 1, 0, 4) == 0


def test_declared_in_the_header_and_on_the_command_line():
    text = open(os.path.join(ROOT, "include", "clx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("clx_label_thin_workspace", "clx_label_thin", "clx_skeleton_census"):
        assert re.search(rf"\b{name}\s*\(", text), name
    from click.testing import CliRunner

    from cellulus_amd.cli import skeleton as command

    res = CliRunner().invoke(command, ["--help"])
    assert res.exit_code == 0 and all(o in res.output for o in ("--source", "--output", "--max-iter", "--planewise", "--radius"))
