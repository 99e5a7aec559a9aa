"""The granularity stage without a device: the restatement (tests/granularity_ref.py) against scipy.ndimage and against itself --
erosion / dilation against grey_erosion / grey_dilation with the face footprint and the L1 ball, the two reconstructions
against each other on random maps with and without masks, the four properties of the reconstruction, the clamp algebra of the
kernel's row scan against the serial recurrence, maps worked by hand --, granularity_columns by hand and against Fractions,
every refusal of the Python layer, and the one-copy rule of the kernel sources."""

import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from granularity_ref import (MAX_LEVEL, ball_footprint, clamp_then, random_levels, ref_columns, ref_morph, ref_reconstruct,
                             ref_reconstruct_sweeps, ref_spectrum, row_by_clamps, row_serial)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (12, 5), (1, 13), (3, 6, 7), (5, 1, 4)], ids=lambda s: "x".join(map(str, s)))
def test_morph_equals_scipy(shape):
    from scipy import ndimage

    rng = np.random.default_rng(sum(shape))
    image = random_levels(rng, shape, 1000)
    nd = len(shape)
    face = ndimage.generate_binary_structure(nd, 1)
    assert ref_morph(image, None, 0, 1)[0].tolist() == ndimage.grey_erosion(image, footprint=face, mode="constant", cval=MAX_LEVEL).tolist()
    assert ref_morph(image, None, 1, 1)[0].tolist() == ndimage.grey_dilation(image, footprint=face, mode="constant", cval=0).tolist()
    for k in (2, 3, 5):
        ball = ball_footprint(nd, k)
        assert ball.sum() == sum(1 for p in np.ndindex(ball.shape) if sum(abs(c - k) for c in p) <= k)
        assert np.array_equal(ref_morph(image, None, 0, k)[0], ndimage.grey_erosion(image, footprint=ball, mode="constant", cval=MAX_LEVEL))
        assert np.array_equal(ref_morph(image, None, 1, k)[0], ndimage.grey_dilation(image, footprint=ball, mode="constant", cval=0))


def test_morph_masks_by_hand():
    image = np.array([[9, 9, 9, 9, 9], [9, 9, 9, 9, 9], [9, 9, 0, 9, 9]], np.int32)
    wall = np.ones(image.shape, np.uint8)
    wall[:, 1] = 0                                                      # column 0 cannot see the 0 behind the wall
    out, bad = ref_morph(image, wall, 0, 4)
    assert bad == 0 and out[:, 0].tolist() == [9, 9, 9] and out[:, 1].tolist() == [0, 0, 0] and (out[:, 2:] == 0).all()
    alone = np.zeros(image.shape, np.uint8)
    alone[1, 3] = 1                                                     # an inside pixel all of whose neighbours are outside
    for op in (0, 1):
        assert ref_morph(image, alone, op, 3)[0].tolist() == (np.where(alone, 9, 0)).tolist()
        assert not ref_morph(image, np.zeros(image.shape, np.uint8), op, 2)[0].any()
    dirty = image.copy()
    dirty[0, 0], dirty[2, 4] = -1, MAX_LEVEL + 1
    out, bad = ref_morph(dirty, None, 1, 1)
    assert bad == 1 and out[0, 0] == 9 and ref_morph(dirty, wall * 0, 1, 1)[1] == 0
    hidden = np.ones(image.shape, np.uint8)
    hidden[0, 0], hidden[2, 4] = 0, 0
    assert ref_morph(dirty, hidden, 0, 1)[1] == 0                        # under outside pixels the value does not count


def test_the_two_reconstructions_agree():
    rng = np.random.default_rng(7)
    for trial in range(120):
        nd = 2 if trial % 3 else 3
        shape = tuple(int(v) for v in rng.integers(1, 41 if nd == 2 else 9, size=nd))
        image = random_levels(rng, shape, int(rng.integers(2, 30)))
        marker = random_levels(rng, shape, 30) * (rng.random(shape) < 0.2)
        mask = (rng.random(shape) < 0.8).astype(np.uint8) if trial % 2 else None
        a, bad_a = ref_reconstruct(marker, image, mask)
        b, bad_b, _ = ref_reconstruct_sweeps(marker, image, mask)
        assert bad_a == bad_b == 0 and np.array_equal(a, b), (trial, shape)


def test_reconstruction_properties():
    rng = np.random.default_rng(11)
    for trial in range(30):
        shape = tuple(int(v) for v in rng.integers(2, 25, size=2 + trial % 2))
        image, marker = random_levels(rng, shape, 20), random_levels(rng, shape, 25) * (rng.random(shape) < 0.15)
        mask = (rng.random(shape) < 0.85).astype(np.uint8) if trial % 2 else None
        inside = np.ones(shape, bool) if mask is None else mask != 0
        out = ref_reconstruct(marker, image, mask)[0]
        m = np.where(inside, np.minimum(marker, image), 0)
        assert (m <= out).all() and (out <= np.where(inside, image, 0)).all()
        assert np.array_equal(ref_reconstruct(out, image, mask)[0], out)
        more = np.maximum(marker, random_levels(rng, shape, 25) * (rng.random(shape) < 0.1))
        assert (ref_reconstruct(more, image, mask)[0] >= out).all()
        axes = tuple(reversed(range(len(shape))))
        turned = ref_reconstruct(marker.transpose(axes), image.transpose(axes), None if mask is None else mask.transpose(axes))[0]
        assert np.array_equal(turned.transpose(axes), out)


def test_clamp_composition_equals_the_serial_row():
    rng = np.random.default_rng(13)
    for a, b, x in rng.integers(0, 12, size=(300, 3, 2)).tolist():
        a, b = (min(a), max(a)), (min(b), max(b))
        lo, hi = clamp_then(a, b)
        assert lo <= hi
        for v in range(0, 13):
            assert min(hi, max(lo, v)) == min(b[1], max(b[0], min(a[1], max(a[0], v))))
    for n in (1, 2, 3, 63, 64):
        for _ in range(20):
            image = rng.integers(0, 9, size=n)
            image[rng.random(n) < 0.1] = 0                              # outside pixels: the clamp to 0
            r = np.minimum(rng.integers(0, 9, size=n) * (rng.random(n) < 0.3), image)
            for carry in (0, 3, 8):
                assert row_by_clamps(r, image, carry) == row_serial(r, image, carry)


def _spectrum_of(image, scales):
    labels = np.ones(image.shape, np.int32)
    return [s[0] for s in ref_spectrum(labels, image, scales)[1]]


def test_hand_worked_maps():
    single = np.zeros((7, 7), np.int32)
    single[3, 3] = 50
    assert _spectrum_of(single, 2) == [50, 0, 0]                        # a single bright pixel vanishes at scale 1
    bar = np.zeros((9, 12), np.int32)
    bar[3:6, 2:10] = 40                                                 # 3 wide: one erosion leaves its middle row, two nothing
    assert _spectrum_of(bar, 3) == [40 * 24, 40 * 24, 0, 0]
    plateau = np.full((6, 8), 5, np.int32)
    plateau[1:5, 2:7] = 30
    marker = np.zeros(plateau.shape, np.int32)
    marker[2, 3] = 30                                                   # the marker touches the plateau at one pixel: restored whole
    out = ref_reconstruct(marker, plateau)[0]
    assert np.array_equal(out, np.where(plateau == 30, 30, 5))
    bridge = np.zeros((3, 9), np.int32)
    bridge[1, :4], bridge[1, 4], bridge[1, 5:] = 20, 7, 25              # a bridge of lower value passes only its own height
    marker = np.zeros(bridge.shape, np.int32)
    marker[1, 0] = 20
    assert ref_reconstruct(marker, bridge)[0][1].tolist() == [20] * 4 + [7] * 5
    marker[1, 0] = 99                                                   # a marker above the image is cut to it
    assert ref_reconstruct(marker, bridge)[0][1].tolist() == [20] * 4 + [7] * 5
    door = np.ones((5, 7), np.uint8)
    door[:, 3] = 0
    flat, seed = np.full((5, 7), 9, np.int32), np.zeros((5, 7), np.int32)
    seed[0, 0] = 9
    assert ref_reconstruct(seed, flat, door)[0].sum() == 9 * 15         # a wall: the far side stays 0
    door[4, 3] = 1
    assert ref_reconstruct(seed, flat, door)[0].sum() == 9 * 31         # a door of one pixel: everything inside


def test_tophat_is_never_negative():
    rng = np.random.default_rng(17)
    for shape in ((20, 30), (4, 9, 11)):
        image = random_levels(rng, shape, 500)
        for radius in (1, 2, 5):
            opened = ref_morph(ref_morph(image, None, 0, radius)[0], None, 1, radius)[0]
            assert (opened <= image).all() and (opened >= 0).all()


def test_granularity_columns_by_hand_and_against_fractions():
    from cellulus_amd.granularity import granularity_columns

    table = granularity_columns(np.array([[200, 0, 7], [150, 0, 7], [50, 0, 0]]), k=2)
    assert list(table) == ["granularity_1_c2", "granularity_2_c2", "granularity_residual_c2"]
    assert table["granularity_1_c2"][[0, 2]].tolist() == [25.0, 0.0] and table["granularity_2_c2"][[0, 2]].tolist() == [50.0, 100.0]
    assert table["granularity_residual_c2"][[0, 2]].tolist() == [25.0, 0.0]
    assert all(math.isnan(c[1]) and c.dtype == np.float64 for c in table.values())          # S_0 == 0
    rng = np.random.default_rng(19)
    drops = rng.integers(0, 10 ** 12, size=(9, 40))
    sums = np.cumsum(drops[::-1], axis=0)[::-1].astype(np.int64)
    sums[:, 5] = 0
    got, want = granularity_columns(sums), ref_columns([[int(v) for v in row] for row in sums])
    assert list(got) == list(want) == [f"granularity_{i}_c0" for i in range(1, 9)] + ["granularity_residual_c0"]
    for name in want:
        assert got[name].tobytes() == want[name].tobytes(), name
        assert np.isnan(got[name][5]) and (np.delete(got[name], 5) >= 0).all()
    total = sum(got[name] for name in got)
    assert np.allclose(np.delete(total, 5), 100.0, rtol=0, atol=1e-11)
    exact = sum(Fraction(100 * int(n), int(sums[0, 0])) for n in list(sums[:-1, 0] - sums[1:, 0]) + [sums[-1, 0]])
    assert exact == 100
    big = granularity_columns(np.array([[3 * 10 ** 30], [10 ** 30]], dtype=object))        # Python ints of any size
    assert big["granularity_1_c0"][0] == float(Fraction(200, 3)) and big["granularity_residual_c0"][0] == float(Fraction(100, 3))
    empty = granularity_columns(np.zeros((3, 0), np.int64))
    assert list(empty) == ["granularity_1_c0", "granularity_2_c0", "granularity_residual_c0"] and all(len(c) == 0 for c in empty.values())
    for bad in (np.zeros((1, 3), np.int64), np.zeros(3, np.int64), np.zeros((2, 2)), np.array([[1], [2]]), np.array([[1], [-1]])):
        with pytest.raises(ValueError, match="^granularity_columns: sums must"):
            granularity_columns(bad)


def test_spectrum_restatement_on_two_blob_sizes():
    from granularity_ref import quadrant_scene

    from cellulus_amd.propagate import image_levels

    labels, image = quadrant_scene(64, small=1.2, large=4.0)
    ids, sums = ref_spectrum(labels, image_levels(image, 256), 8)
    assert ids.tolist() == [1, 2, 3, 4]
    table = ref_columns(sums)
    spectrum = np.stack([table[f"granularity_{i}_c0"] for i in range(1, 9)])
    assert (spectrum >= 0).all() and spectrum[:, 0].argmax() < spectrum[:, 2].argmax()       # small blobs peak at a smaller scale


def test_refusals_without_a_device():
    from cellulus_amd import _clx
    from cellulus_amd.granularity import (granular_spectrum, granularity_stage, granularity_table, grey_dilate, grey_erode, grey_open,
                                          grey_reconstruct, grey_tophat)
    from cellulus_amd.measure import region_table

    flat = np.ones((4, 5), np.int32)
    for entry in (grey_erode, grey_dilate, grey_open, grey_tophat):
        who, steps = entry.__name__, "radius" if entry is grey_tophat else "steps"
        for bad in (1.5, True, "3", None):
            with pytest.raises(TypeError, match=f"^{who}: {steps} must be an integer"):
                entry(flat, bad)
        for bad in (0, -1, 2 ** 31):
            with pytest.raises(ValueError, match=f"^{who}: {steps} must lie in"):
                entry(flat, bad)
        with pytest.raises(TypeError, match=f"^{who}: image must be integers"):
            entry(flat.astype(np.float32), 1)
        with pytest.raises(TypeError, match=f"^{who}: image must be an array or a tensor"):
            entry([[1, 0]], 1)
        with pytest.raises(ValueError, match=f"^{who}: image must be 2-D or 3-D"):
            entry(np.ones(5, np.int32), 1)
        for value in (-1, MAX_LEVEL + 1):
            with pytest.raises(ValueError, match=f"^{who}: image must lie in \\[0, 65535\\]$"):
                entry(np.full((4, 5), value, np.int64), 1)
        with pytest.raises(ValueError, match=f"^{who}: mask has shape"):
            entry(flat, 1, mask=np.ones((4, 6), np.uint8))
        with pytest.raises(TypeError, match=f"^{who}: mask must be an array or a tensor"):
            entry(flat, 1, mask=[[1]])
    who = "grey_reconstruct"
    with pytest.raises(ValueError, match=f"^{who}: marker has shape"):
        grey_reconstruct(np.ones((5, 4), np.int32), flat)
    with pytest.raises(TypeError, match=f"^{who}: marker must be integers"):
        grey_reconstruct(flat.astype(np.float64), flat)
    with pytest.raises(ValueError, match=f"^{who}: marker must lie in"):
        grey_reconstruct(flat - 2, flat)
    with pytest.raises(ValueError, match=f"^{who}: image must lie in"):
        grey_reconstruct(flat, flat + MAX_LEVEL)
    with pytest.raises(ValueError, match=f"^{who}: mask has shape"):
        grey_reconstruct(flat, flat, mask=np.ones((1, 5), bool))
    image = np.zeros((4, 5))
    for who, call in (("granular_spectrum", lambda **kw: granular_spectrum(flat, flat, **kw)),
                      ("granularity_table", lambda **kw: granularity_table(flat, image, **kw)),
                      ("granularity_stage", lambda **kw: granularity_stage(None, "cells", **kw)),
                      ("region_table", lambda **kw: region_table(flat, image, **{("granularity" if k == "scales" else "granularity_" + k): v
                                                                                for k, v in dict({"scales": 4}, **kw).items()}))):
        for bad in (0, 65, -1):
            with pytest.raises(ValueError, match=f"^{who}: scales must lie in \\[1, 64\\]"):
                call(scales=bad)
        for bad in (1.0, True, "4"):
            with pytest.raises(TypeError, match=f"^{who}: scales must be an integer"):
                call(scales=bad)
        for bad in (-1, 65):
            with pytest.raises(ValueError, match=f"^{who}: background must lie in \\[0, 64\\]"):
                call(background=bad)
        with pytest.raises(TypeError, match=f"^{who}: background must be an integer"):
            call(background=0.5)
        if who != "granular_spectrum":
            for bad in (1, 65537):
                with pytest.raises(ValueError, match=f"^{who}: levels must lie in \\[2, 65536\\]"):
                    call(levels=bad)
            with pytest.raises(TypeError, match=f"^{who}: levels must be an integer"):
                call(levels=8.0)
    with pytest.raises(ValueError, match="^region_table: granularity needs raw$"):
        region_table(flat, granularity=4)
    with pytest.raises(ValueError, match="^granular_spectrum: levels_image has shape"):
        granular_spectrum(flat, np.ones((5, 4), np.int32))
    with pytest.raises(TypeError, match="^granular_spectrum: levels_image must be integers"):
        granular_spectrum(flat, image)
    with pytest.raises(ValueError, match="^granular_spectrum: levels_image must lie in"):
        granular_spectrum(flat, flat - 2)
    with pytest.raises(TypeError, match="^granular_spectrum: labels must be integers"):
        granular_spectrum(image, flat)
    with pytest.raises(ValueError, match="^granularity_table: image has shape"):
        granularity_table(flat, np.zeros((2, 5, 4)))
    with pytest.raises(TypeError, match="^granularity_table: image must be an array or a tensor"):
        granularity_table(flat, [[0.0]])
    for source in (None, "", 3):
        with pytest.raises(ValueError, match="^granularity_stage: source must be the name of a dataset"):
            granularity_stage(None, source)
    for channel in (-1, 1.0, True):
        with pytest.raises(ValueError, match="^granularity_stage: channel must be an integer >= 0 or None"):
            granularity_stage(None, "cells", channel=channel)
    if not torch.cuda.is_available():
        for call in (lambda: grey_erode(flat), lambda: grey_reconstruct(flat, flat), lambda: granular_spectrum(flat, flat),
                     lambda: granularity_table(flat, image)):
            with pytest.raises(_clx.ClxError, match="no CPU path"):
                call()


def test_symbols_and_commands():
    from click.testing import CliRunner

    from cellulus_amd import _clx, cli

    for name in ("clx_grey_morph", "clx_grey_reconstruct_workspace", "clx_grey_reconstruct"):
        assert name in _clx.PROTOTYPES
        assert name + "(" in open(os.path.join(ROOT, "include", "clx.h"), encoding="utf-8").read()
    assert len(_clx.PROTOTYPES["clx_grey_morph"][1]) == 11 and len(_clx.PROTOTYPES["clx_grey_reconstruct"][1]) == 14
    res = CliRunner().invoke(cli.granularity, ["--help"])
    assert res.exit_code == 0 and all(opt in res.output for opt in ("--source", "--channel", "--scales", "--levels", "--background"))
    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and all(opt in res.output for opt in ("--granularity ", "--granularity-background", "--granularity-levels"))
    assert "``granularity``" in __import__("cellulus_amd._stage", fromlist=["x"]).__doc__


def test_one_copy_of_the_shared_helpers():
    csrc = os.path.join(ROOT, "cellulus_amd", "csrc")
    text = open(os.path.join(csrc, "grey_morph.hip"), encoding="utf-8").read()
    assert '#include "region_scan.h"' in text
    for piece in ("constexpr int BLOCK", "typedef unsigned long long u64", "int find_slot(", "void load_labels(", "bool clamp_labels(",
                  "int run_lanes(", "Tiles block_tiles(", "long long lane_pixel(", "Heads run_heads(", "V reduce_run(", "struct SumKey",
                  "struct Pixel", "PixelInRow pixel_at(", "Pixel next_pixel(", "void table_init(", "void launch_table_init(",
                  "bool aligned16(", "Tiling tiling_for(", "#define CLX_REQUIRE", "#define CLX_CHECK_LAUNCH"):
        assert piece not in text, piece
        assert any(piece in open(os.path.join(csrc, h), encoding="utf-8").read() for h in ("region_scan.h", "clx_common.h")), piece
