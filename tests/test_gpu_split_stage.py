"""The split stage above the kernels: basins(), basin_passes(), split_labels() and split_table() against the restatement
(tests/split_ref.py) on discs, ellipses, balls and blob maps, the label dtypes, the chain into region_table(), and
split_stage() / the command end to end on a small container.

The device maps and rows are integers and must be EQUAL to the restatement's; the two float columns are correctly rounded
square roots of exact integers and are compared with == too."""

import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from inscribed_ref import ref_distance_sq
from split_ref import NONE, ellipse, noise_blobs, ref_basins, ref_passes, ref_split, same_partition, two_balls, two_discs
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _toml

pytestmark = pytest.mark.gpu

MAPS = {"discs_11": two_discs(11), "discs_6": two_discs(6), "ellipse_16x5": ellipse((25, 25), (12, 12), 16, 5, 0.4),
        "ellipse_18x6": ellipse((25, 25), (12, 12), 18, 6, 1.1), "balls": two_balls(9), "blobs_2": noise_blobs(2), "blobs_7": noise_blobs(7)}
STAGE_DEPTHS = (0, Fraction(1, 2), 1, 2)
_WANT = {}


def want(name, depth, edge=False):
    """the restatement's map and table, computed once per key and left unchanged"""
    if (name, depth, edge) not in _WANT:
        _WANT[name, depth, edge] = ref_split(MAPS[name], depth, edge)[:2]
    return _WANT[name, depth, edge]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_basins_and_passes_equal_restatement(name, device):
    from cellulus_amd.split import basin_passes, basins

    labels = MAPS[name]
    for edge in (False, True):
        dist = ref_distance_sq(labels, edge)
        want_root, want_summits, _ = ref_basins(labels, dist)
        want_passes = ref_passes(labels, dist, want_root)
        for g in (labels, torch.from_numpy(labels).to(device), labels.astype(np.uint8)):
            root, summits = basins(g, edge, device=device)
            assert root.is_cuda and root.dtype == torch.int32 and tuple(root.shape) == labels.shape
            assert np.array_equal(root.cpu().numpy(), want_root) and (want_root[labels == 0] == NONE).all()
            assert summits.dtype == np.int64 and np.array_equal(summits, want_summits)
            got = basin_passes(g, edge, device=device)
            assert all(p.dtype == np.int64 and np.array_equal(p, w) for p, w in zip(got, want_passes))


@pytest.mark.parametrize("name", sorted(MAPS))
def test_split_labels_and_table_equal_restatement(name, device):
    from cellulus_amd.split import split_labels, split_table

    labels = MAPS[name]
    counts = []
    for depth in STAGE_DEPTHS:
        want_map, want_table = want(name, depth)
        for g in (labels, torch.from_numpy(labels).to(device)):
            new = split_labels(g, depth, device=device)
            assert type(new) is type(g) and new.dtype == g.dtype and tuple(new.shape) == labels.shape
            assert np.array_equal(new.cpu().numpy() if torch.is_tensor(new) else new, want_map)
        assert_same_tables((split_table(labels, depth, device=device),), (want_table,))
        counts.append(len(want_table["label"]))
    assert counts == sorted(counts, reverse=True) and counts[0] >= 2
    want_map, want_table = want(name, 1, True)
    assert np.array_equal(split_labels(labels, 1, edge=True, device=device), want_map)
    assert_same_tables((split_table(labels, edge=True, device=device),), (want_table,))
    assert np.array_equal(split_labels(labels, 1.0, device=device), want(name, 1)[0])            # a float depth, and the default
    assert np.array_equal(split_labels(labels, device=device), want(name, 1)[0])


def test_label_dtypes_and_tensors(device):
    from cellulus_amd.split import split_labels

    labels = MAPS["blobs_2"]
    want_map = want("blobs_2", Fraction(1, 2))[0]
    n = int(want_map.max())
    assert n > labels.max()
    given = [labels.astype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int64, np.uint64)]
    given += [torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(labels.astype(np.int16)), torch.from_numpy(labels.astype(np.uint8))]
    for g in given:
        new = split_labels(g, Fraction(1, 2), device=device)
        assert type(new) is type(g) and new.dtype == g.dtype
        if torch.is_tensor(g):
            assert new.device == g.device
            new = new.cpu().numpy()
        assert np.array_equal(new, want_map)
    # more pieces than the dtype holds: refused, nothing half written
    many = np.zeros((3, 600), np.int8)
    many[1, ::2] = 1                                            # 300 pixels of one label that do not touch: 300 pieces
    with pytest.raises(ValueError, match="^split_labels: 300 pieces do not fit int8"):
        split_labels(many, device=device)
    assert split_labels(many.astype(np.int16), device=device).max() == 300


def test_transposed_map(device):
    """Does a map's transpose give the transposed pieces, up to numbering?  NOT in general: among equal heights the smaller
    RASTER index is higher, and transposing changes which of two equal neighbours that is, so a flat ridge can drain to another
    summit and a pass between equal tops can merge the other way.  It holds where no decision rests on a tie, as for the two
    discs 11 apart below (a single highest pixel per disc; the pieces are mirror images either way); on the blob maps the
    partitions may differ, and what is promised instead is that two runs give equal bits."""
    from cellulus_amd.split import split_labels

    discs = MAPS["discs_11"]
    assert same_partition(split_labels(discs.T.copy(), 1, device=device).T, split_labels(discs, 1, device=device))
    blobs = MAPS["blobs_2"]
    assert not same_partition(split_labels(blobs.T.copy(), 1, device=device).T, split_labels(blobs, 1, device=device))
    for name in ("blobs_2", "blobs_7", "balls"):
        for depth in (0, 1):
            first, second = (split_labels(MAPS[name], depth, device=device) for _ in range(2))
            assert first.tobytes() == second.tobytes()


def test_empty_maps_and_errors(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.split import basin_passes, basins, split_labels, split_table

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    real = _clx.call
    monkeypatch.setattr(_clx, "call", no_call)                  # a map without objects makes no library call
    for zeros in (np.zeros((6, 7), np.int32), np.zeros((3, 6, 7), np.uint16), np.zeros((0, 5), np.int32), torch.zeros(4, 5, dtype=torch.int64)):
        new = split_labels(zeros, device=device)
        assert type(new) is type(zeros) and new.dtype == zeros.dtype and tuple(new.shape) == tuple(zeros.shape) and not new.any()
        table = split_table(zeros, device=device)
        assert len(table) == 6 + zeros.ndim and all(len(c) == 0 for c in table.values())
        root, summits = basins(zeros, device=device)
        assert tuple(root.shape) == tuple(zeros.shape) and (root == NONE).all() and len(summits) == 0
        assert all(len(p) == 0 for p in basin_passes(zeros, device=device))
    monkeypatch.setattr(_clx, "call", real)
    with pytest.raises(ValueError, match="^split_labels: label ids must lie in"):
        split_labels(np.full((4, 4), 2 ** 24, np.int64), device=device)
    one = np.zeros((5, 5), np.int32)
    one[2, 2] = 9
    assert np.array_equal(split_labels(one, device=device), (one > 0).astype(np.int32))
    table = split_table(one, device=device)
    assert table["parent"].tolist() == [9] and table["summit_radius"].tolist() == [1.0] and np.isnan(table["pass_radius"][0])
    assert table["area"].tolist() == [1] and table["summit_y"].tolist() == [2]


def test_split_then_region_table(device):
    from cellulus_amd.measure import region_table
    from cellulus_amd.split import split_labels, split_table

    labels = MAPS["blobs_7"]
    pieces = split_labels(labels, 1, device=device)
    table = region_table(pieces, device=device)
    ours = split_table(labels, 1, device=device)
    assert np.array_equal(table["label"], ours["label"]) and np.array_equal(table["area"], ours["area"])
    assert len(table["label"]) > len(np.unique(labels)) - 1 and table["area"].sum() == (labels > 0).sum()


def test_split_stage_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import split as split_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.split import split_stage
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    raw = np.random.default_rng(91).integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    cells = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    cells[0, 0], cells[0, 1] = noise_blobs(21, (40, 50)), noise_blobs(22, (40, 50), 2.0)
    cells[1, 1, 5:26, 9:41] = two_discs(11)                              # sample 1: nothing at bandwidth 0
    f = zarr_io.open(container)
    for name, data in (("test/raw", raw), ("cells", cells)):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))

    def check(name, depth, edge):
        ds = zarr_io.open(container, "r")[name]
        assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16
        assert ds.attrs["axis_names"] == ["s", "c", "y", "x"] and list(ds.attrs["resolution"]) == [1, 1] and list(ds.attrs["offset"]) == [0, 0]
        for b in range(2):
            lines = open(f"split_bandwidth-{b}.csv").read().splitlines()
            header, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
            assert header == ["sample", "label", "parent", "summit_y", "summit_x", "summit_radius", "pass_radius", "pieces_of_parent", "area"]
            row = 0
            for s in range(2):
                new, table, _ = ref_split(cells[s, b].astype(np.int32), depth, edge)
                assert np.array_equal(ds[s, b], new)
                for i in range(len(table["label"])):
                    text = ["%.17g" % c[i] if c.dtype == np.float64 else "%d" % c[i] for c in table.values()]
                    assert rows[row] == [str(s)] + text, (b, s, i)
                    row += 1
            assert row == len(rows)
        return len(open("split_bandwidth-1.csv").readlines())

    split_stage(config.inference_config, "cells", "pieces")
    assert check("pieces", 1, False) > len(np.unique(cells[0, 1])) + 2
    with pytest.raises(ValueError, match="^split_stage: a dataset 'pieces' exists"):
        split_stage(config.inference_config, "cells", "pieces", depth=2)
    with pytest.raises(ValueError, match="^split_stage: no dataset 'cell'"):
        split_stage(config.inference_config, "cell", "pieces2")
    with pytest.raises(ValueError, match="^split_stage: output must name a new dataset"):
        split_stage(config.inference_config, "cells", "cells")
    check("pieces", 1, False)                                           # the refusals changed nothing
    assert "pieces2" not in zarr_io.open(container, "r")
    res = CliRunner().invoke(split_cli, ["experiment.toml", "--source", "cells", "--output", "pieces2", "--depth", "0.5", "--edge"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("pieces2", Fraction(1, 2), True)
    res = CliRunner().invoke(split_cli, ["experiment.toml", "--source", "cells", "--output", "pieces3"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("pieces3", 1, False)
    res = CliRunner().invoke(split_cli, ["experiment.toml", "--source", "cells", "--output", "cells"])
    assert res.exit_code == 1 and isinstance(res.exception, ValueError) and "output must name" in str(res.exception)
    assert os.path.exists("split_bandwidth-0.csv")
