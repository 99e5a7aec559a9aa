"""The expand stage above the kernel: nearest_object(), expand_labels() and zone_table() against the restatements
(tests/nearest_ref.py) and scipy's recipe, the nuclei -> cells -> relate -> cytoplasm chain, and expand_stage() / the command end
to end on a small container.

The device maps and rows are integers and must be EQUAL to the restatement's; every float column is one rounded operation on
exact integers and is compared with the restatement's Fractions rounded once, with == too."""

import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from nearest_ref import DIST_INF, dots_map, ref_nearest, ref_zone_table
from relate_ref import blob_map
from test_cpu_expand import unique_nearest
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _toml

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_regionprops.npz")
MAPS = {"2d": blob_map((48, 70), 9, 51, 8), "3d": blob_map((7, 20, 26), 6, 52, 6), "dots": dots_map((40, 66), 14, 53, size=3)}
_WANT = {}


def want(name, limit_sq):
    """the restatement's maps, computed once per key and left unchanged"""
    if (name, limit_sq) not in _WANT:
        _WANT[name, limit_sq] = ref_nearest(MAPS[name], int(MAPS[name].max()) + 1, limit_sq)[:2]
    return _WANT[name, limit_sq]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_maps_equal_restatement(name, device):
    from cellulus_amd.expand import expand_labels, nearest_object

    labels = MAPS[name]
    given = [labels, torch.from_numpy(labels).to(device), labels.astype(np.uint16), torch.from_numpy(labels.astype(np.int64)).to(device),
             labels.astype(np.int64), torch.from_numpy(labels.astype(np.int64))]
    for limit, limit_sq in ((None, -1), (3, 9), (2.5, 6), (0, 0)):
        for g in given:
            nearest, dist = nearest_object(g, limit, device=device)
            assert all(t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == labels.shape for t in (nearest, dist))
            assert np.array_equal(nearest.cpu().numpy(), want(name, limit_sq)[0]) and np.array_equal(dist.cpu().numpy(), want(name, limit_sq)[1])
            if limit is None:
                continue
            grown = expand_labels(g, limit, device=device)
            assert type(grown) is type(g) and grown.dtype == g.dtype and tuple(grown.shape) == labels.shape
            if torch.is_tensor(g):
                assert grown.device == g.device
                grown = grown.cpu().numpy()
            assert np.array_equal(grown, want(name, limit_sq)[0])
            if limit == 0:
                assert np.array_equal(grown, labels)
    assert (want(name, 9)[0] != labels).sum() > 20 and (want(name, 9)[0] == 0).sum() > 20


def test_expand_labels_equals_the_scipy_recipe(device):
    from cellulus_amd.expand import expand_labels

    golden = np.load(GOLDEN)
    checked = 0
    for name in ("2d", "2d_edge", "3d"):
        labels = golden[f"{name}/labels"]
        edt, indices = ndimage.distance_transform_edt(labels == 0, return_indices=True)
        unique = unique_nearest(labels)
        for distance in (1, 2.5, 4):
            # edt is a rounded root: compare its exact square instead
            recipe = np.where(np.rint(edt ** 2) <= math.floor(distance ** 2), labels[tuple(indices)], 0)
            grown = expand_labels(labels, distance, device=device)
            assert grown.dtype == labels.dtype and np.array_equal(grown[unique], recipe[unique])
            assert np.array_equal(grown > 0, recipe > 0) and (grown[~unique] <= recipe[~unique]).all()
            assert np.array_equal(grown[labels > 0], labels[labels > 0])
            checked += int(((grown > 0) & (labels == 0)).sum())
    assert checked > 500


@pytest.mark.parametrize("name,limit,limit_sq", [("2d", None, -1), ("2d", 4, 16), ("3d", None, -1), ("3d", 2.9, 8), ("dots", None, -1),
                                                 ("dots", 5, 25)])
def test_zone_table_equals_restatement(name, limit, limit_sq, device):
    from cellulus_amd.expand import nearest_object, zone_table
    from cellulus_amd.measure import contact_pairs

    labels = MAPS[name]
    want_tables = ref_zone_table(labels, limit_sq)
    for g in (labels, torch.from_numpy(labels).to(device)):
        got = zone_table(g, limit, device=device)
        assert_same_tables(got, want_tables)
    table, pair = got
    assert len(table["label"]) == len(np.unique(labels)) - 1 > 3 and (limit is not None or (table["num_neighbours"] > 0).all())
    assert (table["zone_border_open"].sum() > 0) == (limit is not None)
    a, b, faces = contact_pairs(nearest_object(labels, limit, device=device)[0])
    assert np.array_equal(pair["label_a"], a) and np.array_equal(pair["label_b"], b) and np.array_equal(pair["faces"], faces)


def test_empty_maps_and_errors(device):
    from cellulus_amd.expand import expand_labels, nearest_object, zone_table

    for shape in ((6, 7), (3, 6, 7)):
        zeros = np.zeros(shape, np.int32)
        nearest, dist = nearest_object(zeros, device=device)
        assert (nearest == 0).all() and (dist == DIST_INF).all()
        assert np.array_equal(expand_labels(zeros, 5, device=device), zeros)
        tables = zone_table(zeros, device=device)
        assert_same_tables(tables, ref_zone_table(zeros))
        assert all(len(c) == 0 for t in tables for c in t.values())
    nothing = np.zeros((0, 5), np.int32)
    assert tuple(nearest_object(nothing, device=device)[0].shape) == (0, 5) and expand_labels(nothing, 1, device=device).shape == (0, 5)
    assert all(len(c) == 0 for t in zone_table(nothing, device=device) for c in t.values())
    with pytest.raises(ValueError, match="^nearest_object: label ids must lie in"):
        nearest_object(np.full((4, 4), 2 ** 24, np.int64), device=device)


def test_nuclei_to_cells_to_cytoplasm(device):
    from cellulus_amd.expand import expand_labels
    from cellulus_amd.relate import relate, tertiary_labels

    nuclei = MAPS["dots"]
    cells = expand_labels(nuclei, 4, device=device)
    child, parent = relate(nuclei, cells, device)
    assert len(child["label"]) == len(np.unique(nuclei)) - 1
    assert np.array_equal(child["parent"], child["label"]) and (child["fraction_inside"] == 1.0).all()
    assert np.array_equal(parent["label"], child["label"]) and (parent["num_children"] == 1).all()
    cytoplasm = tertiary_labels(nuclei, cells)
    assert np.array_equal(cytoplasm, np.where(nuclei > 0, 0, cells)) and (cytoplasm > 0).sum() > 100
    assert np.array_equal(parent["tertiary_area"], np.bincount(cytoplasm.reshape(-1), minlength=int(nuclei.max()) + 1)[parent["label"]])


def test_expand_stage_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import expand as expand_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.expand import expand_stage
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    raw = np.random.default_rng(91).integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    nuclei = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    nuclei[0, 0], nuclei[0, 1] = dots_map((40, 50), 9, 61, size=3), blob_map((40, 50), 6, 62, 10)
    nuclei[1, 1] = dots_map((40, 50), 4, 63)                            # sample 1: nothing at bandwidth 0
    f = zarr_io.open(container)
    for name, data in (("test/raw", raw), ("nuclei", nuclei)):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    paths = [(f"zones_bandwidth-{b}.csv", f"zone_pairs_bandwidth-{b}.csv") for b in range(2)]

    def check_csv(limit_sq):
        for b in range(2):
            for k, path in enumerate(paths[b]):
                lines = open(path).read().splitlines()
                header, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
                row = 0
                for s in range(2):
                    table = ref_zone_table(nuclei[s, b].astype(np.int32), limit_sq)[k]
                    assert header == ["sample"] + list(table)
                    for i in range(len(table[header[1]])):
                        if k == 1 and table["label_a"][i] == 0:
                            continue
                        text = ["%.17g" % c[i] if c.dtype == np.float64 else "%d" % c[i] for c in table.values()]
                        assert rows[row] == [str(s)] + text, (path, s, i)
                        row += 1
                assert row == len(rows)

    def check_dataset(name, limit_sq):
        ds = zarr_io.open(container, "r")[name]
        assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16
        assert ds.attrs["axis_names"] == ["s", "c", "y", "x"] and list(ds.attrs["resolution"]) == [1, 1] and list(ds.attrs["offset"]) == [0, 0]
        for s in range(2):
            for b in range(2):
                labels = nuclei[s, b].astype(np.int32)
                assert np.array_equal(ds[s, b], ref_nearest(labels, int(labels.max()) + 1, limit_sq)[0])

    expand_stage(config.inference_config, "nuclei", neighbours=True)
    check_csv(-1)
    assert len(open(paths[0][0]).readlines()) > 6 and len(open(paths[0][1]).readlines()) > 6 and len(open(paths[1][0]).readlines()) > 6
    assert open(paths[0][0]).readline().strip() == ("sample,label,area,zone_area,zone_fraction,zone_reach,zone_reach_y,zone_reach_x,"
                                                    "zone_dist_sq_mean,num_neighbours,zone_border,zone_border_open")
    assert open(paths[0][1]).readline().strip() == "sample,label_a,label_b,faces"
    assert "cells" not in zarr_io.open(container, "r")
    expand_stage(config.inference_config, "nuclei", output="cells", distance=3.5, neighbours=True, limit=6)
    check_csv(36)
    check_dataset("cells", 12)
    with pytest.raises(ValueError, match="^expand_stage: a dataset 'cells' exists"):
        expand_stage(config.inference_config, "nuclei", output="cells", distance=2)
    with pytest.raises(ValueError, match="^expand_stage: no dataset 'nucleus'"):
        expand_stage(config.inference_config, "nucleus", neighbours=True)
    with pytest.raises(ValueError, match="^expand_stage: nothing to do"):
        expand_stage(config.inference_config, "nuclei")
    check_dataset("cells", 12)                                          # the refusals changed nothing
    res = CliRunner().invoke(expand_cli, ["experiment.toml", "--source", "nuclei", "--distance", "2", "--output", "cells2"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check_dataset("cells2", 4)
    check_csv(36)                                                       # no --neighbours: the files stay
    res = CliRunner().invoke(expand_cli, ["experiment.toml", "--source", "nuclei", "--neighbours", "--limit", "2.9"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check_csv(8)
    res = CliRunner().invoke(expand_cli, ["experiment.toml", "--source", "nuclei"])
    assert res.exit_code == 1 and isinstance(res.exception, ValueError) and "nothing to do" in str(res.exception)
