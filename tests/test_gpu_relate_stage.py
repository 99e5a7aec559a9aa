"""The relate stage above the kernels: label_overlaps(), relate() and tertiary_labels() against the restatement
(tests/relate_ref.py) and scipy, and relate_stage() / the command end to end on a small container.

The device rows are integers and must be EQUAL to the restatement's; every float column is one rounded operation on exact
integers and is compared with the restatement's Fractions rounded once, with == too."""

import numpy as np
import pytest
import torch
from scipy import ndimage

from relate_ref import blob_map, ref_overlaps, ref_relate
from test_cpu_relate import CHILDREN, PARENTS, assert_same_tables
from test_gpu_measure_stage import _toml

pytestmark = pytest.mark.gpu

# children: many small blobs; parents: a few large ones, so that children lie deep inside, across and outside them
CASES = {"2d": ((64, 80), 30, 9, 10, 3, 41), "3d": ((12, 24, 28), 24, 5, 8, 1.6, 42)}
_MAPS, _WANT = {}, {}


def maps(name):
    if name not in _MAPS:
        shape, na, nb, scale_a, scale_b, seed = CASES[name]
        _MAPS[name] = (blob_map(shape, na, seed, scale_a), blob_map(shape, nb, seed + 1, scale_b))
    return _MAPS[name]


def want(name, clearance, edge=False):
    """the restatement's tables, computed once per key and left unchanged"""
    if (name, clearance, edge) not in _WANT:
        _WANT[name, clearance, edge] = ref_relate(*maps(name), clearance, edge)
    return _WANT[name, clearance, edge]


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_equal_restatement(name, device):
    from cellulus_amd.relate import label_overlaps, relate

    children, parents = maps(name)
    given = [(children, parents),
             (torch.from_numpy(children.astype(np.int64)).to(device), torch.from_numpy(parents).to(device)),
             (children.astype(np.uint16), torch.from_numpy(parents).to(device))]
    keys, counts, _ = ref_overlaps(children, parents, int(children.max()) + 1, int(parents.max()) + 1)
    for a, b in given:
        ids_a, ids_b, pixels = label_overlaps(a, b, device)
        assert ids_a.dtype == ids_b.dtype == pixels.dtype == np.int64
        assert np.array_equal((ids_a.astype(np.uint64) << np.uint64(32)) | ids_b.astype(np.uint64), keys) and np.array_equal(pixels, counts)
        assert_same_tables(relate(a, b, device), want(name, False))
        assert_same_tables(relate(a, b, device, clearance=True), want(name, True))
    assert_same_tables(relate(children, parents, device, clearance=True, edge=True), want(name, True, True))
    child, parent = relate(children, parents, device, clearance=True)
    assert (child["parent"] > 0).sum() >= 8 and (child["num_parents"] > 1).any() and (parent["num_children"] > 1).any()
    assert len(np.unique(child["clearance"][child["parent"] > 0])) >= 4          # touching the boundary and deep inside
    # the clearance is scipy's distance transform of the parent's mask, over the child's pixels inside it
    checked = 0
    for row, (i, j) in enumerate(zip(child["label"], child["parent"])):
        inside = (children == i) & (parents == j)
        if j == 0 or not inside.any():
            assert np.isnan(child["clearance"][row])
            continue
        d = ndimage.distance_transform_edt(parents == j)
        d2 = np.rint(d * d).astype(np.int64)
        assert child["clearance"][row] == np.sqrt(float(d2[inside].min()))
        at = tuple(child[f"clearance_{axis}"][row] for axis in "zyx"[3 - children.ndim:])
        assert inside[at] and d2[at] == d2[inside].min()
        checked += 1
    assert checked >= 8


def test_by_hand_tertiary_and_region_table(device):
    from cellulus_amd.measure import region_table
    from cellulus_amd.relate import relate, tertiary_labels

    child, parent = relate(CHILDREN, PARENTS, device, clearance=True)
    assert child["parent"].tolist() == [1, 0, 2, 3, 4] and child["overlap"].tolist() == [4, 0, 4, 4, 2]
    assert child["clearance"][0] == np.sqrt(2.0) and np.isnan(child["clearance"][1]) and child["clearance"][2:].tolist() == [1.0, 1.0, 1.0]
    assert parent["tertiary_area"].tolist() == [3, 0, 1, 0, 0, 2] and parent["num_children"].tolist() == [1, 1, 1, 1, 0, 0]
    for name in sorted(CASES):
        children, parents = maps(name)
        _, parent = want(name, False)
        host = tertiary_labels(children, parents)
        assert host.dtype == parents.dtype and np.array_equal(host, np.where(children > 0, 0, parents))
        on_device = tertiary_labels(torch.from_numpy(children).to(device), torch.from_numpy(parents).to(device))
        assert on_device.is_cuda and on_device.dtype == torch.int32 and np.array_equal(on_device.cpu().numpy(), host)
        table = region_table(on_device, device=device)
        keeps = parent["tertiary_area"] > 0
        assert np.array_equal(table["label"], parent["label"][keeps]) and np.array_equal(table["area"], parent["tertiary_area"][keeps])


def test_retries_empty_maps_and_errors(monkeypatch, device):
    from cellulus_amd import relate as module
    from cellulus_amd.relate import label_overlaps, relate

    a = np.arange(1, 48 * 48 + 1, dtype=np.int32).reshape(48, 48)                  # 2304 pairs
    b = blob_map((48, 48), 9, 5)
    capacities = []
    real = module._clx.call

    def spy(name, *args):
        if name == "clx_label_overlaps":
            capacities.append(args[5])
        return real(name, *args)

    monkeypatch.setattr(module, "_pair_capacity", lambda objects: 1024)
    monkeypatch.setattr(module._clx, "call", spy)
    ids_a, ids_b, pixels = label_overlaps(a, b, device)
    assert capacities[:2] == [1024, 2048] and capacities == [1024 << k for k in range(len(capacities))] and capacities[-1] >= 4096
    keys, counts, _ = ref_overlaps(a, b, 48 * 48 + 1, 10)
    assert np.array_equal((ids_a.astype(np.uint64) << np.uint64(32)) | ids_b.astype(np.uint64), keys) and np.array_equal(pixels, counts)
    monkeypatch.undo()
    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zeros = np.zeros(shape, np.int32)
        assert all(len(v) == 0 and v.dtype == np.int64 for v in label_overlaps(zeros, zeros, device))
        tables = relate(zeros, zeros, device, clearance=True)
        assert_same_tables(tables, ref_relate(zeros, zeros, True))
        assert all(len(c) == 0 for t in tables for c in t.values())
    some = blob_map((6, 7), 3, 1)
    assert_same_tables(relate(np.zeros((6, 7), np.int32), some, device, clearance=True), ref_relate(np.zeros((6, 7), np.int32), some, True))
    assert_same_tables(relate(some, np.zeros((6, 7), np.int32), device, clearance=True), ref_relate(some, np.zeros((6, 7), np.int32), True))
    with pytest.raises(ValueError, match="^relate: label ids must lie in"):
        relate(np.full((4, 4), -1, np.int32), np.ones((4, 4), np.int32), device)
    with pytest.raises(ValueError, match="^label_overlaps: label ids must lie in"):
        label_overlaps(np.ones((4, 4), np.int64), np.full((4, 4), 2 ** 24, np.int64), device)


def test_relate_stage_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import relate as relate_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.relate import relate_stage
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    raw = np.random.default_rng(91).integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    cells = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    nuclei = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    cells[0, 0], nuclei[0, 0] = blob_map((40, 50), 7, 92, 3), blob_map((40, 50), 15, 93, 10)
    cells[0, 1], nuclei[0, 1] = blob_map((40, 50), 5, 94, 3), blob_map((40, 50), 12, 95, 10)
    nuclei[1, 1] = blob_map((40, 50), 4, 96)                            # sample 1: nothing at bandwidth 0, no cells at 1
    f = zarr_io.open(container)
    for name, data in (("test/raw", raw), ("cells", cells), ("nuclei", nuclei)):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    paths = [[f"relate_{kind}_bandwidth-{b}.csv" for kind in ("children", "parents")] for b in range(2)]

    def check(clearance):
        for b in range(2):
            for k, path in enumerate(paths[b]):
                lines = open(path).read().splitlines()
                header, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
                row = 0
                for s in range(2):
                    table = ref_relate(nuclei[s, b], cells[s, b], clearance)[k]
                    assert header == ["sample"] + list(table)
                    for i in range(len(table["label"])):
                        text = ["%.17g" % c[i] if c.dtype == np.float64 else "%d" % c[i] for c in table.values()]
                        assert rows[row] == [str(s)] + text, (path, s, i)
                        row += 1
                assert row == len(rows)
        assert len(open(paths[0][0]).readlines()) > 8 and len(open(paths[1][1]).readlines()) > 3

    relate_stage(config.inference_config, "nuclei", "cells")
    check(False)
    assert "cytoplasm" not in zarr_io.open(container, "r")
    relate_stage(config.inference_config, "nuclei", "cells", clearance=True, tertiary="cytoplasm")
    check(True)
    ds = zarr_io.open(container, "r")["cytoplasm"]
    assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16 and ds.attrs["axis_names"] == ["s", "c", "y", "x"]
    assert np.array_equal(ds[...], np.where(nuclei > 0, 0, cells))
    with pytest.raises(zarr_io.ContainsArrayError):                    # as segment(): an existing dataset is not clobbered
        relate_stage(config.inference_config, "nuclei", "cells", tertiary="cytoplasm")
    with pytest.raises(ValueError, match="^relate_stage: no dataset 'nucleus'"):
        relate_stage(config.inference_config, "nucleus", "cells")
    res = CliRunner().invoke(relate_cli, ["experiment.toml", "--children", "nuclei", "--parents", "cells", "--clearance", "--tertiary", "cyto2"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(True)
    assert np.array_equal(zarr_io.open(container, "r")["cyto2"][...], np.where(nuclei > 0, 0, cells))
    res = CliRunner().invoke(relate_cli, ["experiment.toml", "--children", "nuclei", "--parents", "cells"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(False)
