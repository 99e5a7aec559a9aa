"""The convex hull quantities above the kernel: region_table(hull=True) against hull_columns of the restatement's integers
(tests/hull_ref.py), and measure(hull=True) / the command's --hull end to end.

The columns are formed by the same host function from integers that must be equal, so they are compared with ==."""

import os

import numpy as np
import pytest
import torch

from hull_ref import ref_hull
from test_gpu_contacts_stage import BOUNDARY, KEYS_2D, KEYS_3D
from test_gpu_measure_stage import _blob_map, _toml
from test_gpu_topology_stage import TOPOLOGY_2D, TOPOLOGY_3D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HULL_2D = ["area_convex", "solidity", "feret_diameter_max", "feret_diameter_min", "hull_vertices"]
HULL_3D = ["feret_diameter_max"]


def _maps():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    m = {name: g[f"{name}/labels"] for name in ("2d", "2d_edge", "3d")}
    m["blobs_2d"] = _blob_map((90, 120), 40, 41)
    m["blobs_3d"] = _blob_map((9, 30, 40), 25, 42)
    return m


MAPS = _maps()
WANT = {name: ref_hull(labels, labels.ndim) for name, labels in MAPS.items()}       # computed once, read by every test


@pytest.mark.parametrize("name", sorted(MAPS))
def test_hull_columns_equal_restatement(name, device):
    from cellulus_amd.measure import hull_columns, region_table

    labels = MAPS[name]
    nd = labels.ndim
    plain = region_table(labels, None, device)
    table = region_table(labels, None, device, hull=True)
    extra = HULL_2D if nd == 2 else HULL_3D
    assert list(table) == list(plain) + extra                          # appended; every old column where it was
    for k in plain:
        assert np.array_equal(plain[k], table[k]), k
    want = hull_columns(table["area"], WANT[name][table["label"]], nd)
    assert list(want) == extra and len(table["label"]) == len(np.unique(labels[labels > 0]))
    for k in extra:
        assert table[k].dtype == (np.int64 if k == "hull_vertices" else np.float64)
        assert np.array_equal(table[k], want[k]), k
    if nd == 2:
        assert (table["solidity"] <= 1.0).all() and (table["solidity"] > 0.0).all()
        assert (table["feret_diameter_min"] <= table["feret_diameter_max"]).all() and (table["feret_diameter_min"] >= 1.0).all()
        assert (table["area_convex"] >= table["area"]).all() and (table["hull_vertices"] >= 4).all()
    # with the other flags and a raw channel: the hull columns come last, everything else is what it was
    raw = np.random.default_rng(44).integers(0, 65536, size=labels.shape).astype(np.uint16)
    full = region_table(labels, raw, device, boundary=True, topology=True, hull=True)
    rest = region_table(labels, raw, device, boundary=True, topology=True)
    assert list(full) == list(rest) + extra
    for k in rest:
        assert np.array_equal(full[k], rest[k]), k
    for k in extra:
        assert np.array_equal(full[k], table[k]), k


def test_region_table_without_hull_keeps_its_keys(device):
    from cellulus_amd.measure import region_table

    raw = np.random.default_rng(43).integers(0, 65536, size=MAPS["2d"].shape).astype(np.uint16)
    assert list(region_table(MAPS["2d"], raw, device)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, hull=False)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, False, False, False)) == KEYS_2D
    assert list(region_table(MAPS["3d"], None, device)) == KEYS_3D
    assert list(region_table(MAPS["2d"], raw, device, hull=True)) == KEYS_2D + HULL_2D
    assert list(region_table(MAPS["2d"], raw, device, topology=True, hull=True)) == KEYS_2D + TOPOLOGY_2D + HULL_2D
    assert list(region_table(MAPS["2d"], raw, device, True, True, True)) == KEYS_2D + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D + HULL_2D
    assert list(region_table(MAPS["3d"], None, device, boundary=True, topology=True, hull=True)) == KEYS_3D + BOUNDARY + TOPOLOGY_3D + HULL_3D


def test_device_tensors_views_empty_and_errors(device):
    from cellulus_amd.measure import region_table

    for name in ("blobs_3d", "blobs_2d"):
        labels = MAPS[name]
        table = region_table(labels.astype(np.uint16), None, device, hull=True)
        again = region_table(torch.from_numpy(labels).to(device), hull=True)
        buf = torch.zeros(labels.size + 1, dtype=torch.int32, device=device)
        buf[1:] = torch.from_numpy(labels).to(device).reshape(-1)
        view = buf[1:].view(labels.shape)                              # does not start on a 16-byte boundary
        assert view.data_ptr() % 16 == 4
        third = region_table(view, hull=True)
        for other in (again, third):
            assert list(other) == list(table)
            for k in table:
                assert np.array_equal(other[k], table[k]), k
    for shape, names in (((6, 7), HULL_2D), ((3, 6, 7), HULL_3D), ((0, 5), HULL_2D)):
        empty = region_table(np.zeros(shape, np.int32), None, device, boundary=True, topology=True, hull=True)
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert all(empty[k].dtype == (np.int64 if k == "hull_vertices" else np.float64) for k in names)
    with pytest.raises(ValueError, match="^region_table:"):
        region_table(MAPS["2d"] - 1, None, device, hull=True)
    with pytest.raises(TypeError, match="^region_table:"):
        region_table(MAPS["2d"].astype(np.float32), None, device, hull=True)


def test_measure_hull_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(61)
    raw = rng.integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 9, 62)
    seg[0, 0, 10:20, 10:20] = 11
    seg[0, 0, 13:20, 13:20] = 0                                       # object 11 is an L: 51 pixels in a 10 x 10 box
    seg[0, 1] = _blob_map((40, 50), 6, 63)
    seg[1, 1] = _blob_map((40, 50), 5, 64)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    old_header = ["sample"] + KEYS_2D
    paths = [f"measurements_bandwidth-{b}.csv" for b in range(2)]

    def check(header_want, **flags):
        for b, path in enumerate(paths):
            header = open(path).readline().strip().split(",")
            assert header == header_want
            data = np.genfromtxt(path, delimiter=",", skip_header=1, dtype=np.float64).reshape(-1, len(header))
            row = 0
            for s in range(2):
                table = region_table(seg[s, b], raw[s], device, **flags)
                assert header == ["sample"] + list(table)
                n = len(table["label"])
                for name, column in table.items():                    # %.17g round-trips a float64
                    assert np.array_equal(data[row:row + n, header.index(name)], column.astype(np.float64)), (b, s, name)
                row += n
            assert row == len(data)
        return [open(path, "rb").read() for path in paths]

    measure(config.inference_config)
    plain = check(old_header)
    measure(config.inference_config, hull=True)
    check(old_header + HULL_2D, hull=True)
    lines = open(paths[0]).read().splitlines()
    header = lines[0].split(",")
    row = [line.split(",") for line in lines[1:] if line.split(",")[:2] == ["0", "11"]]
    assert len(row) == 1 and row[0][header.index("area")] == "51" and row[0][header.index("hull_vertices")] == "5"
    # the L's hull is the box less the triangle over its notch: 100 - 49 / 2
    assert float(row[0][header.index("area_convex")]) == 75.5 and float(row[0][header.index("solidity")]) == 51 / 75.5
    assert float(row[0][header.index("feret_diameter_max")]) == 200.0 ** 0.5
    measure(config.inference_config, contacts=True, topology=True, hull=True)
    check(old_header + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D + HULL_2D, boundary=True, topology=True, hull=True)
    assert os.path.exists("contacts_bandwidth-0.csv")
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--hull"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + HULL_2D, hull=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--hull", "--topology"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + TOPOLOGY_2D + HULL_2D, topology=True, hull=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check(old_header) == plain                                 # without the flag: the same bytes as before
