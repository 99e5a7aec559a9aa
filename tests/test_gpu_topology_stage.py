"""The topology quantities above the kernel: region_table(topology=True) against the restated columns of
tests/topology_ref.py, and measure(topology=True) / the command's --topology end to end.

The float columns are formed twice from the same integers, by cellulus_amd.measure.topology_columns and by the
restatement, so they may differ by the roundings of either side and no more.  Every term of the sums is non-negative, so
a rounding of relative size u = 2^-53 stays one: the bars below are 2 x (roundings of one evaluation) x u.
  perimeter_crofton  sqrt 2, N2 / sqrt 2, the sum, pi / 8, the product: 5
  surface_area       per term the weight, its product with N, sqrt k, the division: 4; two sums; the factors 2 and 4 are
                     exact: 6
  sphericity         surface_area: 6; pi^(1/3): pi, the exponent, pow (1 ulp = 2 u): 4; (6 area)^(2/3): the exponent is the
                     same constant on both sides, pow: 2; the product and the division: 2; 14 in all"""

import os

import numpy as np
import pytest
import torch

from test_gpu_contacts_stage import BOUNDARY, KEYS_2D, KEYS_3D
from test_gpu_measure_stage import _blob_map, _toml
from test_gpu_topology import call_topology
from topology_ref import ref_topology_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
RTOL = {"perimeter_crofton": 2 * 5 * U, "surface_area": 2 * 6 * U, "sphericity": 2 * 14 * U}
EULER = ["euler_number", "euler_number_conn1"]
TOPOLOGY_2D = EULER + ["perimeter_crofton"]
TOPOLOGY_3D = EULER + ["surface_area", "sphericity"]


def _maps():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    m = {name: g[f"{name}/labels"] for name in ("2d", "2d_edge", "3d")}
    m["blobs_2d"] = _blob_map((90, 120), 40, 41)
    m["blobs_3d"] = _blob_map((9, 30, 40), 25, 42)
    return m


MAPS = _maps()
WANT = {name: ref_topology_table(labels) for name, labels in MAPS.items()}      # computed once, read by every test


@pytest.mark.parametrize("name", sorted(MAPS))
def test_topology_columns_equal_restatement(name, device):
    from cellulus_amd.measure import region_table

    labels = MAPS[name]
    nd = labels.ndim
    plain = region_table(labels, None, device)
    table = region_table(labels, None, device, topology=True)
    want, counts = WANT[name]
    extra = TOPOLOGY_2D if nd == 2 else TOPOLOGY_3D
    assert list(table) == list(plain) + extra                          # appended; every old column where it was
    for k in plain:
        assert np.array_equal(plain[k], table[k]), k
    assert len(want["euler_number"]) == len(table["label"])
    for k in extra:
        if k in EULER:
            assert table[k].dtype == np.int64 and np.array_equal(table[k], want[k]), k
        else:
            assert table[k].dtype == np.float64
            print(name, k, "largest relative difference", float(np.max(np.abs(table[k] - want[k]) / want[k], initial=0.0)),
                  "bar", RTOL[k])
            assert np.allclose(table[k], want[k], rtol=RTOL[k], atol=0), k
    # both flags: the topology columns come after the boundary columns, and T1 counts the same faces
    both = region_table(labels, None, device, boundary=True, topology=True)
    bound = region_table(labels, None, device, boundary=True)
    assert list(both) == list(bound) + extra
    for k in bound:
        assert np.array_equal(both[k], bound[k]), k
    for k in extra:
        assert np.array_equal(both[k], table[k]), k
    raw_counts, bad = call_topology(labels, nd, int(labels.max()) + 1, device)
    assert bad == 0 and np.array_equal(raw_counts[table["label"]], counts)
    assert np.array_equal(counts[:, 0], both["boundary_faces"] << (nd - 1))


def test_region_table_without_topology_keeps_its_keys(device):
    from cellulus_amd.measure import region_table

    raw = np.random.default_rng(43).integers(0, 65536, size=MAPS["2d"].shape).astype(np.uint16)
    assert list(region_table(MAPS["2d"], raw, device)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, topology=False)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, False, False)) == KEYS_2D
    assert list(region_table(MAPS["3d"], None, device)) == KEYS_3D
    assert list(region_table(MAPS["2d"], raw, device, boundary=True, topology=False)) == KEYS_2D + BOUNDARY + ["border_pixels", "perimeter"]
    assert list(region_table(MAPS["2d"], raw, device, topology=True)) == KEYS_2D + TOPOLOGY_2D
    assert list(region_table(MAPS["2d"], raw, device, True, True)) == KEYS_2D + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D
    assert list(region_table(MAPS["3d"], None, device, boundary=True, topology=True)) == KEYS_3D + BOUNDARY + TOPOLOGY_3D


def test_device_tensors_views_empty_and_errors(device):
    from cellulus_amd.measure import region_table

    labels = MAPS["blobs_3d"]
    table = region_table(labels.astype(np.uint16), None, device, topology=True)
    again = region_table(torch.from_numpy(labels).to(device), topology=True)
    buf = torch.zeros(labels.size + 1, dtype=torch.int32, device=device)
    buf[1:] = torch.from_numpy(labels).to(device).reshape(-1)
    view = buf[1:].view(labels.shape)                                  # does not start on a 16-byte boundary
    assert view.data_ptr() % 16 == 4
    third = region_table(view, topology=True)
    for other in (again, third):
        assert list(other) == list(table)
        for k in table:
            assert np.array_equal(other[k], table[k]), k
    for shape, names in (((6, 7), TOPOLOGY_2D), ((3, 6, 7), TOPOLOGY_3D)):
        empty = region_table(np.zeros(shape, np.int32), None, device, boundary=True, topology=True)
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert empty["euler_number"].dtype == empty["euler_number_conn1"].dtype == np.int64
        assert all(empty[k].dtype == np.float64 for k in names[2:])
    with pytest.raises(ValueError, match="^region_table:"):
        region_table(MAPS["2d"] - 1, None, device, topology=True)
    with pytest.raises(TypeError, match="^region_table:"):
        region_table(MAPS["2d"].astype(np.float32), None, device, topology=True)


def test_measure_topology_end_to_end_and_cli(tmp_path, monkeypatch, device):
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
    seg[0, 0, 13:16, 13:16] = 0                                       # object 11 has a hole: Euler number 0
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
                for name, column in table.items():
                    assert np.array_equal(data[row:row + n, header.index(name)], column.astype(np.float64)), (b, s, name)
                row += n
            assert row == len(data)
        return [open(path, "rb").read() for path in paths]

    measure(config.inference_config)
    plain = check(old_header)
    measure(config.inference_config, topology=True)
    check(old_header + TOPOLOGY_2D, topology=True)
    lines = open(paths[0]).read().splitlines()
    header = lines[0].split(",")
    row = [line.split(",") for line in lines[1:] if line.split(",")[:2] == ["0", "11"]]
    assert len(row) == 1 and row[0][header.index("euler_number")] == "0" and row[0][header.index("euler_number_conn1")] == "0"
    assert row[0][header.index("area")] == "91" and float(row[0][header.index("perimeter_crofton")]) > 36.0
    assert not os.path.exists("contacts_bandwidth-0.csv")
    measure(config.inference_config, contacts=True, topology=True)
    check(old_header + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D, boundary=True, topology=True)
    assert os.path.exists("contacts_bandwidth-0.csv")
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--topology"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + TOPOLOGY_2D, topology=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check(old_header) == plain                                 # without the flag: the same bytes as before
