"""The inscribed circle / ball above the kernels: label_distance_sq and region_table(inscribed=True) against the restatement
(tests/inscribed_ref.py), and measure(inscribed=True) / the command's --inscribed end to end.

The columns are formed by the same host function from integers that must be equal, so they are compared with ==."""

import os

import numpy as np
import pytest
import torch

from inscribed_ref import DIST_INF, ref_distance_sq, ref_inscribed
from test_gpu_contacts_stage import BOUNDARY, KEYS_2D, KEYS_3D
from test_gpu_hull_stage import HULL_2D, HULL_3D
from test_gpu_measure_stage import _blob_map, _toml
from test_gpu_topology_stage import TOPOLOGY_2D, TOPOLOGY_3D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSCRIBED_2D = ["inscribed_radius", "inscribed_centre_y", "inscribed_centre_x", "distance_sq_mean"]
INSCRIBED_3D = ["inscribed_radius", "inscribed_centre_z", "inscribed_centre_y", "inscribed_centre_x", "distance_sq_mean"]


def _maps():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: g[f"{name}/labels"] for name in ("2d", "2d_edge", "3d")}


MAPS = _maps()
WANT = {(name, edge): ref_distance_sq(labels, edge) for name, labels in MAPS.items() for edge in (False, True)}   # read by every test


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_distance_map_and_columns_equal_restatement(name, edge, device):
    from cellulus_amd.measure import inscribed_columns, label_distance_sq, region_table

    labels = MAPS[name]
    nd = labels.ndim
    want_map = WANT[name, edge]
    for given in (labels, torch.from_numpy(labels.astype(np.int64)).to(device)):
        dist = label_distance_sq(given, edge=edge, device=device)
        assert torch.is_tensor(dist) and dist.is_cuda and dist.dtype == torch.int32 and tuple(dist.shape) == labels.shape
        assert np.array_equal(dist.cpu().numpy(), want_map)
    plain = region_table(labels, None, device)
    extra = INSCRIBED_2D if nd == 2 else INSCRIBED_3D
    rows, _ = ref_inscribed(labels, want_map, int(labels.max()) + 1)
    for given in (labels, torch.from_numpy(labels.astype(np.int32)).to(device)):
        table = region_table(given, None, device, inscribed=True, edge=edge)
        assert list(table) == list(plain) + extra                       # appended; every old column where it was
        for k in plain:
            assert np.array_equal(plain[k], table[k]), k
        want = inscribed_columns(table["area"], rows[table["label"]], labels.shape, nd)
        assert list(want) == extra and len(table["label"]) == len(np.unique(labels[labels > 0]))
        for k in extra:
            assert table[k].dtype == (np.int64 if "centre" in k else np.float64)
            assert np.array_equal(table[k], want[k]), k
    assert (table["inscribed_radius"] >= 1.0).all() and np.isfinite(table["inscribed_radius"]).all()
    assert (table["distance_sq_mean"] >= 1.0).all() and (table["distance_sq_mean"] <= np.rint(table["inscribed_radius"] ** 2)).all()
    centre = tuple(table[f"inscribed_centre_{a}"] for a in "zyx"[3 - nd:])
    assert np.array_equal(labels[centre], table["label"])               # the centre is a pixel of the object
    assert np.array_equal(want_map[centre].astype(np.float64), np.rint(table["inscribed_radius"] ** 2))
    # with the other flags and a raw channel: the inscribed columns come last, everything else is what it was
    raw = np.random.default_rng(44).integers(0, 65536, size=labels.shape).astype(np.uint16)
    full = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True, edge=edge)
    rest = region_table(labels, raw, device, boundary=True, topology=True, hull=True)
    assert list(full) == list(rest) + extra
    for k in rest:
        assert np.array_equal(full[k], rest[k]), k
    for k in extra:
        assert np.array_equal(full[k], table[k]), k


def test_region_table_without_inscribed_keeps_its_keys(device):
    from cellulus_amd.measure import region_table

    raw = np.random.default_rng(43).integers(0, 65536, size=MAPS["2d"].shape).astype(np.uint16)
    assert list(region_table(MAPS["2d"], raw, device)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, inscribed=False, edge=True)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, False, False, False, False)) == KEYS_2D
    assert list(region_table(MAPS["3d"], None, device)) == KEYS_3D
    assert list(region_table(MAPS["2d"], raw, device, inscribed=True)) == KEYS_2D + INSCRIBED_2D
    assert list(region_table(MAPS["2d"], raw, device, hull=True, inscribed=True)) == KEYS_2D + HULL_2D + INSCRIBED_2D
    assert list(region_table(MAPS["2d"], raw, device, True, True, True, True)) == (
        KEYS_2D + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D + HULL_2D + INSCRIBED_2D)
    assert list(region_table(MAPS["3d"], None, device, boundary=True, topology=True, hull=True, inscribed=True)) == (
        KEYS_3D + BOUNDARY + TOPOLOGY_3D + HULL_3D + INSCRIBED_3D)


def test_views_empty_background_and_one_object_maps(device):
    from cellulus_amd.measure import label_distance_sq, region_table

    labels = MAPS["2d_edge"]
    table = region_table(labels.astype(np.uint16), None, device, inscribed=True)
    buf = torch.zeros(labels.size + 1, dtype=torch.int32, device=device)
    buf[1:] = torch.from_numpy(labels.astype(np.int32)).to(device).reshape(-1)
    view = buf[1:].view(labels.shape)                                  # does not start on a 16-byte boundary
    assert view.data_ptr() % 16 == 4
    other = region_table(view, inscribed=True)
    assert list(other) == list(table) and all(np.array_equal(other[k], table[k]) for k in table)
    assert np.array_equal(label_distance_sq(view).cpu().numpy(), WANT["2d_edge", False])
    for shape, names in (((6, 7), INSCRIBED_2D), ((3, 6, 7), INSCRIBED_3D), ((0, 5), INSCRIBED_2D)):
        zeros = np.zeros(shape, np.int32)
        empty = region_table(zeros, None, device, boundary=True, topology=True, hull=True, inscribed=True)
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert all(empty[k].dtype == (np.int64 if "centre" in k else np.float64) for k in names)
        for edge in (False, True):
            dist = label_distance_sq(zeros, edge=edge, device=device)
            assert dist.is_cuda and dist.dtype == torch.int32 and tuple(dist.shape) == shape and not dist.any()
    # one object everywhere: nothing to measure to without `edge`
    full = np.full((5, 5), 3, np.int32)
    assert (label_distance_sq(full, device=device).cpu().numpy() == DIST_INF).all()
    t = region_table(full, None, device, inscribed=True)
    assert t["inscribed_radius"].tolist() == [np.inf] and t["distance_sq_mean"].tolist() == [np.inf]
    assert t["inscribed_centre_y"].tolist() == [0] and t["inscribed_centre_x"].tolist() == [0]
    t = region_table(full, None, device, inscribed=True, edge=True)
    assert t["inscribed_radius"].tolist() == [3.0] and t["distance_sq_mean"].tolist() == [57 / 25]
    assert t["inscribed_centre_y"].tolist() == [2] and t["inscribed_centre_x"].tolist() == [2]
    with pytest.raises(ValueError, match="^label_distance_sq:"):
        label_distance_sq(MAPS["2d"] - 1, device=device)
    with pytest.raises(TypeError, match="^label_distance_sq:"):
        label_distance_sq(MAPS["2d"].astype(np.float32), device=device)


def test_measure_inscribed_end_to_end_and_cli(tmp_path, monkeypatch, device):
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
    seg[0, 0, 10:21, 10:17] = 11                                      # an 11 x 7 box away from the edge: the largest circle has
    seg[0, 0, 9, :] = seg[0, 0, 21, :] = 0                            # radius 4, first attained at (13, 13)
    seg[0, 0, :, 9] = seg[0, 0, :, 17] = 0
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
    measure(config.inference_config, inscribed=True)
    check(old_header + INSCRIBED_2D, inscribed=True)                  # measure() uses edge=False, region_table's default
    lines = open(paths[0]).read().splitlines()
    header = lines[0].split(",")
    row = [line.split(",") for line in lines[1:] if line.split(",")[:2] == ["0", "11"]]
    assert len(row) == 1 and row[0][header.index("area")] == "77"
    assert float(row[0][header.index("inscribed_radius")]) == 4.0
    assert (row[0][header.index("inscribed_centre_y")], row[0][header.index("inscribed_centre_x")]) == ("13", "13")
    box = np.zeros((13, 9), np.int32)
    box[1:12, 1:8] = 1
    assert float(row[0][header.index("distance_sq_mean")]) == int(ref_distance_sq(box, False).sum()) / 77
    measure(config.inference_config, contacts=True, topology=True, hull=True, inscribed=True)
    check(old_header + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D + HULL_2D + INSCRIBED_2D, boundary=True, topology=True,
          hull=True, inscribed=True)
    assert os.path.exists("contacts_bandwidth-0.csv")
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--inscribed"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + INSCRIBED_2D, inscribed=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--inscribed", "--hull", "--contacts"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + BOUNDARY + ["border_pixels", "perimeter"] + HULL_2D + INSCRIBED_2D, boundary=True, hull=True, inscribed=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check(old_header) == plain                                 # without the flag: the same bytes as before
