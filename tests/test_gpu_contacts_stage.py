"""The boundary quantities above the kernels: region_table(boundary=True) and contact_pairs against the restatements
of tests/contacts_ref.py, and measure(contacts=True) / the command's --contacts end to end."""

import os

import numpy as np
import pytest
import torch

from contacts_ref import ref_boundary_columns
from test_gpu_measure_stage import _blob_map, _toml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARY = ["boundary_faces", "contact_faces", "num_neighbours", "touches_border"]
# what region_table returns without `boundary`, in this order (2-D, one raw channel)
KEYS_2D = ["label", "area", "bbox_min_y", "bbox_min_x", "bbox_max_y", "bbox_max_x", "centroid_y", "centroid_x", "cov_yy", "cov_xx",
           "cov_yx", "cov_eig_0", "cov_eig_1", "equivalent_diameter", "intensity_mean_c0", "intensity_min_c0", "intensity_max_c0"]
KEYS_3D = ["label", "area", "bbox_min_z", "bbox_min_y", "bbox_min_x", "bbox_max_z", "bbox_max_y", "bbox_max_x", "centroid_z",
           "centroid_y", "centroid_x", "cov_zz", "cov_yy", "cov_xx", "cov_zy", "cov_zx", "cov_yx", "cov_eig_0", "cov_eig_1", "cov_eig_2",
           "equivalent_diameter"]


def _maps():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    m = {name: g[f"{name}/labels"] for name in ("2d", "2d_edge", "3d")}
    m["blobs_2d"] = _blob_map((90, 120), 40, 41)
    m["blobs_3d"] = _blob_map((9, 30, 40), 25, 42)
    return m


MAPS = _maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_boundary_columns_equal_restatement(name, device):
    from cellulus_amd.measure import contact_pairs, region_table

    labels = MAPS[name]
    nd = labels.ndim
    plain = region_table(labels, None, device)
    table = region_table(labels, None, device, boundary=True)
    want, (a, b, faces) = ref_boundary_columns(labels)
    extra = BOUNDARY + (["border_pixels", "perimeter"] if nd == 2 else [])
    assert list(table) == list(plain) + extra                          # appended; every old column where it was
    for k in plain:
        assert np.array_equal(plain[k], table[k]), k
    for k in extra:
        if k == "perimeter":
            print(name, "perimeter: largest relative difference",
                  float(np.max(np.abs(table[k] - want[k]) / np.maximum(want[k], 1e-300), initial=0.0)))
            assert np.allclose(table[k], want[k], rtol=1e-14, atol=0)
        else:
            assert table[k].dtype == np.int64 and np.array_equal(table[k], want[k]), k
    got = contact_pairs(labels, device)
    assert all(v.dtype == np.int64 for v in got)
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], faces)
    assert (got[0] < got[1]).all() and (np.diff((got[0] << 32) | got[1]) > 0).all()       # a < b, sorted by (a, b)
    # identities between the columns and the pairs
    to_outside = np.array([int(faces[(a == 0) & (b == i)].sum()) for i in table["label"]], dtype=np.int64)
    assert np.array_equal(table["boundary_faces"], table["contact_faces"] + to_outside)
    assert table["contact_faces"].sum() == 2 * faces[a > 0].sum()
    assert table["num_neighbours"].sum() == 2 * int((a > 0).sum())
    ax = "zyx"[3 - nd:]
    touches = np.zeros(len(table["label"]), dtype=bool)
    for k, c in enumerate(ax):
        touches |= (table[f"bbox_min_{c}"] == 0) | (table[f"bbox_max_{c}"] == labels.shape[k])
    assert np.array_equal(table["touches_border"], touches.astype(np.int64))
    if name == "2d_edge":
        rows = {int(i): r for r, i in enumerate(table["label"])}
        assert table["perimeter"][rows[2]] == pytest.approx(34.41421356237309, rel=1e-14)
        assert table["perimeter"][rows[3]] == 136.0 and table["perimeter"][rows[7]] == 0.0


def test_region_table_without_boundary_keeps_its_keys(device):
    from cellulus_amd.measure import region_table

    raw = np.random.default_rng(43).integers(0, 65536, size=MAPS["2d"].shape).astype(np.uint16)
    assert list(region_table(MAPS["2d"], raw, device)) == KEYS_2D
    assert list(region_table(MAPS["2d"], raw, device, boundary=False)) == KEYS_2D
    assert list(region_table(MAPS["3d"], None, device)) == KEYS_3D
    with_raw = region_table(MAPS["2d"], raw, device, boundary=True)
    assert list(with_raw) == KEYS_2D + BOUNDARY + ["border_pixels", "perimeter"]
    assert list(region_table(MAPS["3d"], None, device, boundary=True)) == KEYS_3D + BOUNDARY


def test_device_tensors_numpy_and_empty(device):
    from cellulus_amd.measure import contact_pairs, region_table

    labels = MAPS["blobs_2d"]
    table = region_table(labels.astype(np.uint16), None, device, boundary=True)
    again = region_table(torch.from_numpy(labels).to(device), boundary=True)
    third = region_table(torch.from_numpy(labels.astype(np.int64)), None, device, boundary=True)
    for other in (again, third):
        assert list(other) == list(table)
        for k in table:
            assert np.array_equal(other[k], table[k]), k
    p0, p1 = contact_pairs(labels, device), contact_pairs(torch.from_numpy(labels).to(device))
    assert all(np.array_equal(x, y) for x, y in zip(p0, p1))
    for shape in ((6, 7), (3, 6, 7)):
        empty = region_table(np.zeros(shape, np.int32), None, device, boundary=True)
        assert all(len(v) == 0 for v in empty.values()) and "boundary_faces" in empty
        assert ("perimeter" in empty) == (len(shape) == 2)
        assert all(len(v) == 0 and v.dtype == np.int64 for v in contact_pairs(np.zeros(shape, np.int32), device))
    with pytest.raises(ValueError):
        contact_pairs(labels - 1, device)
    with pytest.raises(TypeError):
        contact_pairs(labels.astype(np.float32), device)


@pytest.mark.parametrize("name", ["2d", "blobs_2d", "3d"])
def test_device_view_one_element_into_a_buffer(name, device):
    """A contiguous int32 device view that does not start on a 16-byte boundary goes to the kernels as it is (no copy):
    contact_pairs and region_table(boundary=True) accept it and give what the aligned map gives."""
    from cellulus_amd.measure import contact_pairs, region_table

    labels = MAPS[name].astype(np.int32)
    buf = torch.zeros(labels.size + 1, dtype=torch.int32, device=device)
    buf[1:] = torch.from_numpy(labels).to(device).reshape(-1)
    view = buf[1:].view(labels.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    want, (a, b, faces) = ref_boundary_columns(labels)
    got = contact_pairs(view)
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], faces)
    table = region_table(view, boundary=True)
    aligned = region_table(labels, None, device, boundary=True)
    assert list(table) == list(aligned)
    for k in aligned:
        assert np.array_equal(table[k], aligned[k]), k
    for k in want:
        if k != "perimeter":
            assert np.array_equal(table[k], want[k]), k
    # a slice of a volume whose Y * X is no multiple of 4
    if labels.ndim == 3:
        vol = torch.from_numpy(np.pad(labels, ((0, 0), (0, 1), (0, 1)))).to(device)       # 13 x 17 per slice
        assert vol[1].data_ptr() % 16 != 0
        _, (a, b, faces) = ref_boundary_columns(vol[1].cpu().numpy())
        got = contact_pairs(vol[1])
        assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], faces)


def test_messages_name_the_caller(device):
    from cellulus_amd.measure import contact_pairs, region_table

    labels = MAPS["2d"]
    with pytest.raises(ValueError, match="^contact_pairs:"):
        contact_pairs(labels - 1, device)
    with pytest.raises(TypeError, match="^contact_pairs:"):
        contact_pairs(labels.astype(np.float32), device)
    with pytest.raises(ValueError, match="^contact_pairs:"):
        contact_pairs(labels.reshape(-1), device)
    with pytest.raises(ValueError, match="^region_table:"):
        region_table(labels - 1, None, device, boundary=True)


def test_measure_contacts_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import contact_pairs, measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(51)
    raw = rng.integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 9, 52)
    seg[0, 1] = _blob_map((40, 50), 6, 53)
    seg[1, 1] = _blob_map((40, 50), 5, 54)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    old_header = ["sample"] + KEYS_2D
    new_header = old_header + BOUNDARY + ["border_pixels", "perimeter"]

    def check(contacts):
        pairs_seen = 0
        for b in range(2):
            path, pairs_path = f"measurements_bandwidth-{b}.csv", f"contacts_bandwidth-{b}.csv"
            header = open(path).readline().strip().split(",")
            assert header == (new_header if contacts else old_header)
            assert os.path.exists(pairs_path) == contacts
            data = np.genfromtxt(path, delimiter=",", skip_header=1, dtype=np.float64).reshape(-1, len(header))
            row, want_pairs = 0, []
            for s in range(2):
                table = region_table(seg[s, b], raw[s], device, boundary=contacts)
                assert header == ["sample"] + list(table)
                n = len(table["label"])
                for name, column in table.items():
                    assert np.array_equal(data[row:row + n, header.index(name)], column.astype(np.float64)), (b, s, name)
                row += n
                a, bb, faces = contact_pairs(seg[s, b], device)
                want_pairs += [f"{s},{i},{j},{k}" for i, j, k in zip(a, bb, faces) if i > 0]
            assert row == len(data)
            os.remove(path)
            if contacts:
                lines = open(pairs_path).read().splitlines()
                assert lines[0] == "sample,label_a,label_b,faces" and lines[1:] == want_pairs
                pairs_seen += len(want_pairs)
                os.remove(pairs_path)
        assert not contacts or pairs_seen > 0                         # the maps do have objects that touch

    measure(config.inference_config)
    check(False)
    measure(config.inference_config, contacts=True)
    check(True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--contacts"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(False)
