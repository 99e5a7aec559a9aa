"""The measure stage above the kernels: region_table against a plain NumPy table and against scikit-image's
regionprops_table (tests/golden/g13_regionprops.npz), and measure() / the click command end to end."""

import os
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = "zyx"


def _blob_map(shape, n, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.int32)
    grid = np.indices(shape).astype(np.float64)
    for i in range(1, n + 1):
        centre = [rng.uniform(0, s) for s in shape]
        radius = [rng.uniform(1.0, max(2.0, s / 4)) for s in shape]
        lab[sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radius)) <= 1.0] = i
    return lab


def _one_rounding(value, exact):
    exact = Fraction(exact)
    if exact == 0:
        return value == 0.0
    return abs(Fraction(float(value)) - exact) <= abs(exact) * Fraction(1, 2 ** 52)


def _numpy_rows(labels):
    """per label present: (id, points (n, nd) as Python-int sums) from np.argwhere"""
    for i in np.unique(labels):
        if i == 0:
            continue
        yield int(i), np.argwhere(labels == i).astype(np.int64)


def _check_geometry(table, labels):
    nd = labels.ndim
    ax = AXES[3 - nd:]
    rows = list(_numpy_rows(labels))
    assert table["label"].tolist() == [i for i, _ in rows]
    for r, (i, pts) in enumerate(rows):
        n = len(pts)
        assert table["area"][r] == n
        s1 = [int(pts[:, a].sum()) for a in range(nd)]
        cov = np.zeros((nd, nd))
        for a in range(nd):
            assert table[f"bbox_min_{ax[a]}"][r] == pts[:, a].min() and table[f"bbox_max_{ax[a]}"][r] == pts[:, a].max() + 1
            assert _one_rounding(table[f"centroid_{ax[a]}"][r], Fraction(s1[a], n))
            for b in range(a, nd):
                exact = Fraction(n * int((pts[:, a] * pts[:, b]).sum()) - s1[a] * s1[b], n * n)
                assert _one_rounding(table[f"cov_{ax[a]}{ax[b]}"][r], exact), (i, a, b)
                cov[a, b] = cov[b, a] = float(exact)
        eig = np.linalg.eigvalsh(cov)[::-1]
        got = [table[f"cov_eig_{k}"][r] for k in range(nd)]
        assert np.allclose(got, eig, rtol=0, atol=1e-12 * max(1.0, np.trace(cov)))
        d = np.sqrt(4 * n / np.pi) if nd == 2 else np.cbrt(6 * n / np.pi)
        assert table["equivalent_diameter"][r] == pytest.approx(d, rel=1e-15)
    return rows


def test_region_table_2d_two_uint16_channels(device):
    from cellulus_amd.measure import region_table

    labels = _blob_map((48, 61), 12, 21)
    raw = np.random.default_rng(22).integers(0, 65536, size=(2, 48, 61)).astype(np.uint16)
    table = region_table(labels.astype(np.uint16), raw, device)
    rows = _check_geometry(table, labels)
    assert not any(k.endswith("_z") or k in ("cov_zz", "cov_zy", "cov_zx", "cov_eig_2") for k in table)
    for r, (i, pts) in enumerate(rows):
        for k in range(2):
            v = raw[k][labels == i].astype(np.int64)
            assert _one_rounding(table[f"intensity_mean_c{k}"][r], Fraction(int(v.sum()), len(v)))
            assert table[f"intensity_min_c{k}"][r] == v.min() and table[f"intensity_max_c{k}"][r] == v.max()
    # the same table from device tensors, and a single channel given without the channel axis
    again = region_table(torch.from_numpy(labels).to(device), torch.from_numpy(raw.astype(np.int32)).to(device))
    assert list(again) == list(table)
    for k in table:
        assert np.array_equal(again[k], table[k]), k
    single = region_table(labels, raw[1], device)
    assert np.array_equal(single["intensity_mean_c0"], table["intensity_mean_c1"]) and "intensity_mean_c1" not in single


def test_region_table_3d_float32(device):
    from cellulus_amd.measure import intensity_shift, region_table

    labels = _blob_map((10, 14, 18), 8, 23)
    raw = np.random.default_rng(24).normal(10.0, 50.0, size=labels.shape).astype(np.float32)
    table = region_table(labels, raw, device)
    rows = _check_geometry(table, labels)
    shift = intensity_shift(float(np.abs(raw).max()), labels.size)
    for r, (i, pts) in enumerate(rows):
        v = raw[labels == i]
        exact = sum(Fraction(float(x)) for x in v) / len(v)
        # every quantised value is within 2^-(shift+1) of the true one, then one rounding of the division
        assert abs(Fraction(float(table["intensity_mean_c0"][r])) - exact) <= Fraction(1, 2 ** (shift + 1)) + abs(exact) / 2 ** 52
        assert table["intensity_min_c0"][r] == v.min() and table["intensity_max_c0"][r] == v.max()
        assert table["intensity_min_c0"].dtype == np.float32


def test_region_table_errors_and_empty(device):
    from cellulus_amd.measure import region_table

    labels = _blob_map((20, 30), 4, 25)
    with pytest.raises(ValueError):
        region_table(labels - 1, None, device)                       # negative labels
    raw = np.ones(labels.shape, np.float32)
    raw[tuple(np.argwhere(labels > 0)[0])] = np.nan
    with pytest.raises(ValueError):
        region_table(labels, raw, device)
    raw = np.ones(labels.shape, np.float64)
    raw[tuple(np.argwhere(labels == 0)[0])] = np.inf                  # outside every object: not an error
    table = region_table(labels, raw, device)
    assert np.array_equal(table["intensity_mean_c0"], np.ones(len(table["label"])))
    empty = region_table(np.zeros((6, 7), np.int32), np.zeros((2, 6, 7), np.uint8), device)
    assert list(empty)[:2] == ["label", "area"] and all(len(v) == 0 for v in empty.values())
    assert "intensity_max_c1" in empty and "cov_eig_1" in empty


@pytest.mark.parametrize("name", ["2d", "2d_edge", "3d"])
def test_golden_regionprops(name, device):
    """scikit-image 0.18.3's regionprops_table: bbox is half open; inertia_tensor_eigvals equals cov_eig in 2-D and
    trace(cov) − cov_eig[nd−1−i] in 3-D.  Its moments are float sums, ours exact: the bar is 4 x its worst-case
    rounding for the fixture's largest object, area · 2^-52 · extent².  Largest differences observed: eigenvalues
    2.8e-14 (2d_edge, bar 1.2e-10), 7.1e-15 (2d), 1.8e-15 (3d, bar 1.2e-12); centroids and mean intensities 0."""
    from cellulus_amd.measure import region_table

    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    labels, raw = g[f"{name}/labels"], g[f"{name}/raw"]
    nd = labels.ndim
    ax = AXES[3 - nd:]
    t = region_table(labels, raw, device)
    assert np.array_equal(t["label"], g[f"{name}/label"]) and np.array_equal(t["area"], g[f"{name}/area"])
    for i, a in enumerate(ax):
        assert np.array_equal(t[f"bbox_min_{a}"], g[f"{name}/bbox-{i}"])
        assert np.array_equal(t[f"bbox_max_{a}"], g[f"{name}/bbox-{i + nd}"])
    assert np.array_equal(t["intensity_min_c0"], g[f"{name}/min_intensity"])
    assert np.array_equal(t["intensity_max_c0"], g[f"{name}/max_intensity"])
    big = int(np.argmax(t["area"]))
    extent = max(int(t[f"bbox_max_{a}"][big] - t[f"bbox_min_{a}"][big]) for a in ax)
    bar = 4 * float(t["area"][big]) * 2.0 ** -52 * extent ** 2
    eig = np.stack([t[f"cov_eig_{i}"] for i in range(nd)], axis=1)
    want = eig if nd == 2 else eig.sum(axis=1, keepdims=True) - eig[:, ::-1]
    got = np.stack([g[f"{name}/inertia_tensor_eigvals-{i}"] for i in range(nd)], axis=1)
    worst = {"eig": float(np.abs(want - got).max())}
    for i, a in enumerate(ax):
        worst[f"centroid_{a}"] = float(np.abs(t[f"centroid_{a}"] - g[f"{name}/centroid-{i}"]).max())
    worst["mean"] = float(np.abs(t["intensity_mean_c0"] - g[f"{name}/mean_intensity"]).max())
    print(name, "bar", bar, worst)
    assert worst["eig"] <= bar
    assert all(worst[f"centroid_{a}"] <= bar for a in ax)
    assert worst["mean"] <= 4 * float(t["area"][big]) * 2.0 ** -52 * 65535
    assert np.allclose(t["equivalent_diameter"], g[f"{name}/equivalent_diameter"], rtol=4 * 2.0 ** -52, atol=0)


def _toml(container):
    return f"""
[model_config]
num_fmaps = 8
fmap_inc_factor = 2

[inference_config]
num_bandwidths = 2

[inference_config.dataset_config]
container_path = "{container}"
dataset_name = "test/raw"

[inference_config.segmentation_dataset_config]
container_path = "{container}"
dataset_name = "segmentation"
secondary_dataset_name = "detection"
"""


def test_measure_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(31)
    raw = rng.integers(0, 65536, size=(2, 2, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 7, 32)
    seg[0, 1] = _blob_map((40, 50), 5, 33)
    seg[1, 1] = _blob_map((40, 50), 3, 34)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))

    def check():
        for b in range(2):
            path = f"measurements_bandwidth-{b}.csv"
            assert os.path.exists(path)
            header = open(path).readline().strip().split(",")
            data = np.genfromtxt(path, delimiter=",", skip_header=1, dtype=np.float64).reshape(-1, len(header))
            row = 0
            for s in range(2):
                table = region_table(seg[s, b], raw[s], device)
                assert header == ["sample"] + list(table)
                n = len(table["label"])
                if b == 0 and s == 1:
                    assert n == 0
                for name, column in table.items():
                    got = data[row:row + n, header.index(name)]
                    assert np.array_equal(got, column.astype(np.float64)), (b, s, name)     # %.17g round-trips
                assert (data[row:row + n, 0] == s).all()
                row += n
            assert row == len(data)
            os.remove(path)

    measure(config.inference_config)
    check()
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check()
