"""The intensity quantiles and the MAD above the kernel: region_table(quantiles=..., mad=True) against the restatement
(tests/order_ref.py: a plain sort of every object's values, Fractions for the index and the interpolation), and
measure(quantiles=..., mad=True) / the command's --quantiles / --mad end to end.

A selected key is one of the values and the interpolation has one rounding, so every column is compared with ==."""

import os

import numpy as np
import pytest
import torch

from order_ref import ref_columns
from test_gpu_contacts_stage import BOUNDARY, KEYS_2D, KEYS_3D
from test_gpu_hull_stage import HULL_2D
from test_gpu_inscribed_stage import INSCRIBED_2D
from test_gpu_measure_stage import _blob_map, _toml
from test_gpu_topology_stage import TOPOLOGY_2D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0.25, 0.5, 0.75)
NEW = ["intensity_q0.25", "intensity_q0.5", "intensity_q0.75", "intensity_mad"]


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: {k: g[f"{name}/{k}"] for k in ("labels", "raw", "min_intensity", "max_intensity")} for name in ("2d", "2d_edge", "3d")}


G = _fixture()


def _raws(name):
    """the raw inputs of a map: its own uint16, float casts scaled by a non-power-of-two, and two channels"""
    raw = G[name]["raw"]
    return {"uint16": raw, "float32": raw.astype(np.float32) * np.float32(0.3), "float64": raw.astype(np.float64) * 0.7 - 1234.5,
            "two_channels": np.stack([raw, (65535 - raw)])}


_WANT = {}


def want_columns(name, kind):
    """ref_columns for every channel, computed once per input and left unchanged -> {column name: float64}"""
    if (name, kind) not in _WANT:
        raw = _raws(name)[kind]
        channels = raw if kind == "two_channels" else raw[None]
        cols = {}
        for k, channel in enumerate(channels):
            cols.update({f"{n}_c{k}": c for n, c in ref_columns(G[name]["labels"], channel, QS, True).items()})
        for c in cols.values():
            c.setflags(write=False)
        _WANT[name, kind] = cols
    return _WANT[name, kind]


@pytest.mark.parametrize("kind", ["uint16", "float32", "float64", "two_channels"])
@pytest.mark.parametrize("name", sorted(G))
def test_columns_equal_restatement(name, kind, device):
    from cellulus_amd.measure import region_table

    labels, raw = G[name]["labels"], _raws(name)[kind]
    nchan = 2 if kind == "two_channels" else 1
    names = [f"{n}_c{k}" for k in range(nchan) for n in NEW]                          # channel 0 first, the MAD last in a channel
    want = want_columns(name, kind)
    assert list(want) == names
    plain = region_table(labels, raw, device)
    given_raw = raw.astype(np.int32) if raw.dtype == np.uint16 else raw              # torch has no uint16 arithmetic
    for lab, r in ((labels, raw), (torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(given_raw).to(device))):
        table = region_table(lab, r, device, quantiles=QS, mad=True)
        assert list(table) == list(plain) + names                                    # appended; every old column where it was
        for k in plain:
            assert np.array_equal(plain[k], table[k]), k
        for k in names:
            assert table[k].dtype == np.float64 and table[k].shape == plain["label"].shape
            assert np.array_equal(table[k], want[k]), (k, table[k][:4], want[k][:4])
    for k in range(nchan):
        lo, hi = plain[f"intensity_min_c{k}"], plain[f"intensity_max_c{k}"]
        q1, q2, q3 = (table[f"intensity_q{q!r}_c{k}"] for q in QS)
        assert (lo <= q1).all() and (q1 <= q2).all() and (q2 <= q3).all() and (q3 <= hi).all()
        assert (table[f"intensity_mad_c{k}"] >= 0).all()
    # quantiles alone, the MAD alone (it needs the median's ranks itself), the order given
    only = region_table(labels, raw, device, quantiles=(0.75, 0.25))
    assert list(only) == list(plain) + [f"intensity_q{q!r}_c{k}" for k in range(nchan) for q in (0.75, 0.25)]
    assert all(np.array_equal(only[k], table[k]) for k in list(only)[len(plain):])
    only = region_table(labels, raw, device, mad=True)
    assert list(only) == list(plain) + [f"intensity_mad_c{k}" for k in range(nchan)]
    assert all(np.array_equal(only[k], table[k]) for k in list(only)[len(plain):])


@pytest.mark.parametrize("name", sorted(G))
def test_uint16_against_numpy_and_the_fixture(name, device):
    from cellulus_amd.measure import region_table

    labels, raw = G[name]["labels"], G[name]["raw"]
    table = region_table(labels, raw, device, quantiles=(0.0, 0.5, 1.0), mad=True)
    assert list(table)[-4:] == ["intensity_q0.0_c0", "intensity_q0.5_c0", "intensity_q1.0_c0", "intensity_mad_c0"]
    assert np.array_equal(table["intensity_q0.0_c0"], G[name]["min_intensity"])
    assert np.array_equal(table["intensity_q1.0_c0"], G[name]["max_intensity"])
    values = [raw[labels == i].astype(np.int64) for i in table["label"]]
    assert np.array_equal(table["intensity_q0.5_c0"], [np.median(v) for v in values])
    assert np.array_equal(table["intensity_mad_c0"], [np.median(np.abs(v - np.median(v))) for v in values])
    assert np.array_equal(table["intensity_q0.5_c0"], want_columns(name, "uint16")["intensity_q0.5_c0"])


def test_other_flags_keys_and_bad_arguments(device):
    from cellulus_amd.measure import region_table

    labels, raw = G["2d"]["labels"], G["2d"]["raw"]
    names = [f"{n}_c0" for n in NEW]
    # without the new arguments the key lists are what they were
    assert list(region_table(labels, raw, device)) == KEYS_2D
    assert list(region_table(labels, raw, device, quantiles=None, mad=False)) == KEYS_2D
    assert list(region_table(labels, raw, device, quantiles=())) == KEYS_2D
    assert list(region_table(G["3d"]["labels"], None, device)) == KEYS_3D
    assert list(region_table(G["3d"]["labels"], G["3d"]["raw"], device, quantiles=QS, mad=True))[len(KEYS_3D) + 3:] == names
    # with all four other flags: the new columns come last, every other column is what it was
    rest = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True)
    assert list(rest) == KEYS_2D + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D + HULL_2D + INSCRIBED_2D
    full = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True, quantiles=QS, mad=True)
    assert list(full) == list(rest) + names
    for k in rest:
        assert np.array_equal(full[k], rest[k]), k
    want = want_columns("2d", "uint16")
    for k in names:
        assert np.array_equal(full[k], want[k]), k
    # a view that does not start on a 16-byte boundary
    buf = torch.zeros(labels.size + 1, dtype=torch.int32, device=device)
    buf[1:] = torch.from_numpy(labels.astype(np.int32)).to(device).reshape(-1)
    rbuf = torch.zeros(labels.size + 1, dtype=torch.float32, device=device)
    rbuf[1:] = torch.from_numpy(_raws("2d")["float32"]).to(device).reshape(-1)
    other = region_table(buf[1:].view(labels.shape), rbuf[1:].view(labels.shape), quantiles=QS, mad=True)
    want = want_columns("2d", "float32")
    assert all(np.array_equal(other[k], want[k]) for k in names)
    # bad arguments
    for quantiles in ((0.5, float("nan")), (-0.25,), (1.5,), (0.5, 0.5), tuple(np.linspace(0, 1, 17))):
        with pytest.raises(ValueError, match="^region_table:.*quantile"):
            region_table(labels, raw, device, quantiles=quantiles)
    for kw in (dict(quantiles=QS), dict(mad=True)):
        with pytest.raises(ValueError, match="^region_table:.*need raw"):
            region_table(labels, None, device, **kw)
    bad = _raws("2d")["float32"].copy()
    bad[tuple(np.argwhere(labels > 0)[0])] = np.nan
    with pytest.raises(ValueError, match="non-finite values inside objects"):
        region_table(labels, bad, device, quantiles=QS)
    with pytest.raises(ValueError, match="must fit in int32"):
        region_table(labels, raw.astype(np.int64) << 20, device, quantiles=QS)
    # 16 quantiles are accepted: 32 ranks in one call
    many = tuple(float(q) for q in np.linspace(0, 1, 16))
    table = region_table(labels, raw, device, quantiles=many)
    assert np.array_equal(table["intensity_q0.0_c0"], G["2d"]["min_intensity"]) and np.array_equal(table["intensity_q1.0_c0"], G["2d"]["max_intensity"])
    ref = ref_columns(labels, raw, many, False)
    assert all(np.array_equal(table[f"{k}_c0"], ref[k]) for k in ref)


@pytest.mark.parametrize("name", sorted(G))
def test_sixteen_quantiles_without_the_median_and_mad(name, device):
    """16 quantiles, none of them 0.5, and the MAD: 17 pairs of ranks, more than one clx_region_order_stats call takes"""
    from cellulus_amd.measure import region_table

    labels = G[name]["labels"]
    many = tuple(float(q) for q in np.linspace(0, 1, 16))
    assert len(many) == 16 and 0.5 not in many
    for kind in ("uint16", "float32", "two_channels"):
        raw = _raws(name)[kind]
        channels = raw if kind == "two_channels" else raw[None]
        plain = region_table(labels, raw, device)
        table = region_table(labels, raw, device, quantiles=many, mad=True)
        names = [f"{n}_c{k}" for k in range(len(channels)) for n in [f"intensity_q{q!r}" for q in many] + ["intensity_mad"]]
        assert list(table) == list(plain) + names
        for k, channel in enumerate(channels):
            want = ref_columns(labels, channel, many, True)
            for n, column in want.items():
                assert np.array_equal(table[f"{n}_c{k}"], column), (kind, n, k)
            assert np.array_equal(table[f"intensity_mad_c{k}"], want_columns(name, kind)[f"intensity_mad_c{k}"])
    # 16 quantiles with 0.5 among them and the MAD: one call
    with_median = many[:15] + (0.5,)
    table = region_table(labels, G[name]["raw"], device, quantiles=with_median, mad=True)
    want = ref_columns(labels, G[name]["raw"], with_median, True)
    assert all(np.array_equal(table[f"{n}_c0"], column) for n, column in want.items())


def test_negative_zero_is_zero(device):
    from cellulus_amd.measure import region_table

    labels, raw = G["2d"]["labels"], G["2d"]["raw"]
    table = region_table(labels, raw, device, quantiles=(-0.0, 1.0))
    assert list(table)[-2:] == ["intensity_q0.0_c0", "intensity_q1.0_c0"]
    assert np.array_equal(table["intensity_q0.0_c0"], G["2d"]["min_intensity"])
    with pytest.raises(ValueError, match="^region_table:.*distinct"):
        region_table(labels, raw, device, quantiles=(0.0, -0.0))


def test_maps_without_objects_and_single_pixels(device):
    from cellulus_amd.measure import region_table

    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zeros = np.zeros(shape, np.int32)
        empty = region_table(zeros, np.zeros((2,) + shape, np.float32), device, boundary=True, topology=True, hull=True, inscribed=True,
                             quantiles=QS, mad=True)
        names = [f"{n}_c{k}" for k in range(2) for n in NEW]
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert all(empty[k].dtype == np.float64 for k in names)
    lab = np.array([[0, 3, 0], [1, 1, 0]], np.int32)
    raw = np.array([[9.0, -0.0, 9.0], [2.0, 5.0, 9.0]], np.float32)
    t = region_table(lab, raw, device, quantiles=(0.0, 0.3, 1.0), mad=True)
    assert t["label"].tolist() == [1, 3]
    assert t["intensity_q0.0_c0"].tolist() == [2.0, 0.0] and t["intensity_q1.0_c0"].tolist() == [5.0, 0.0]
    assert t["intensity_q0.3_c0"].tolist() == [float(2 + 3 * __import__("fractions").Fraction(0.3)), 0.0]
    assert t["intensity_mad_c0"].tolist() == [1.5, 0.0]


def test_measure_quantiles_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(71)
    raw = rng.integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 9, 72)
    seg[0, 1] = _blob_map((40, 50), 6, 73)
    seg[1, 1] = _blob_map((40, 50), 5, 74)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    old_header = ["sample"] + KEYS_2D
    names = [f"{n}_c0" for n in NEW]
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
    measure(config.inference_config, quantiles=QS, mad=True)
    check(old_header + names, quantiles=QS, mad=True)
    want = ref_columns(seg[0, 0], raw[0, 0], QS, True)
    lines = open(paths[0]).read().splitlines()
    header = lines[0].split(",")
    rows = [line.split(",") for line in lines[1:] if line.split(",")[0] == "0"]
    for n in NEW:
        assert [float(r[header.index(f"{n}_c0")]) for r in rows] == want[n].tolist()
    everything = old_header + BOUNDARY + ["border_pixels", "perimeter"] + TOPOLOGY_2D + HULL_2D + INSCRIBED_2D + names
    measure(config.inference_config, contacts=True, topology=True, hull=True, inscribed=True, quantiles=QS, mad=True)
    check(everything, boundary=True, topology=True, hull=True, inscribed=True, quantiles=QS, mad=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--quantiles", "0.25,0.5,0.75", "--mad"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + names, quantiles=QS, mad=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--quantiles", "0.25,0.5,0.75", "--mad", "--contacts", "--topology", "--hull",
                                           "--inscribed"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(everything, boundary=True, topology=True, hull=True, inscribed=True, quantiles=QS, mad=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--quantiles", "0.5"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + ["intensity_q0.5_c0"], quantiles=(0.5,))
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check(old_header) == plain                                 # without the flags: the same bytes as before
