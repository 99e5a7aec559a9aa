"""The weighted and border columns above the kernels: weighted_moments(), border_intensity() and region_table(weighted=True,
border_intensity=True) against the restatement (tests/weighted_ref.py), and measure(weighted=True, border_intensity=True) / the
command's options end to end.

The device tables are integers and must be EQUAL to the restatement's; the columns are then compared with the restatement's
Fractions rounded once, with == too."""

import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from coloc_ref import round_sqrt, same_floats
from test_gpu_contacts_stage import KEYS_2D, KEYS_3D
from test_gpu_measure_stage import _blob_map, _toml
from weighted_ref import MOMENTS, ref_border, ref_border_columns, ref_max_keys, ref_weighted, ref_weighted_columns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: (g[f"{name}/labels"], g[f"{name}/raw"]) for name in ("2d", "3d")}


G = _fixture()


def _case(name):
    labels, raw = G[name]
    if name == "3d":                                         # two float32 channels, one with negative values
        f = raw.astype(np.float32)
        noise = np.random.default_rng(3).normal(0.0, 2000.0, size=raw.shape).astype(np.float32)
        return labels, np.stack([f * np.float32(0.3) - np.float32(5000.0), np.float32(40000.0) - f / np.float32(7.0) + noise])
    other = np.random.default_rng(2).integers(0, 65536, size=raw.shape).astype(np.uint16)
    return labels, np.stack([raw, (raw // 2 + other // 2).astype(np.uint16)])             # two uint16 channels


def _channel(c):
    return c.astype(np.int32) if c.dtype.kind in "iu" else c


def _shift(channel, npix):
    from cellulus_amd.measure import intensity_shift

    return 0 if channel.dtype.kind in "iu" else intensity_shift(float(np.abs(channel.astype(np.float64)).max()), npix)


_WANT = {}


def want_rows(name, labels, raw, k):
    """(ids, area, sum1, weighted rows, border rows, shift) of the restatement for channel k, computed once per key"""
    if (name, k) not in _WANT:
        labels = np.ascontiguousarray(labels).astype(np.int32)
        nid = int(labels.max()) + 1
        ids = np.unique(labels[labels > 0]).astype(np.int64)
        chan = _channel(raw[k])
        shift = _shift(chan, labels.size)
        rows, bad = ref_weighted(labels, chan, nid, shift, ref_max_keys(labels, chan, nid, shift))
        assert bad == 0
        brows, bad = ref_border(labels, chan, nid, labels.ndim, shift)
        assert bad == 0
        coords = np.indices((1,) * (3 - labels.ndim) + labels.shape).reshape(3, -1)
        flat = labels.reshape(-1)
        area = np.bincount(flat, minlength=nid)[ids]
        sum1 = np.stack([np.bincount(flat, c, minlength=nid).astype(np.int64) for c in coords], axis=1)[ids]       # exact: far below 2^53
        _WANT[name, k] = (ids, area, sum1, [rows[i] for i in ids], [brows[i] for i in ids], shift)
    return _WANT[name, k]


def want_columns(name, labels, raw, weighted, border):
    cols = {}
    nch = raw.shape[0]
    for k in range(nch if weighted else 0):
        ids, area, sum1, rows, _, shift = want_rows(name, labels, raw, k)
        cols.update({n: np.array(v) for n, v in ref_weighted_columns(area, sum1, rows, shift, labels.ndim, k, labels.shape).items()})
    for k in range(nch if border else 0):
        _, _, _, _, brows, shift = want_rows(name, labels, raw, k)
        if k == 0:
            cols["intensity_border_pixels"] = np.array([r[0] for r in brows], dtype=np.int64)
        cols.update({n: np.array(v) for n, v in ref_border_columns(brows, shift, _channel(raw[k]).dtype, k).items()})
    return cols


def _names(nd, nch, weighted, border):
    axes = "zyx"[3 - nd:]
    pairs = ("yy", "xx", "yx") if nd == 2 else ("zz", "yy", "xx", "zy", "zx", "yx")
    out = []
    for k in range(nch if weighted else 0):
        out += ([f"intensity_sum_c{k}"] + [f"centroid_weighted_{a}_c{k}" for a in axes] + [f"cov_weighted_{p}_c{k}" for p in pairs]
                + [f"mass_displacement_c{k}"] + [f"intensity_peak_{a}_c{k}" for a in axes])
    if border:
        out.append("intensity_border_pixels")
    for k in range(nch if border else 0):
        out += [f"intensity_border_{q}_c{k}" for q in ("sum", "mean", "std", "min", "max")]
    return out


def _same(got, want):
    if np.asarray(want).dtype.kind == "f":
        return same_floats(got, want)
    return np.array_equal(got, want)


@pytest.mark.parametrize("name", ["2d", "3d"])
def test_tables_and_columns_equal_restatement(name, device):
    from cellulus_amd.measure import border_intensity, region_table, weighted_moments

    labels, raw = _case(name)
    nd, nch = labels.ndim, raw.shape[0]
    plain = region_table(labels, raw, device)
    assert list(plain) == (KEYS_2D if nd == 2 else KEYS_3D + KEYS_2D[-3:]) + [f"intensity_{q}_c1" for q in ("mean", "min", "max")]
    for k in range(nch):
        wi, area, _, rows, brows, shift = want_rows(name, labels, raw, k)
        ids, table, s = weighted_moments(labels, raw, k, device)
        assert ids.dtype == np.int64 and np.array_equal(ids, wi) and s == shift and list(table) == ["n", "sum_q", "peak"] + list(MOMENTS)
        for w, key in enumerate(table):
            assert [int(v) for v in table[key]] == [r[w] for r in rows], key
        assert table["n"].dtype == np.int64 and np.array_equal(table["n"], area) and table["sum_qx"].dtype == object
        ids, table, s = border_intensity(labels, raw, k, device)
        assert np.array_equal(ids, wi) and s == shift and list(table) == ["pixels", "n", "sum_q", "key_min", "key_max", "sum_qq"]
        for w, key in enumerate(table):
            assert [int(v) for v in table[key]] == [r[w] for r in brows], key
    one_channel = weighted_moments(labels, raw[1], device=device)
    assert [int(v) for v in one_channel[1]["sum_qyx"]] == [r[11] for r in want_rows(name, labels, raw, 1)[3]]
    given = [(labels, raw)]
    if name == "3d":
        given.append((torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(raw).to(device)))
    for weighted, border in ((True, True), (True, False), (False, True)):
        names = _names(nd, nch, weighted, border)
        want = want_columns(name, labels, raw, weighted, border)
        assert list(want) == names
        for lab, r in given:
            table = region_table(lab, r, device, weighted=weighted, border_intensity=border)
            assert list(table) == list(plain) + names            # appended; every old column where it was
            assert all(np.array_equal(plain[k], table[k]) for k in plain)
            for k in names:
                assert table[k].shape == plain["label"].shape and table[k].dtype == want[k].dtype, (k, table[k].dtype, want[k].dtype)
                assert _same(table[k], want[k]), (k, table[k][:4], want[k][:4])
    # against NumPy on the pixels themselves, loosely: these are the quantities they claim to be
    table = region_table(labels, raw, device, weighted=True, border_intensity=True)
    grid = np.indices(labels.shape)
    for row, i in enumerate(plain["label"][:5]):
        m = labels == i
        v = raw[0][m].astype(np.float64)
        assert np.isclose(table["intensity_sum_c0"][row], v.sum(), rtol=1e-5)
        if abs(v.sum()) > 1e-3 * np.abs(v).sum():
            for a, axis in enumerate("zyx"[3 - nd:]):
                assert np.isclose(table[f"centroid_weighted_{axis}_c0"][row], (v * grid[a][m]).sum() / v.sum(), rtol=1e-4, atol=1e-4)
        peak = tuple(table[f"intensity_peak_{axis}_c0"][row] for axis in "zyx"[3 - nd:])
        assert labels[peak] == i and raw[0][peak] == raw[0][m].max()
    if nd == 2:
        with_boundary = region_table(labels, raw, device, boundary=True, border_intensity=True)
        assert np.array_equal(with_boundary["border_pixels"], with_boundary["intensity_border_pixels"])


def test_order_among_the_other_flags_and_call_counts(monkeypatch, device):
    from cellulus_amd import measure
    from cellulus_amd.measure import region_table

    labels, raw = _case("2d")
    names = _names(2, 2, True, True)
    want = want_columns("2d", labels, raw, True, True)
    real = measure._clx.call

    def recorded(**flags):
        calls = []
        monkeypatch.setattr(measure._clx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        table = region_table(labels, raw, device, **flags)
        monkeypatch.undo()
        return table, calls

    others = dict(quantiles=(0.25, 0.5), mad=True, radial=True, radial_rings=2, std=True, colocalization=True)
    rest, rest_calls = recorded(**others)
    full, calls = recorded(weighted=True, border_intensity=True, **others)
    assert calls.count("clx_region_weighted") == 2 and calls.count("clx_region_border_intensity") == 2     # one per channel
    assert [c for c in calls if c not in ("clx_region_weighted", "clx_region_border_intensity")] == rest_calls
    assert calls[-4:] == ["clx_region_weighted"] * 2 + ["clx_region_border_intensity"] * 2
    assert list(full) == list(rest) + names and all(np.array_equal(full[k], rest[k], equal_nan=True) for k in rest)
    assert all(_same(full[k], want[k]) for k in names)
    # with the flags off: no such call, and the calls of the table as it was
    plain, plain_calls = recorded()
    off, off_calls = recorded(weighted=False, border_intensity=False)
    assert off_calls == plain_calls and "clx_region_weighted" not in off_calls and "clx_region_border_intensity" not in off_calls
    assert plain_calls.count("clx_region_moments") == 1 and plain_calls.count("clx_region_intensity") == 2
    assert list(off) == list(plain) == KEYS_2D + [f"intensity_{q}_c1" for q in ("mean", "min", "max")]
    one, one_calls = recorded(weighted=True)
    assert one_calls.count("clx_region_weighted") == 2 and "clx_region_border_intensity" not in one_calls
    assert list(one) == list(plain) + _names(2, 2, True, False)
    single = region_table(labels, raw[0], device, border_intensity=True)
    assert list(single) == KEYS_2D + _names(2, 1, False, True)


def test_errors_and_the_empty_map(monkeypatch, device):
    from cellulus_amd import measure
    from cellulus_amd.measure import border_intensity, region_table, weighted_moments

    labels, raw = _case("2d")
    calls = []
    monkeypatch.setattr(measure._clx, "call", lambda name, *a: calls.append(name))
    for flags in (dict(weighted=True), dict(border_intensity=True)):
        with pytest.raises(ValueError, match="^region_table: weighted and border_intensity need raw"):
            region_table(labels, None, device, **flags)
    with pytest.raises(ValueError, match="^weighted_moments: channel k"):
        weighted_moments(labels, raw, 2, device)
    with pytest.raises(ValueError, match="^border_intensity: raw is needed"):
        border_intensity(labels, None, device=device)
    assert calls == []
    monkeypatch.undo()
    bad = raw.astype(np.float32)
    inside = np.argwhere(labels > 0)
    bad[1][tuple(inside[0])] = np.nan
    for flags in (dict(weighted=True), dict(border_intensity=True)):
        with pytest.raises(ValueError, match="non-finite values inside objects"):
            region_table(labels, bad, device, **flags)
    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zeros = np.zeros(shape, np.int32)
        for dtype in (np.float32, np.uint16):
            empty = region_table(zeros, np.zeros((2,) + shape, dtype), device, weighted=True, border_intensity=True)
            names = _names(len(shape), 2, True, True)
            assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
            for k in names:
                integral = k.startswith("intensity_peak") or k == "intensity_border_pixels"
                raw_typed = k.startswith(("intensity_border_min", "intensity_border_max"))
                assert empty[k].dtype == (np.int64 if integral else (np.float32 if dtype == np.float32 else np.int32) if raw_typed else np.float64), k
        ids, table, shift = weighted_moments(zeros, np.zeros(shape, np.float32), device=device)
        assert ids.shape == (0,) and shift == 0 and all(len(v) == 0 for v in table.values()) and list(table)[:3] == ["n", "sum_q", "peak"]
        ids, table, shift = border_intensity(zeros, np.zeros(shape, np.float32), device=device)
        assert ids.shape == (0,) and shift == 0 and all(len(v) == 0 for v in table.values()) and list(table)[0] == "pixels"
    # a tiny map by hand: object 1 has the values 1 2 / 3 4 at (0,0) (0,1) / (1,0) (1,1), object 2 one pixel of value 5
    lab = np.array([[1, 1, 0], [1, 1, 2]], np.int32)
    one = np.array([[1, 2, 9], [3, 4, 5]], np.float32)
    t = region_table(lab, one, device, weighted=True, border_intensity=True)
    assert t["intensity_sum_c0"].tolist() == [10.0, 5.0]
    assert t["centroid_weighted_y_c0"].tolist() == [0.7, 1.0] and t["centroid_weighted_x_c0"].tolist() == [0.6, 2.0]
    assert t["cov_weighted_yy_c0"].tolist() == [0.21, 0.0] and t["cov_weighted_xx_c0"].tolist() == [0.24, 0.0]
    assert t["cov_weighted_yx_c0"].tolist() == [(10 * 4 - 7 * 6) / 100, 0.0]
    assert t["mass_displacement_c0"].tolist() == [round_sqrt(Fraction(1, 20)), 0.0]      # (0.2, 0.1) off the plain centroid
    assert t["intensity_peak_y_c0"].tolist() == [1, 1] and t["intensity_peak_x_c0"].tolist() == [1, 2]
    assert t["intensity_border_pixels"].tolist() == [4, 1] and t["intensity_border_sum_c0"].tolist() == [10.0, 5.0]
    assert t["intensity_border_mean_c0"].tolist() == [2.5, 5.0] and t["intensity_border_std_c0"].tolist() == [np.sqrt(1.25), 0.0]
    assert t["intensity_border_min_c0"].tolist() == [1.0, 5.0] and t["intensity_border_max_c0"].dtype == np.float32


def test_measure_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(91)
    raw = rng.integers(0, 65536, size=(2, 2, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 9, 92)
    seg[0, 1] = _blob_map((40, 50), 6, 93)
    seg[1, 1] = _blob_map((40, 50), 5, 94)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    paths = [f"measurements_bandwidth-{b}.csv" for b in range(2)]

    def check(**flags):
        for b, path in enumerate(paths):
            header = open(path).readline().strip().split(",")
            data = np.genfromtxt(path, delimiter=",", skip_header=1, dtype=np.float64).reshape(-1, len(header))
            row = 0
            for s in range(2):
                table = region_table(seg[s, b], raw[s], device, **flags)
                assert header == ["sample"] + list(table)
                n = len(table["label"])
                for name, column in table.items():                    # %.17g round-trips a float64, nan reads back as nan
                    assert np.array_equal(data[row:row + n, header.index(name)], column.astype(np.float64), equal_nan=True), (b, s, name)
                row += n
            assert row == len(data)
        return [open(path, "rb").read() for path in paths]

    measure(config.inference_config)
    plain = check()
    measure(config.inference_config, weighted=True, border_intensity=True)
    check(weighted=True, border_intensity=True)
    names = _names(2, 2, True, True)
    header = open(paths[0]).readline().strip().split(",")
    assert header[-len(names):] == names
    want = want_columns("cli", seg[0, 0].astype(np.int32), raw[0], True, True)
    lines = open(paths[0]).read().splitlines()
    rows = [line.split(",") for line in lines[1:] if line.split(",")[0] == "0"]
    for n in names:
        text = [r[header.index(n)] for r in rows]
        assert _same(np.array([float(t) for t in text]), want[n].astype(np.float64)), n
        if want[n].dtype.kind == "f":
            assert text == ["%.17g" % v for v in want[n]], n
        else:
            assert text == ["%d" % v for v in want[n]], n
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--weighted", "--border-intensity"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(weighted=True, border_intensity=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--border-intensity", "--contacts", "--std"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(boundary=True, std=True, border_intensity=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check() == plain                                           # without the options: the same bytes as before
