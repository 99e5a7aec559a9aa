"""CPU tier of the measure stage (no kernel is launched): the intensity scale, the host arithmetic that turns
integer moments into the table's columns, the C-ABI symbols and the entry points."""

import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DENORMAL = 5e-324
MAX_ABS = ([0.0, DENORMAL, 3.4e38, 1e308]
           + [2.0 ** k for k in (-1022, -149, -20, -1, 0, 1, 10, 127, 1023)]
           + [float(np.nextafter(2.0 ** k, 0.0)) for k in (-1022, -149, -20, -1, 0, 1, 10, 127, 1023)])
NPIX = [1, 2 ** 32 - 1] + [2 ** k for k in (1, 12, 24, 31)] + [2 ** k - 1 for k in (1, 12, 24, 31)]


def _round_half_even(fr):
    fl = fr.numerator // fr.denominator
    rem = fr - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2):
        return fl + 1
    return fl


@pytest.mark.parametrize("npix", NPIX)
def test_intensity_shift_fits_and_is_tight(npix):
    from cellulus_amd.measure import intensity_shift

    bound = 2 ** 62 >> int(npix).bit_length()
    for max_abs in MAX_ABS:
        shift = intensity_shift(max_abs, npix)
        assert isinstance(shift, int)
        if max_abs == 0.0:
            assert shift == 0
            continue
        scaled = Fraction(max_abs) * Fraction(2) ** shift
        assert math.ceil(scaled) * npix < 2 ** 62, (max_abs, npix, shift)
        assert _round_half_even(scaled) <= bound
        assert math.isfinite(math.ldexp(max_abs, shift)) and math.isfinite(2.0 ** shift)
        clamped = shift in (-1022, 1023)
        if not clamped:
            # one more bit would break the kernel's per-pixel bound |q| <= 2^62 >> bit_length(npix)
            assert _round_half_even(scaled * 2) > bound, (max_abs, npix, shift)
    assert intensity_shift(DENORMAL, npix) == 1023                       # the clamp
    for wrong in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            intensity_shift(wrong, npix)


def _box_moments(origin, size):
    """Hand-written integer moments of a filled box: (area, bbox, sum1, sum2), axes z y x."""
    coords = [range(o, o + s) for o, s in zip(origin, size)]
    area = size[0] * size[1] * size[2]
    s1 = [sum(c) * area // len(c) for c in coords]
    sq = [sum(v * v for v in c) * area // len(c) for c in coords]
    cross = [sum(coords[a]) * sum(coords[b]) * area // (len(coords[a]) * len(coords[b])) for a, b in ((0, 1), (0, 2), (1, 2))]
    bbox = list(origin) + [o + s - 1 for o, s in zip(origin, size)]
    return area, bbox, s1, sq + cross


def _one_rounding(value, exact):
    """|value - exact| within one float64 rounding of the exact rational."""
    exact = Fraction(exact)
    if exact == 0:
        return value == 0.0
    return abs(Fraction(float(value)) - exact) <= abs(exact) * Fraction(1, 2 ** 52)


@pytest.mark.parametrize("origin,size", [((0, 0, 0), (1, 5, 9)), ((0, 3, 1000), (1, 12, 7)), ((0, 4095, 4000), (1, 1, 96)),
                                         ((0, 100000, 3), (1, 30, 30))])
def test_shape_columns_rectangle_2d(origin, size):
    from cellulus_amd.measure import shape_columns

    area, bbox, s1, s2 = _box_moments(origin, size)
    c = shape_columns([7], [area], [bbox], [s1], [s2], 2)
    _, h, w = size
    assert not any("z" in k.split("_")[-1] for k in c if k.startswith(("bbox", "centroid", "cov_")))     # no z in 2-D
    assert c["label"].tolist() == [7] and c["area"].tolist() == [h * w]
    assert c["bbox_min_y"][0] == origin[1] and c["bbox_max_y"][0] == origin[1] + h
    assert c["bbox_min_x"][0] == origin[2] and c["bbox_max_x"][0] == origin[2] + w
    assert _one_rounding(c["centroid_y"][0], origin[1] + Fraction(h - 1, 2))
    assert _one_rounding(c["centroid_x"][0], origin[2] + Fraction(w - 1, 2))
    assert _one_rounding(c["cov_yy"][0], Fraction(h * h - 1, 12))
    assert _one_rounding(c["cov_xx"][0], Fraction(w * w - 1, 12))
    assert c["cov_yx"][0] == 0.0
    hi, lo = max(h, w), min(h, w)
    assert c["cov_eig_0"][0] == pytest.approx((hi * hi - 1) / 12, rel=1e-14)
    assert c["cov_eig_1"][0] == pytest.approx((lo * lo - 1) / 12, rel=1e-14, abs=1e-300)
    assert c["equivalent_diameter"][0] == pytest.approx(math.sqrt(4 * h * w / math.pi), rel=1e-15)


def test_shape_columns_one_pixel_and_box_3d():
    from cellulus_amd.measure import shape_columns

    one = _box_moments((3, 17, 250), (1, 1, 1))
    box = _box_moments((2, 40, 1000), (4, 6, 11))
    for nd in (2, 3):
        c = shape_columns([1, 9], [one[0], box[0]], [one[1], box[1]], [one[2], box[2]], [one[3], box[3]], nd)
        names = [k for k in c if k.startswith("cov_")]
        assert len(names) == (3 + 2 if nd == 2 else 6 + 3)
        for k in names:
            assert c[k][0] == 0.0, k                                     # a single pixel has no extent
        assert c["centroid_y"][0] == 17.0 and c["centroid_x"][0] == 250.0
    assert c["centroid_z"][0] == 3.0 and c["bbox_min_z"][0] == 3 and c["bbox_max_z"][0] == 4
    assert _one_rounding(c["centroid_z"][1], 2 + Fraction(3, 2))
    assert _one_rounding(c["centroid_y"][1], 40 + Fraction(5, 2))
    assert _one_rounding(c["centroid_x"][1], 1005)
    assert _one_rounding(c["cov_zz"][1], Fraction(15, 12))
    assert _one_rounding(c["cov_yy"][1], Fraction(35, 12))
    assert _one_rounding(c["cov_xx"][1], Fraction(120, 12))
    assert c["cov_zy"][1] == 0.0 and c["cov_zx"][1] == 0.0 and c["cov_yx"][1] == 0.0
    assert [c[f"cov_eig_{i}"][1] for i in range(3)] == pytest.approx([10.0, 35 / 12, 15 / 12], rel=1e-14)
    assert c["equivalent_diameter"][1] == pytest.approx((6 * 264 / math.pi) ** (1 / 3), rel=1e-15)
    assert c["bbox_max_z"][1] == 6 and c["bbox_max_y"][1] == 46 and c["bbox_max_x"][1] == 1011


def test_shape_columns_no_cancellation_far_from_origin():
    """area·Σab − Σa·Σb is formed in integers: a 2 x 3 object at x ~ 2^30 still has the exact covariance, which float64
    sums of x² (~2^60) could not give."""
    from cellulus_amd.measure import shape_columns

    area, bbox, s1, s2 = _box_moments((0, 2 ** 30, 2 ** 30 + 5), (1, 2, 3))
    c = shape_columns([1], [area], [bbox], [s1], [s2], 2)
    assert _one_rounding(c["cov_yy"][0], Fraction(3, 12)) and _one_rounding(c["cov_xx"][0], Fraction(8, 12))
    assert c["cov_yx"][0] == 0.0


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name in ("clx_region_moments", "clx_region_intensity"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES
    assert len(_clx.PROTOTYPES["clx_region_moments"][1]) == 11
    assert len(_clx.PROTOTYPES["clx_region_intensity"][1]) == 10
    assert _clx.load().clx_abi_version() == 13


def test_cli_command_and_scripts(tmp_path):
    import click
    import tomli
    from click.testing import CliRunner

    from cellulus_amd import cli

    assert isinstance(cli.measure, click.Command)
    res = CliRunner().invoke(cli.measure, [str(tmp_path / "missing.toml")])
    assert res.exit_code != 0 and "does not exist" in res.output
    doc = tomli.load(open(os.path.join(ROOT, "pyproject.toml"), "rb"))
    assert doc["project"]["scripts"] == {"train": "cellulus_amd.cli:train", "infer": "cellulus_amd.cli:infer"}
    import cellulus_amd.infer as infer_module
    assert "measure" not in open(infer_module.__file__).read()           # infer() does not call the new stage


def test_region_table_has_no_cpu_path():
    from cellulus_amd._clx import ClxError
    from cellulus_amd.measure import region_table

    labels = torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ClxError):
        region_table(labels, device="cpu")
    with pytest.raises(ClxError):
        region_table(labels.numpy(), device=torch.device("cpu"))
    if not torch.cuda.is_available():
        with pytest.raises(ClxError):
            region_table(labels)
        with pytest.raises(ClxError):
            region_table(labels.numpy(), raw=np.zeros((4, 5), np.float32))
