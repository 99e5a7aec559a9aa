"""Call records of the measure and relate stages, made on the device through the public API alone: with _clx.call wrapped,
every case writes down (a) the ordered library calls it makes -- the entry point, every int / float argument by value, for
every pointer only whether it is NULL (`0`) or not (`p`); utils/otsu.py's clx_minmax_* calls are part of the sequence -- and
(b) what it returns: per array its dtype, shape and the sha256 of its bytes (an object column of Python ints: of their
decimal text), a table's column names in order, or the exception's type and message.  tests/test_gpu_measure_calls.py compares
both with tests/measure_calls.json, in which a text longer than a line is kept as its sha256.

The inputs are formulas, not random numbers, and tiny: the host code above the kernels is what the record pins, and the
kernels are integer-exact.  The record was made before the stage's host code was split into measure_columns.py and folded
around one scene: a refactor of the stage keeps every entry.

    python tests/measure_calls.py --dump DIR      one text file per case
    python tests/measure_calls.py --write         rewrite tests/measure_calls.json (only from a tree whose stage is trusted)
"""

import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), HERE) if p not in sys.path]

from cellulus_amd import _clx                                                   # noqa: E402

RECORD = os.path.join(HERE, "measure_calls.json")
INLINE = 160                            # a text up to this many characters is kept as it is in the JSON


def labels_2d():
    """24 x 40: ids 1 and 2 adjacent rectangles, 4 with a 2 x 2 hole, 5 a single pixel, 7 in a corner; 3 and 6 absent"""
    m = np.zeros((24, 40), dtype=np.int32)
    m[2:10, 2:10] = 1
    m[2:10, 10:16] = 2
    m[12:20, 4:14] = 4
    m[15:17, 8:10] = 0
    m[5, 25] = 5
    m[20:24, 35:40] = 7
    return m


def children_2d():
    """two small boxes inside ids 1 and 4 of labels_2d"""
    m = np.zeros((24, 40), dtype=np.int32)
    m[4:7, 4:7] = 1
    m[13:15, 5:8] = 2
    return m


def labels_3d():
    """5 x 12 x 16: two touching boxes and a single voxel"""
    m = np.zeros((5, 12, 16), dtype=np.int32)
    m[1:4, 2:8, 2:7] = 1
    m[1:4, 2:8, 7:12] = 2
    m[0, 10, 14] = 3
    return m


def channels(shape, nch):
    """(nch, *shape) int64: (37 y + 11 x + 101 c [+ 53 z]) % 251"""
    grid = np.indices(shape, dtype=np.int64)
    y, x = grid[-2], grid[-1]
    z = grid[0] if len(shape) == 3 else 0
    return np.stack([(37 * y + 11 * x + 53 * z + 101 * c) % 251 for c in range(nch)])


def as_float(values, dtype):
    return (values.astype(np.float64) / 8 - 7).astype(dtype)


ALONE = {"boundary": dict(boundary=True), "topology": dict(topology=True), "hull": dict(hull=True), "inscribed": dict(inscribed=True),
         "quantiles": dict(quantiles=(0.25, 0.5), mad=True), "texture": dict(texture=True), "radial": dict(radial=True),
         "radial_wedges": dict(radial=True, radial_wedges=True, radial_width=2), "std": dict(std=True),
         "colocalization": dict(colocalization=True), "weighted": dict(weighted=True), "border_intensity": dict(border_intensity=True)}
ALL_3D = dict(boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.25, 0.5), mad=True, texture=True, radial=True,
              std=True, colocalization=True, weighted=True, border_intensity=True)
ALL_2D = dict(ALL_3D, radial_wedges=True)


def cases():
    """{case id: a function of the device that makes the case's calls and returns its result}"""
    from cellulus_amd import measure as M
    from cellulus_amd import relate as R

    out = {}

    def table(name, labels, raw, flags):
        out[name] = lambda device: M.region_table(labels, raw, device, **flags)

    lab2, u16 = labels_2d(), channels((24, 40), 2).astype(np.uint16)
    f32 = as_float(channels((24, 40), 2), np.float32)
    f32_inf = f32.copy()
    f32_inf[1, 0, 20] = np.inf                               # a background pixel
    assert lab2[0, 20] == 0
    for tag, raw in (("u16", u16), ("f32", f32), ("f32_inf", f32_inf)):
        for flag, kwargs in [("plain", {})] + list(ALONE.items()) + [("all", ALL_2D)]:
            table(f"table/2d_{tag}/{flag}", lab2, raw, kwargs)
    lab3 = labels_3d()
    f64 = as_float(channels((5, 12, 16), 1), np.float64)[0]
    table("table/3d_f64/plain", lab3, f64, {})
    table("table/3d_f64/all", lab3, f64, ALL_3D)                                # one channel has no pair: the error is the record
    table("table/3d_f64/all_but_colocalization", lab3, f64, dict(ALL_3D, colocalization=False))
    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zero, raw = np.zeros(shape, dtype=np.int32), as_float(channels(shape, 2), np.float32)
        tag = "x".join(str(v) for v in shape)
        table(f"table/zero_{tag}/plain", zero, raw, {})
        table(f"table/zero_{tag}/all", zero, raw, ALL_2D if len(shape) == 2 else ALL_3D)
    out["contact_pairs"] = lambda device: M.contact_pairs(lab2, device)
    out["label_distance_sq"] = lambda device: M.label_distance_sq(lab2, device=device)
    out["cooccurrence"] = lambda device: M.cooccurrence(lab2, u16[0], device=device)
    out["radial_distribution"] = lambda device: M.radial_distribution(lab2, u16, device=device)
    out["channel_products"] = lambda device: M.channel_products(lab2, u16, device=device)
    out["channel_products/threshold"] = lambda device: M.channel_products(lab2, u16, threshold=0.15, device=device)
    out["weighted_moments"] = lambda device: M.weighted_moments(lab2, u16, device=device)
    out["border_intensity"] = lambda device: M.border_intensity(lab2, u16, device=device)
    out["label_overlaps"] = lambda device: R.label_overlaps(children_2d(), lab2, device)
    out["relate/clearance"] = lambda device: R.relate(children_2d(), lab2, device, clearance=True)
    return out


def call_line(name, args):
    words = [name]
    for a in args:
        if isinstance(a, ctypes.c_void_p):
            words.append("p" if a.value else "0")
        elif isinstance(a, (int, float)):
            words.append(repr(a))
        else:
            words.append("<%s>" % type(a).__name__)
    return " ".join(words)


def describe(value, lines, prefix=""):
    """one line per leaf of a result: arrays by dtype, shape and hash, tables by their columns in order"""
    if isinstance(value, dict):
        for name, v in value.items():
            describe(v, lines, f"{prefix}{name}: ")
    elif isinstance(value, (tuple, list)):
        lines.append(f"{prefix}{type(value).__name__} of {len(value)}")
        for i, v in enumerate(value):
            describe(v, lines, f"{prefix}[{i}] ")
    elif torch.is_tensor(value):
        describe(value.cpu().numpy(), lines, f"{prefix}tensor ")
    elif isinstance(value, np.ndarray):
        data = " ".join(str(int(v)) for v in value.reshape(-1)).encode() if value.dtype == object else np.ascontiguousarray(value).tobytes()
        lines.append(f"{prefix}{value.dtype} {value.shape} {hashlib.sha256(data).hexdigest()}")
    else:
        lines.append(f"{prefix}{value.item() if isinstance(value, np.generic) else value!r}")


def record(case, device):
    """-> (the calls' text, the result's text) of one case"""
    calls, real = [], _clx.call

    def spy(name, *args):
        calls.append(call_line(name, args))
        return real(name, *args)

    _clx.call = spy
    try:
        lines = []
        try:
            describe(case(device), lines)
        except Exception as e:                               # what the stage raises on an input is part of its behaviour
            lines.append(f"{type(e).__name__}: {e}")
    finally:
        _clx.call = real
    return "\n".join(calls), "\n".join(lines)


def all_records(device):
    return {name: record(case, device) for name, case in cases().items()}


def compact(text):
    if len(text) <= INLINE and "\n" not in text:
        return text
    return "sha256:%s (%d lines)" % (hashlib.sha256(text.encode()).hexdigest(), text.count("\n") + 1)


def compacted(records):
    return {name: {"calls": compact(calls), "result": compact(result)} for name, (calls, result) in sorted(records.items())}


if __name__ == "__main__":
    records_ = all_records(torch.device("cuda", torch.cuda.current_device()))
    if sys.argv[1:2] == ["--dump"] and len(sys.argv) == 3:
        os.makedirs(sys.argv[2], exist_ok=True)
        for key, (calls_, result_) in records_.items():
            with open(os.path.join(sys.argv[2], key.replace("/", "__") + ".txt"), "w") as f:
                f.write(calls_ + "\n--\n" + result_ + "\n")
    elif sys.argv[1:] == ["--write"]:
        with open(RECORD, "w") as f:
            json.dump(compacted(records_), f, indent=0)
            f.write("\n")
    else:
        sys.exit(__doc__)
