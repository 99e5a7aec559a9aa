"""CPU tier of csrc/sparse_rows.hip: the NumPy restatement the GPU tests compare with (tests/sparse_rows_ref.py) against
plain per-pixel loops, and the argument refusals of the five entry points through the C ABI — each returns -1 before
any launch, so none of this needs a device."""

import ctypes

import numpy as np
import pytest

from cellulus_amd import _build, _clx
from sparse_rows_ref import changed_rows_loops, changed_rows_ref, changed_tiles_loops, changed_tiles_ref


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("T, C, shape, window, chunk", [
    (3, 1, (1, 5, 9), (1, 3, 3), 2),          # 2-D, a ragged last chunk
    (2, 2, (3, 4, 6), (2, 1, 3), 1),          # 3-D, two channels, KH = 1
    (4, 3, (2, 3, 5), (2, 3, 5), 5),          # the window is the image (one output pixel), chunk > T
])
def test_changed_rows_ref_equals_the_per_pixel_loops(T, C, shape, window, chunk):
    rng = np.random.default_rng(T * 100 + C)
    clean = rng.random((C,) + shape, dtype=np.float32)
    clean[0, 0, 1, 2] = np.nan                                   # the same NaN in every copy: differs from itself
    clean[-1, -1, -1, -1] = 0.0
    noisy = np.repeat(clean[None], T, axis=0)
    noisy[:, -1, -1, -1, -1] = -0.0                              # equals 0.0
    noisy[rng.random(noisy.shape) < 0.06] = 0.5
    noisy[T - 1] = clean                                         # a copy whose only difference is the NaN
    noisy[T - 1, -1, -1, -1, -1] = -0.0
    want, lists = changed_rows_ref(clean, noisy, window, chunk)
    loops = changed_rows_loops(clean, noisy, window, chunk)
    assert len(lists) == len(loops) == -(-T // chunk)
    for got, ref in zip(lists, loops):
        assert got.tolist() == ref
    assert sum(len(x) for x in lists) == int(want.sum()) > 0
    # the NaN pixel is reported in the last copy, the -0.0 pixel is not
    kd, kh, kw = window
    od, oh, ow = want.shape[1:]
    near_nan = np.zeros((od, oh, ow), bool)
    near_nan[0:1, max(0, 1 - kh + 1):2, max(0, 2 - kw + 1):3] = True
    assert np.array_equal(want[T - 1], near_nan)


@pytest.mark.parametrize("T, OH, OW, WH, WW, tile, chunk", [
    (3, 7, 9, 3, 3, 4, 2),                    # 5 x 7 output pixels: clipped bottom and right tiles
    (2, 6, 10, 3, 3, 4, 1),                   # 4 x 8: whole tiles only
    (4, 5, 7, 2, 1, 2, 3),                    # WW = 1, an unequal window
])
def test_changed_tiles_ref_equals_the_per_pixel_loops(T, OH, OW, WH, WW, tile, chunk):
    rng = np.random.default_rng(OH * OW)
    want = rng.random((T, OH, OW)) < 0.04
    want[0] = False
    want[0, OH - 1, OW - 1] = True            # the last row of the last (clipped) window only
    changed, lists = changed_tiles_ref(want, WH, WW, tile, chunk)
    loops = changed_tiles_loops(want, WH, WW, tile, chunk)
    for got, ref in zip(lists, loops):
        assert got.tolist() == ref
    assert changed[0].sum() == 1 and changed[0, -1, -1]
    changed4, lists4 = changed_tiles_ref(want[:, None], WH, WW, tile, chunk)                   # (T, 1, OH, OW) as well
    assert np.array_equal(changed4, changed) and all(np.array_equal(a, b) for a, b in zip(lists4, lists))


# --------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _clx.load()


P = ctypes.c_void_p(4096)          # aligned, never dereferenced: every call below is refused before a launch
OFF4 = ctypes.c_void_p(4100)
NULL = ctypes.c_void_p(0)

# clean, noisy, T, C, ID, IH, IW, KD, KH, KW, chunk, rows, counts, cap, workspace, stream
ROWS_GOOD = [P, P, 4, 1, 3, 16, 70, 1, 3, 3, 2, P, P, 8, P, NULL]
# workspace, T, ID, IH, IW, KD, KH, KW, WH, WW, tile, chunk, tiles, counts, cap, stream
TILES_GOOD = [P, 4, 1, 16, 70, 1, 3, 3, 3, 3, 4, 2, P, P, 8, NULL]
# src, ld_src, rows, n, width, dst, ld_dst, stream
MOVE_GOOD = [P, 12, P, 5, 8, P, 16, NULL]
# src, nfloats, dst, copies, stream
BCAST_GOOD = [P, 16, P, 2, NULL]


def _refused(lib, name, good, change, message):
    args = list(good)
    for i, v in change.items():
        args[i] = v
    assert getattr(lib, name)(*args) == -1
    assert message in lib.clx_last_error().decode()
    with pytest.raises(_clx.ClxError, match=name):
        _clx.call(name, *args)


@pytest.mark.parametrize("change, message", [
    ({0: NULL}, "null pointer"),
    ({1: NULL}, "null pointer"),
    ({11: NULL}, "null pointer"),
    ({12: NULL}, "null pointer"),
    ({14: NULL}, "null pointer"),
    ({2: 0}, "bad extents"),
    ({3: 0}, "bad extents"),
    ({4: 0}, "bad extents"),
    ({5: 0}, "bad extents"),
    ({6: 0}, "bad extents"),
    ({2: -1}, "bad extents"),
    ({9: 64, 6: 200}, "bad window"),              # KW = 64: a window's bits must come from two words
    ({9: 0}, "bad window"),
    ({8: 0}, "bad window"),
    ({7: 0}, "bad window"),
    ({9: 63, 6: 62}, "bad window"),               # larger than the image, in x ...
    ({8: 17}, "bad window"),                      # ... in y ...
    ({7: 4}, "bad window"),                       # ... in z
    ({10: 0}, "bad chunk / capacity"),
    ({13: 0}, "bad chunk / capacity"),
    ({10: -3}, "bad chunk / capacity"),
    ({14: OFF4}, "8-byte aligned"),
])
def test_changed_rows_refuses_bad_arguments(lib, change, message):
    _refused(lib, "clx_changed_rows", ROWS_GOOD, change, message)


@pytest.mark.parametrize("change, message", [
    ({0: NULL}, "null pointer"),
    ({12: NULL}, "null pointer"),
    ({13: NULL}, "null pointer"),
    ({1: 0}, "bad extents"),
    ({3: 0}, "bad extents"),
    ({4: 0}, "bad extents"),
    ({7: 0}, "bad extents"),
    ({2: 2}, "2-D layers only"),                  # OD = 2
    ({2: 3, 5: 2}, "2-D layers only"),            # ID = 3, KD = 2: OD = 2
    ({10: 63}, "bad window / tile"),              # tile + WW - 1 = 65
    ({10: 64, 9: 2}, "bad window / tile"),        # 65 again
    ({8: 15}, "bad window / tile"),               # WH > OH = 14
    ({9: 69}, "bad window / tile"),               # WW > OW = 68
    ({8: 0}, "bad window / tile"),
    ({10: 0}, "bad window / tile"),
    ({11: 0}, "bad chunk / capacity"),
    ({14: 0}, "bad chunk / capacity"),
])
def test_changed_tiles_refuses_bad_arguments(lib, change, message):
    _refused(lib, "clx_changed_tiles", TILES_GOOD, change, message)


@pytest.mark.parametrize("name", ["clx_gather_rows", "clx_scatter_rows"])
@pytest.mark.parametrize("change, message", [
    ({3: -1}, "bad count"),
    ({0: NULL}, "null pointer"),
    ({2: NULL}, "null pointer"),
    ({5: NULL}, "null pointer"),
    ({4: 6}, "multiples of 4"),                   # width % 4
    ({4: 0}, "multiples of 4"),
    ({1: 14}, "multiples of 4"),                  # ld_src % 4
    ({6: 18}, "multiples of 4"),                  # ld_dst % 4
    ({4: 16}, "multiples of 4"),                  # width > ld_src
    ({4: 12, 6: 8}, "multiples of 4"),            # width > ld_dst
    ({0: OFF4}, "16-byte alignment"),
    ({5: OFF4}, "16-byte alignment"),
])
def test_gather_and_scatter_refuse_bad_arguments(lib, name, change, message):
    _refused(lib, name, MOVE_GOOD, change, message)


def test_gather_and_scatter_of_no_rows_is_not_an_error(lib):
    for name in ("clx_gather_rows", "clx_scatter_rows"):
        assert getattr(lib, name)(NULL, 8, NULL, 0, 8, NULL, 8, NULL) == 0


@pytest.mark.parametrize("change, message", [
    ({0: NULL}, "null pointer"),
    ({2: NULL}, "null pointer"),
    ({1: 18}, "bad extents"),                     # nfloats % 4
    ({1: 0}, "bad extents"),
    ({3: 0}, "bad extents"),                      # copies = 0
    ({0: OFF4}, "16-byte alignment"),
    ({2: OFF4}, "16-byte alignment"),
])
def test_broadcast_refuses_bad_arguments(lib, change, message):
    _refused(lib, "clx_broadcast_rows", BCAST_GOOD, change, message)


def test_a_chunk_whose_rows_do_not_fit_31_bits_is_refused(lib):
    """chunk * npix_out >= 2^31 is refused: a row's entry is an int.  One small image, T = 1, a huge chunk: every
    pointer is a real buffer of the size the call asks for (one chunk: one count, `cap` rows, the workspace)."""
    C, shape, window = 1, (1, 11, 10), (1, 3, 3)
    npix_out = 9 * 8
    chunk = -(-2 ** 31 // npix_out)                              # 29826162: the smallest refused one
    assert (chunk - 1) * npix_out < 2 ** 31 <= chunk * npix_out
    clean = np.zeros((C,) + shape, np.float32)
    noisy = np.zeros((1, C) + shape, np.float32)
    rows = np.full(npix_out, -1, np.int32)
    counts = np.full(1, -1, np.int32)
    ws = np.zeros(lib.clx_changed_rows_workspace(1, *shape) // 8, np.uint64)
    args = [clean.ctypes.data_as(ctypes.c_void_p), noisy.ctypes.data_as(ctypes.c_void_p), 1, C, *shape, *window, chunk,
            rows.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p), npix_out,
            ws.ctypes.data_as(ctypes.c_void_p), NULL]
    assert lib.clx_changed_rows(*args) == -1
    assert "must fit 31 bits" in lib.clx_last_error().decode()
    assert (rows == -1).all() and counts[0] == -1 and not ws.any()
    # clx_changed_tiles: chunk * th * tw (2 x 2 tiles of 4 x 4 here)
    tiles = np.full(4, -1, np.int32)
    targs = [ws.ctypes.data_as(ctypes.c_void_p), 1, *shape, *window, 3, 3, 4, 2 ** 29,
             tiles.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p), 4, NULL]
    assert lib.clx_changed_tiles(*targs) == -1
    assert "must fit 31 bits" in lib.clx_last_error().decode()
    assert (tiles == -1).all() and counts[0] == -1
