"""clx_changed_rows, clx_changed_tiles, clx_gather_rows, clx_scatter_rows and clx_broadcast_rows (csrc/sparse_rows.hip)
through the C ABI against the NumPy restatement (tests/sparse_rows_ref.py), at the widths where the 64-bit word
arithmetic of the kernels takes another branch: rows of exactly one, two and three words, one pixel more, one less, input
rows with more words than output rows, windows up to 63 wide, chunks that end inside a wavefront, lists longer than their
capacity, grids above the launch cap.  Integer lists and moved bits: every comparison is EQUALITY.  Each output (rows,
counts, tiles, the workspace at exactly the size clx_changed_rows_workspace names) has a sentinel-filled tail that must
come back unchanged, and list slots past a chunk's count keep their sentinel.

And the infer-mode forward end to end at those widths: the sparse path's embeddings equal the dense path's bit for bit."""

import ctypes

import numpy as np
import pytest
import torch

from sparse_rows_ref import changed_rows_ref, changed_tiles_ref, out_extents

pytestmark = pytest.mark.gpu

SENT = -7                        # fills every list and count before a call
FSENT = -123.0                   # ... and every float destination
TAIL = 64                        # sentinel entries behind every list / count buffer
WS_TAIL = 256                    # 0xAB bytes behind the workspace
NULL = ctypes.c_void_p(0)


def _clx():
    from cellulus_amd import _clx
    return _clx


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ============================================================================================================ running
def run_rows(device, clean, noisy, window, chunk, cap=None):
    """clx_changed_rows -> (counts (nchunks,), slots (nchunks, cap), workspace tensor); the tails are checked here"""
    clx = _clx()
    T, C, ID, IH, IW = noisy.shape
    npix = int(np.prod(out_extents((ID, IH, IW), window)))
    nchunks = -(-T // chunk)
    if cap is None:
        cap = min(chunk, T) * npix
    rows = torch.full((nchunks * cap + TAIL,), SENT, dtype=torch.int32, device=device)
    counts = torch.full((nchunks + TAIL,), SENT, dtype=torch.int32, device=device)
    nbytes = int(clx.load().clx_changed_rows_workspace(T, ID, IH, IW))
    assert nbytes == 2 * T * ID * IH * ((IW + 63) // 64) * 8
    ws = torch.full((nbytes + WS_TAIL,), 0xAB, dtype=torch.uint8, device=device)
    c_d, n_d = _up(clean, device), _up(noisy, device)
    status = clx.load().clx_changed_rows(clx.ptr(c_d), clx.ptr(n_d), T, C, ID, IH, IW, *window, chunk, clx.ptr(rows),
                                         clx.ptr(counts), cap, clx.ptr(ws), clx.stream_ptr(device))
    assert status == 0, clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    rows_h, counts_h = rows.cpu().numpy(), counts.cpu().numpy()
    assert (rows_h[nchunks * cap:] == SENT).all(), "rows: written past the last chunk's capacity"
    assert (counts_h[nchunks:] == SENT).all(), "counts: written past the last chunk"
    assert bool((ws[nbytes:] == 0xAB).all().item()), "workspace: written past clx_changed_rows_workspace bytes"
    return counts_h[:nchunks], rows_h[:nchunks * cap].reshape(nchunks, cap), ws


def run_tiles(device, ws, T, shape, window, WH, WW, tile, chunk, cap=None):
    """clx_changed_tiles on the workspace clx_changed_rows left -> (counts, slots)"""
    clx = _clx()
    _od, oh, ow = out_extents(shape, window)
    th, tw = -(-(oh - WH + 1) // tile), -(-(ow - WW + 1) // tile)
    nchunks = -(-T // chunk)
    if cap is None:
        cap = min(chunk, T) * th * tw
    tiles = torch.full((nchunks * cap + TAIL,), SENT, dtype=torch.int32, device=device)
    counts = torch.full((nchunks + TAIL,), SENT, dtype=torch.int32, device=device)
    before = ws.clone()
    status = clx.load().clx_changed_tiles(clx.ptr(ws), T, *shape, *window, WH, WW, tile, chunk, clx.ptr(tiles),
                                          clx.ptr(counts), cap, clx.stream_ptr(device))
    assert status == 0, clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    assert torch.equal(ws, before), "clx_changed_tiles wrote to the workspace it reads"
    tiles_h, counts_h = tiles.cpu().numpy(), counts.cpu().numpy()
    assert (tiles_h[nchunks * cap:] == SENT).all(), "tiles: written past the last chunk's capacity"
    assert (counts_h[nchunks:] == SENT).all(), "tile counts: written past the last chunk"
    return counts_h[:nchunks], tiles_h[:nchunks * cap].reshape(nchunks, cap)


def check_lists(counts, slots, ref_lists, what=""):
    """counts are the true ones whatever the capacity; a chunk's slots hold its sorted reference list, or — capacity
    below the count — `cap` distinct members of it; the slots behind keep their sentinel"""
    cap = slots.shape[1]
    assert len(counts) == len(ref_lists)
    for k, ref in enumerate(ref_lists):
        assert counts[k] == len(ref), (what, k, int(counts[k]), len(ref))
        n = min(len(ref), cap)
        got = slots[k, :n]
        if len(ref) <= cap:
            assert np.array_equal(np.sort(got), ref), (what, k)
        else:
            assert len(np.unique(got)) == n and np.isin(got, ref).all(), (what, k)
        assert (slots[k, n:] == SENT).all(), (what, k, "written past the count")


# =========================================================================================================== patterns
def xs_of(IW):
    return sorted({x for x in (0, 62, 63, 64, 65, IW - 1) if 0 <= x < IW})


def copies(rng, C, shape, channel=0):
    """clean (C, *shape) and one noisy copy per pattern, every difference in `channel` only:
    0 nothing, 1 every pixel, then one copy per corner with that single pixel, one per x in {0, 62, 63, 64, 65, IW - 1}
    with that single pixel of a middle row, and a last one with 1 % random pixels"""
    ID, IH, IW = shape
    clean = rng.random((C,) + tuple(shape), dtype=np.float32)
    single = [(z, y, x) for z in sorted({0, ID - 1}) for y in sorted({0, IH - 1}) for x in sorted({0, IW - 1})]
    single += [(ID // 2, IH // 2, x) for x in xs_of(IW)]
    T = 2 + len(single) + 1
    noisy = np.repeat(clean[None], T, axis=0)
    noisy[1, channel] += 1.0
    for i, (z, y, x) in enumerate(single):
        noisy[2 + i, channel, z, y, x] = 2.0
    hits = rng.random(shape) < 0.01
    hits[ID // 2, IH // 2, IW // 2] = True
    noisy[T - 1, channel][hits] = 3.0
    return clean, noisy


def rows_case(device, rng, C, shape, window, chunks=(1, 3), channel=0):
    """the patterns of copies() at one shape and window, per chunk size, against the reference; -> (want, workspace)"""
    clean, noisy = copies(rng, C, shape, channel)
    T = noisy.shape[0]
    npix = int(np.prod(out_extents(shape, window)))
    ws = want = None
    for chunk in chunks:
        want, ref = changed_rows_ref(clean, noisy, window, chunk)
        counts, slots, ws = run_rows(device, clean, noisy, window, chunk)
        check_lists(counts, slots, ref, (shape, window, chunk))
        if chunk == 1:
            assert counts[0] == 0 and (slots[0] == SENT).all()                 # no difference: nothing written
            assert counts[1] == npix                                           # every pixel: every row
            assert (counts[2:] > 0).all()
    return want, ws, T


# =================================================================================================== clx_changed_rows
WIDTHS = (63, 64, 65, 66, 127, 128, 129, 130, 194)


@pytest.mark.parametrize("KW", [1, 2, 3, 5])
def test_changed_rows_at_word_edges(KW, device):
    """IW in {KW, 63 .. 66, 127 .. 130, 194} x KH in {1, 3, IH}, seven input rows, every pattern of copies(), chunks of 1
    and 3 copies.  Branches of dilate_rows_kernel:
      `left < 64` FALSE                     OW % 64 == 0: IW - KW + 1 in {64, 128} (IW = 64 + KW - 1, e.g. 64 / 1, 65 / 2, 66 / 3)
      `wd + 1 < nw` FALSE                   IW % 64 == 0 (IW = 64, 128): the row's last word has no right neighbour
      `wd + 1 < nw` TRUE at the last word   nw > onw: IW = 65 and 129 with KW >= 2 (output pixel 62 reads input word 1),
                                            IW = 66 / 130 with KW >= 3
      KW = 1 (no shifts), KH = 1, KH = IH (one output row)"""
    rng = np.random.default_rng(KW)
    IH = 7
    for IW in (KW,) + WIDTHS:
        for KH in (1, 3, IH):
            rows_case(device, rng, 1, (1, IH, IW), (1, KH, KW))


def test_changed_rows_with_a_63_wide_window(device):
    """dilate_rows_kernel, KW large: 62 shifts, `hi << (64 - dx)` down to a shift by 2; IW = 130: nw = 3, onw = 2"""
    rng = np.random.default_rng(63)
    for KH in (1, 3):
        rows_case(device, rng, 1, (1, 7, 130), (1, KH, 63))
    rows_case(device, rng, 1, (1, 4, 63), (1, 2, 63))                         # one output pixel per row


@pytest.mark.parametrize("KD", [1, 2, 3])
def test_changed_rows_in_3d(KD, device):
    """ID = 3 with KD in {1, 2, 3}: dilate_rows_kernel's KD loop, the (oz * OH + oy) line decode, KD = ID (one plane)"""
    rng = np.random.default_rng(30 + KD)
    for IW in (64, 65, 130):
        for KH, KW in ((1, 1), (3, 3), (5, 2)):
            rows_case(device, rng, 1, (3, 5, IW), (KD, KH, KW))


def test_changed_rows_with_the_difference_in_the_last_channel_only(device):
    """diff_bits_kernel, C > 2: channels 0 and 1 are equal everywhere, every pattern sits in channel 2"""
    rng = np.random.default_rng(3)
    for shape, window in (((1, 7, 130), (1, 3, 3)), ((3, 5, 65), (2, 3, 3))):
        rows_case(device, rng, 3, shape, window, channel=2)
        rows_case(device, rng, 2, shape, window, channel=1)


def test_changed_rows_chunking(device):
    """chunk = 1, chunk = T, chunk > T (also the largest chunk the 31-bit rule admits), T % chunk != 0, with nothing,
    everything and the mixed patterns"""
    rng = np.random.default_rng(4)
    shape, window = (1, 11, 10), (1, 3, 3)
    npix = 9 * 8
    clean, mixed = copies(rng, 1, shape)
    T = mixed.shape[0]
    nothing = np.repeat(clean[None], T, axis=0)
    everything = nothing + 1.0
    biggest = (2 ** 31 - 1) // npix                          # 29826161: chunk * npix_out < 2^31 still holds
    assert (biggest + 1) * npix >= 2 ** 31
    for chunk in (1, T, T + 1, 4, T - 1, biggest):
        assert chunk != 4 or T % 4 != 0
        nchunks = -(-T // chunk)
        counts, slots, _ws = run_rows(device, clean, nothing, window, chunk)
        assert (counts == 0).all() and (slots == SENT).all()
        counts, slots, _ws = run_rows(device, clean, everything, window, chunk)
        full = [min(chunk, T - k * chunk) * npix for k in range(nchunks)]
        assert counts.tolist() == full
        check_lists(counts, slots, changed_rows_ref(clean, everything, window, chunk)[1], ("everything", chunk))
        counts, slots, _ws = run_rows(device, clean, mixed, window, chunk)
        check_lists(counts, slots, changed_rows_ref(clean, mixed, window, chunk)[1], ("mixed", chunk))


def test_changed_rows_a_wavefront_serves_ten_chunks(device):
    """dilate_rows_kernel's allocation loop, more than two rounds: three output words per copy (OD * OH * onw = 1 * 3 * 1),
    70 copies in chunks of 2, a hit in every copy — a wavefront's 64 words belong to 21 or 22 copies = 11 or 12 chunks, and
    chunks 10, 21 and 32 are shared by two wavefronts (two atomics into one count).  Then the same with copies that have
    no hit in between (lanes that never ask) and chunks of 3 and 1."""
    rng = np.random.default_rng(5)
    shape, window = (1, 3, 40), (1, 1, 3)
    T = 70
    assert int(np.prod(out_extents(shape, window)[:2])) * ((out_extents(shape, window)[2] + 63) // 64) == 3
    clean = rng.random((1,) + shape, dtype=np.float32)
    noisy = np.repeat(clean[None], T, axis=0)
    for t in range(T):
        noisy[t, 0, 0, t % 3, (7 * t) % 40] = 2.0
    noisy[:, 0][rng.random((T,) + shape) < 0.05] = 3.0
    for chunk in (2, 3, 1):
        counts, slots, _ws = run_rows(device, clean, noisy, window, chunk)
        assert (counts > 0).all()
        check_lists(counts, slots, changed_rows_ref(clean, noisy, window, chunk)[1], chunk)
    noisy[5:9] = clean
    noisy[20:41:2] = clean[None]
    counts, slots, _ws = run_rows(device, clean, noisy, window, 2)
    check_lists(counts, slots, changed_rows_ref(clean, noisy, window, 2)[1], "gaps")
    assert counts[3] == 0 and (counts == 0).sum() == 1


def test_changed_rows_capacity_below_the_count(device):
    """cap = 5 against counts of 0, 1, some hundreds and chunk * npix_out: the counts stay the true ones, the first `cap`
    slots of a chunk hold distinct members of its list, a chunk below the capacity keeps its sentinels, nothing is written
    behind (run_rows checks the tail).  Also cap = 1 and a capacity of exactly the largest count."""
    rng = np.random.default_rng(6)
    shape, window = (1, 7, 130), (1, 3, 3)
    clean, noisy = copies(rng, 1, shape)
    T = noisy.shape[0]
    order = [0, 0, 2, 0, 1, 1, T - 1, T - 1, 1]              # chunks of 2: nothing | one row | all | 1 % | all, ragged
    noisy = np.ascontiguousarray(noisy[order])
    _want, ref = changed_rows_ref(clean, noisy, window, 2)
    assert [len(r) for r in ref][:3] == [0, 1, 2 * 5 * 128] and len(ref[3]) > 5 and len(ref[4]) == 5 * 128
    for cap in (5, 1, max(len(r) for r in ref)):
        counts, slots, _ws = run_rows(device, clean, noisy, window, 2, cap=cap)
        check_lists(counts, slots, ref, cap)


def test_changed_rows_above_the_grid_cap_of_diff_bits(device):
    """diff_bits_kernel's grid-stride loop, second trip: 8 copies of 1 x 600 x 1000 are 76800 words = 4.9 M threads against
    the cap of 16384 blocks x 256 = 4.19 M, so words from 65536 on — copy 6 from row 496, all of copy 7 — are written on
    the second trip.  A few hundred hits, three of them placed at the seam and at the very end.
    (dilate_rows_kernel has one thread per output WORD: its cap would take 268 M output pixels, which is left out.)"""
    rng = np.random.default_rng(7)
    T, shape, window = 8, (1, 600, 1000), (1, 3, 3)
    assert T * 600 * 16 * 64 > 16384 * 256 and 6 * 600 * 16 + 496 * 16 == 65536
    clean = rng.random((1,) + shape, dtype=np.float32)
    noisy = np.repeat(clean[None], T, axis=0)
    for t, y, x in zip(rng.integers(0, T, 300), rng.integers(0, 600, 300), rng.integers(0, 1000, 300)):
        noisy[t, 0, 0, y, x] = 2.0
    for t, y, x in ((6, 495, 999), (6, 496, 0), (7, 599, 999), (7, 0, 0), (7, 300, 960)):
        noisy[t, 0, 0, y, x] = 2.0
    _want, ref = changed_rows_ref(clean, noisy, window, 2)
    assert all(200 < len(r) < 4096 for r in ref)
    counts, slots, _ws = run_rows(device, clean, noisy, window, 2, cap=4096)
    check_lists(counts, slots, ref)


def test_changed_rows_value_semantics(device):
    """The comparison is the float `!=` of the reference: a pixel holding the same NaN in both images IS reported (a NaN
    differs from itself), -0.0 against 0.0 is NOT."""
    rng = np.random.default_rng(8)
    shape = (1, 7, 130)
    IW = shape[2]
    clean = rng.random((1,) + shape, dtype=np.float32)
    clean[0, 0, 3, 64] = np.nan
    clean[0, 0, 5, 70] = 0.0
    clean[0, 0, 1, 2] = -0.0
    noisy = np.repeat(clean[None], 2, axis=0)
    noisy[:, 0, 0, 5, 70] = -0.0
    noisy[:, 0, 0, 1, 2] = 0.0
    noisy[1, 0, 0, 6, 129] = np.nan                                           # a NaN in the copy alone
    assert noisy[0].tobytes() != clean.tobytes()                              # (the zeros differ in their sign bit)
    counts, slots, _ws = run_rows(device, clean, noisy, (1, 1, 1), 1)
    assert counts.tolist() == [1, 2]
    assert slots[0, 0] == 3 * IW + 64 and sorted(slots[1, :2].tolist()) == [3 * IW + 64, 6 * IW + 129]
    for window in ((1, 1, 1), (1, 3, 3)):
        counts, slots, _ws = run_rows(device, clean, noisy, window, 1)
        check_lists(counts, slots, changed_rows_ref(clean, noisy, window, 1)[1], window)


# ================================================================================================== clx_changed_tiles
TILE_OW = (64, 65, 66, 126, 128, 129, 130, 148)


@pytest.mark.parametrize("tile, WH, WW", [(2, 1, 1), (4, 3, 3), (6, 2, 3), (4, 3, 1), (62, 3, 3)])
def test_changed_tiles_at_word_edges(tile, WH, WW, device):
    """OW in {64, 65, 66, 126, 128, 129, 130, 148} x OH in {7, 10}, behind a (1, 1, 1) first window (the row bits ARE the
    difference) and a (1, 3, 3) one, every pattern of copies(), chunks of 1 and 3 copies.
    Branches of changed_tiles_kernel:
      `nbits >= 64`                       (62, 3, 3): tile + WW - 1 = 64, at x0 = 0 (OW >= 64) and x0 = 62 (OW >= 126)
      `sh != 0` with `wd + 1 == onw`      a window inside the row's last word: (4, 3, 3) at OW = 148, x0 = 132;
                                          (62, 3, 3) at OW = 128, x0 = 124; (2, 1, 1) at OW = 126, x0 = 66
      `sh != 0` with `wd + 1 < onw`       a window across a word boundary: (4, 3, 3) x0 = 60; (62, 3, 3) x0 = 62
      clipped right / bottom windows      OW - WW + 1 (OH - WH + 1) no multiple of the tile: e.g. (4, 3, 3) at OW = 65,
                                          OH = 7; whole tiles at OW = 66, OH = 10; (2, 1, 1) is clipped at the odd extents
      `x0 % 64 == 0`                      tiles 2 and 4 from OW = 66 on (x0 = 64, 128)
    and, for (62, 3, 3), OH = OW = 64: one whole tile whose window is one full word."""
    rng = np.random.default_rng(tile * 100 + WH * 10 + WW)
    cases = [(OH, OW) for OW in TILE_OW for OH in (7, 10)] + ([(64, 64)] if tile == 62 else [])
    for OH, OW in cases:
        for window in ((1, 1, 1), (1, 3, 3)):
            shape = (1, OH + window[1] - 1, OW + window[2] - 1)
            want, ws, T = rows_case(device, rng, 1, shape, window, chunks=(3,))
            th, tw = -(-(OH - WH + 1) // tile), -(-(OW - WW + 1) // tile)
            for chunk in (1, 3):
                changed, ref = changed_tiles_ref(want, WH, WW, tile, chunk)
                counts, slots = run_tiles(device, ws, T, shape, window, WH, WW, tile, chunk)
                check_lists(counts, slots, ref, (OH, OW, window, chunk))
                if chunk == 1:
                    assert counts[0] == 0 and (slots[0] == SENT).all()         # nothing changed
                    assert counts[1] == th * tw                                # everything changed
                    assert (counts[2:] > 0).all()


def test_changed_tiles_a_wavefront_serves_many_chunks(device):
    """changed_tiles_kernel's allocation loop, three or more rounds: th * tw = 1 * 2, 70 copies in chunks of 2, a hit in
    every copy: a wavefront's 64 tiles belong to 32 copies = 16 chunks.  Then with copies that have no changed tile."""
    rng = np.random.default_rng(9)
    shape, window = (1, 8, 12), (1, 3, 3)                                     # OH = 6, OW = 10: 4 x 8 outputs of (3, 3)
    T = 70
    clean = rng.random((1,) + shape, dtype=np.float32)
    noisy = np.repeat(clean[None], T, axis=0)
    for t in range(T):
        noisy[t, 0, 0, t % 8, (5 * t) % 12] = 2.0
    for gaps in (False, True):
        if gaps:
            noisy[6:10] = clean
            noisy[21:50:2] = clean[None]
        for chunk in (2, 3):
            want, ref_rows = changed_rows_ref(clean, noisy, window, chunk)
            counts, slots, ws = run_rows(device, clean, noisy, window, chunk)
            check_lists(counts, slots, ref_rows)
            changed, ref = changed_tiles_ref(want, 3, 3, 4, chunk)
            assert changed.shape[1:] == (1, 2) and 0 < changed.sum() < changed.size
            counts, slots = run_tiles(device, ws, T, shape, window, 3, 3, 4, chunk)
            check_lists(counts, slots, ref, (gaps, chunk))
            assert gaps == bool((counts == 0).any())


def test_changed_tiles_nothing_everything_and_capacity(device):
    """no changed row in any copy: counts 0, no slot written; every row changed: every tile of every chunk, with chunk =
    1, T, > T and T % chunk != 0; a capacity below the count: true counts, `cap` distinct members, nothing behind"""
    rng = np.random.default_rng(10)
    shape, window, T = (1, 15, 134), (1, 3, 3), 5                             # OH = 13, OW = 132: 3 x 33 tiles (clipped)
    th, tw = 3, 33
    clean = rng.random((1,) + shape, dtype=np.float32)
    nothing = np.repeat(clean[None], T, axis=0)
    _c, _s, ws = run_rows(device, clean, nothing, window, 2)
    for chunk in (1, 2, T, T + 3):
        counts, slots = run_tiles(device, ws, T, shape, window, 3, 3, 4, chunk)
        assert (counts == 0).all() and (slots == SENT).all()
    everything = nothing + 1.0
    want, _ref = changed_rows_ref(clean, everything, window, 2)
    _c, _s, ws = run_rows(device, clean, everything, window, 2)
    for chunk in (1, 2, T, T + 3):
        counts, slots = run_tiles(device, ws, T, shape, window, 3, 3, 4, chunk)
        assert counts.tolist() == [min(chunk, T - k * chunk) * th * tw for k in range(-(-T // chunk))]
        check_lists(counts, slots, changed_tiles_ref(want, 3, 3, 4, chunk)[1], chunk)
    mixed = nothing.copy()
    mixed[1] = everything[1]
    mixed[2, 0, 0, 7, 64] = 2.0
    mixed[4, 0][rng.random(shape) < 0.004] = 2.0
    want, _ref = changed_rows_ref(clean, mixed, window, 2)
    _c, _s, ws = run_rows(device, clean, mixed, window, 2)
    changed, ref = changed_tiles_ref(want, 3, 3, 4, 2)
    assert len(ref[0]) == th * tw and 0 < len(ref[1]) <= 4 and len(ref[2]) > 4
    for cap in (3, 1, th * tw):
        counts, slots = run_tiles(device, ws, T, shape, window, 3, 3, 4, 2, cap=cap)
        check_lists(counts, slots, ref, cap)


# ========================================================================================================== row movers
def _filled(device, shape, tail=TAIL):
    """a float destination of `shape` filled with FSENT, with `tail` more sentinels behind it -> (whole, view)"""
    n = int(np.prod(shape))
    whole = torch.full((n + tail,), FSENT, dtype=torch.float32, device=device)
    return whole, whole[:n].view(*shape)


def test_gather_rows_strides_duplicates_and_untouched_columns(device):
    """ld_src = 20, ld_dst = 12, width = 8; duplicate and descending indices; n = 1; columns [width, ld_dst) of dst and
    the floats behind the last row keep their sentinel"""
    clx = _clx()
    rng = np.random.default_rng(11)
    src_h = rng.random((50, 20), dtype=np.float32)
    src = _up(src_h, device)
    st = clx.stream_ptr(device)
    for idx_h in ([49, 49, 40, 7, 7, 7, 3, 0, 0], [31], list(range(49, -1, -1)) + [0, 49]):
        idx_h = np.asarray(idx_h, np.int32)
        n = len(idx_h)
        idx = _up(idx_h, device)
        whole, dst = _filled(device, (n, 12))
        clx.call("clx_gather_rows", clx.ptr(src), 20, clx.ptr(idx), n, 8, clx.ptr(dst), 12, st)
        torch.cuda.synchronize(device)
        got = whole.cpu().numpy()
        ref = np.full((n, 12), FSENT, np.float32)
        ref[:, :8] = src_h[idx_h, :8]
        assert np.array_equal(got[:n * 12].reshape(n, 12), ref)
        assert (got[n * 12:] == FSENT).all()
        assert np.array_equal(src.cpu().numpy(), src_h)


def test_gather_and_scatter_of_no_rows_launch_nothing(device):
    """n = 0 with null pointers: OK, and no launch (a launch with these arguments would be an error)"""
    clx = _clx()
    st = clx.stream_ptr(device)
    for name in ("clx_gather_rows", "clx_scatter_rows"):
        assert getattr(clx.load(), name)(NULL, 8, NULL, 0, 8, NULL, 8, st) == 0
    torch.cuda.synchronize(device)


def test_scatter_rows_strides_and_untouched_rows_and_columns(device):
    """distinct indices, ld_src = 12, ld_dst = 20, width = 8: rows of dst that are not named, columns past `width` of the
    named ones and the floats behind dst keep their sentinel"""
    clx = _clx()
    rng = np.random.default_rng(12)
    st = clx.stream_ptr(device)
    for n in (17, 1, 50):
        idx_h = rng.permutation(50)[:n].astype(np.int32)
        src_h = rng.random((n, 12), dtype=np.float32)
        whole, dst = _filled(device, (50, 20))
        src, idx = _up(src_h, device), _up(idx_h, device)
        clx.call("clx_scatter_rows", clx.ptr(src), 12, clx.ptr(idx), n, 8, clx.ptr(dst), 20, st)
        torch.cuda.synchronize(device)
        ref = np.full((50, 20), FSENT, np.float32)
        ref[idx_h, :8] = src_h[:, :8]
        got = whole.cpu().numpy()
        assert np.array_equal(got[:1000].reshape(50, 20), ref)
        assert (got[1000:] == FSENT).all()


def test_broadcast_rows_small(device):
    """copies in {1, 3}, nfloats = 4 (one 16-byte group) and 1000; nothing behind the last copy is written"""
    clx = _clx()
    rng = np.random.default_rng(13)
    st = clx.stream_ptr(device)
    for nfloats in (4, 1000):
        src_h = rng.random(nfloats, dtype=np.float32)
        src = _up(src_h, device)
        for copies_ in (1, 3):
            whole, dst = _filled(device, (copies_, nfloats))
            clx.call("clx_broadcast_rows", clx.ptr(src), nfloats, clx.ptr(dst), copies_, st)
            torch.cuda.synchronize(device)
            got = whole.cpu().numpy()
            assert np.array_equal(got[:copies_ * nfloats].reshape(copies_, nfloats), np.repeat(src_h[None], copies_, 0))
            assert (got[copies_ * nfloats:] == FSENT).all()


def test_gather_and_scatter_above_the_grid_cap(device):
    """140000 rows of 128 floats are 4.48 M 16-byte groups against the cap of 16384 blocks x 256 threads = 4.19 M: rows
    from 131072 on move on the second trip of the grid-stride loop.  (72 MB per full-size buffer; compared on the
    device with torch's own indexing.)"""
    clx = _clx()
    n, width = 140000, 128
    assert n * (width // 4) > 16384 * 256
    g = torch.Generator(device="cpu").manual_seed(14)
    src = torch.rand((4096, width), generator=g).to(device)
    idx = torch.randint(0, 4096, (n,), generator=g, dtype=torch.int32).to(device)
    st = clx.stream_ptr(device)
    whole, dst = _filled(device, (n, width))
    clx.call("clx_gather_rows", clx.ptr(src), width, clx.ptr(idx), n, width, clx.ptr(dst), width, st)
    assert torch.equal(dst, src[idx.long()])
    assert bool((whole[n * width:] == FSENT).all().item())
    perm = torch.randperm(n, generator=g).to(torch.int32).to(device)
    whole2, back = _filled(device, (n, width))
    clx.call("clx_scatter_rows", clx.ptr(dst), width, clx.ptr(perm), n, width, clx.ptr(back), width, st)
    assert torch.equal(back[perm.long()], dst)
    assert bool((whole2[n * width:] == FSENT).all().item())


def test_broadcast_rows_above_the_grid_cap(device):
    """17 M floats are 4.25 M 16-byte groups against the cap of 4.19 M threads; two copies"""
    clx = _clx()
    nfloats = 17_000_000
    assert nfloats % 4 == 0 and nfloats // 4 > 16384 * 256
    src = torch.rand(nfloats, device=device)
    whole, dst = _filled(device, (2, nfloats))
    clx.call("clx_broadcast_rows", clx.ptr(src), nfloats, clx.ptr(dst), 2, clx.stream_ptr(device))
    assert torch.equal(dst[0], src) and torch.equal(dst[1], src)
    assert bool((whole[2 * nfloats:] == FSENT).all().item())


# ================================================================================================== end to end
@pytest.mark.parametrize("W", [66, 68, 130])
@pytest.mark.parametrize("name", ["2d_small", "2d_96"])
def test_sparse_forward_equals_dense_at_word_edge_widths(name, W, device, monkeypatch):
    """infer mode on a 28 x W image, W in {66, 68, 130}: the first convolution's output rows are 64, 66 and 128 pixels
    wide — exactly one word, two pixels into the second, exactly two words — where the existing dense-versus-sparse
    tests have 30 to 90.  The changed-rows path (and, at 96 channels, the tile list of the Winograd layer behind it) gives
    the dense forward's bits."""
    from cellulus_amd.models import get_model
    from test_gpu_unet import CONFIGS

    cfg = CONFIGS[name]["cfg"]
    torch.manual_seed(6)
    model = get_model(**cfg)
    for _n, layer in model.named_modules():
        if isinstance(layer, torch.nn.modules.conv._ConvNd):
            torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
            torch.nn.init.uniform_(layer.bias, -0.1, 0.1)
    model = model.to(device)
    n_it = 4
    raw = torch.rand(1, 1, 28, W)
    noise = torch.rand(1, 2 * n_it, 1, 28, W, generator=torch.Generator().manual_seed(2))
    x = raw.to(device)
    model.max_infer_batch = 4
    model.set_infer(p_salt_pepper=0.008, num_infer_iterations=n_it, device=device)
    monkeypatch.setenv("CLX_STREAMS_MIN_GFLOP", "0")          # (an image this small is below the size the path starts at)
    monkeypatch.setenv("CLX_SPARSE_NOISE", "0")
    dense = model.infer_on_device(x, noise=noise).clone()
    monkeypatch.delenv("CLX_SPARSE_NOISE")
    model._last_changed_rows = None
    sparse = model.infer_on_device(x, noise=noise)
    info = model._last_changed_rows
    assert info is not None and info["used"], info
    assert info["window"] == (1, 3, 3) and 0.0 < info["fraction"] < 0.3
    if name == "2d_96":
        assert "tile_fraction" in info and 0.0 < info["tile_fraction"] < 0.7, info
    assert torch.isfinite(dense).all()
    assert torch.equal(dense, sparse)
    monkeypatch.setenv("CLX_INFER_STREAMS", "1")              # the chunks one after the other instead of on two streams
    model._last_changed_rows = None
    assert torch.equal(dense, model.infer_on_device(x, noise=noise))
    assert model._last_changed_rows["used"]
