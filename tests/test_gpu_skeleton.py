"""clx_label_thin and clx_skeleton_census through the C ABI against the restatement of tests/skeleton_ref.py.  Everything is
bits and integers: every element of out, info and the census words must be EQUAL.  Outputs and the workspace are prefilled
with 0xAB bytes and sit between guard words that must stay untouched.

The constants below mirror csrc/label_thin.hip: a word is 64 pixels of a row (a segment of csrc/segments.h); a block loads an
extent of 8 words x 128 rows, a TILE of 6 words x 96 rows with a halo of one word / 16 rows; a launch runs at most 8 iterations,
a call at most 64; a launch has at most 1024 blocks, beyond which a block takes more than one tile."""

import ctypes

import numpy as np
import pytest
import torch

from skeleton_ref import DIST_INF, census, disc, noise_map, serpentine, skeleton, thin
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

WORD, TILE_X, TILE_Y, HALO_X, HALO_Y, LAUNCH_ITERATIONS, MAX_GRID = 64, 384, 96, 64, 16, 8, 1024
_REF = {}


def ref(key, make):
    """a reference computed once per key and left unchanged"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


class Thinner:
    """the buffers of one map and calls of clx_label_thin on them"""

    def __init__(self, labels, device):
        from cellulus_amd import _clx

        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.nd = self.labels.ndim
        self.Z, self.Y, self.X = (1,) * (3 - self.nd) + self.labels.shape
        self.lib, self.device = _clx.load(), device
        self.lab = _dev(self.labels, device)
        self.nbytes = int(self.lib.clx_label_thin_workspace(self.nd, self.Z, self.Y, self.X))
        words = self.Z * self.Y * ((self.X + WORD - 1) // WORD)
        tiles = self.Z * ((self.Y + TILE_Y - 1) // TILE_Y) * ((self.X + TILE_X - 1) // TILE_X)
        assert self.nbytes == 128 + 80 * words + 2 * ((tiles + 7) // 8 * 8)
        self.out, self.info = Out(self.labels.shape, np.int32, device), Out((3,), np.int32, device)
        self.workspace = Out((self.nbytes,), np.uint8, device)
        self.calls = 0

    def call(self, iterations):
        from cellulus_amd import _clx

        status = self.lib.clx_label_thin(_clx.ptr(self.lab), self.nd, self.Z, self.Y, self.X, iterations, int(self.calls > 0), self.out.ptr,
                                         self.info.ptr, self.workspace.ptr, self.nbytes, _clx.stream_ptr(self.device))
        assert status == 0, self.lib.clx_last_error()
        torch.cuda.synchronize(self.device)
        self.calls += 1
        self.workspace.get()
        return self.out.get(), self.info.get().tolist()


def run_thin(labels, device, iterations=64, limit=400):
    """calls of ``iterations`` each until one reports the fixed point -> (out, the pixels deleted by all calls, the calls)"""
    t = Thinner(labels, device)
    deleted = 0
    while True:
        out, info = t.call(iterations)
        assert info[0] == 0 and info[1] >= 0 and info[2] >= info[1]
        deleted += info[2]
        if info[1] == 0:
            return out, deleted, t.calls
        assert t.calls < limit


def assert_skeleton(labels, device, key=None, iterations=64):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    want = ref(key, lambda: skeleton(labels)) if key else skeleton(labels)
    out, deleted, calls = run_thin(labels, device, iterations)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]
    assert deleted == int((labels != 0).sum() - (want != 0).sum())
    return out, calls


@pytest.mark.parametrize("Y", (1, 2, 3))
def test_widths_1_to_67(Y, device):
    for X in range(1, 68):
        assert_skeleton(noise_map((Y, X), 1000 * Y + X, block=5, sigma=0.8) if X > 1 else np.ones((Y, X), np.int32), device)
        assert_skeleton(np.full((Y, X), 3, np.int32), device)


@pytest.mark.parametrize("shape", [(20, x) for x in (383, 384, 385, 447, 448, 449, 511, 512, 513)]
                         + [(y, 70) for y in (95, 96, 97, 111, 112, 113, 127, 128, 129)] + [(97, 385), (113, 449), (129, 513)])
def test_tile_and_halo_extents(shape, device):
    assert_skeleton(noise_map(shape, shape[0] + shape[1], block=17, sigma=2.5), device)
    assert_skeleton(np.ones(shape, np.int32), device)                     # one object over the whole map: the longest schedule


def test_objects_across_word_and_tile_seams(device):
    labels = np.zeros((200, 800), np.int32)
    labels[5:30, 50:80] = 1                                               # across the word seam at x = 64
    labels[40:75, 360:410] = 2                                            # across the tile seam at x = 384
    labels[80:115, 100:160] = 3                                           # across the tile seam at y = 96
    yy, xx = np.indices(labels.shape)
    labels[(yy - 96) ** 2 + (xx - 384) ** 2 <= 30 ** 2] = 4               # over the corner where four tiles meet
    labels[150:190, 740:800], labels[150:190, 0:30] = 5, 5                # at both ends of the rows
    out, _ = assert_skeleton(labels, device)
    assert all((out == k).any() for k in range(1, 6))


def test_row_ends_do_not_wrap(device):
    for X in (6, 64, 65, 128):
        labels = np.zeros((7, X), np.int32)
        labels[0:3, X - 2:X], labels[1:4, 0:2], labels[4:7, X - 3:X], labels[5:7, 0:3] = 1, 1, 1, 1
        out, _ = assert_skeleton(labels, device)
        wide = np.pad(labels, ((0, 0), (0, 5)))                           # the same objects away from the right edge
        assert np.array_equal(out, skeleton(wide)[:, :X])
    stack = np.zeros((3, 4, 5), np.int32)                                  # the last row of a slice and the first of the next
    stack[0, 2:4, :], stack[1, 0:2, :] = 1, 1
    assert_skeleton(stack, device)


def test_touching_objects_and_label_values(device):
    base = noise_map((60, 90), 5, block=10, labels=2)
    assert ((base[:, :-1] != base[:, 1:]) & (base[:, :-1] != 0) & (base[:, 1:] != 0)).any()       # two labels do touch
    ordered = assert_skeleton(base, device)[0]
    swapped = assert_skeleton(np.where(base == 1, 2, np.where(base == 2, 1, 0)), device)[0]
    assert np.array_equal(ordered != 0, swapped != 0)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    extreme = np.where(base == 1, lo, np.where(base == 2, hi, 0))
    out = assert_skeleton(extreme, device)[0]
    assert np.array_equal(out != 0, ordered != 0) and set(np.unique(out).tolist()) == {lo, 0, hi}
    assert_skeleton(np.where(base == 1, -1, base), device)


def test_disc_over_several_launches_and_calls(device):
    labels = disc(40)
    want, deleted = ref("disc40", lambda: thin(labels))
    assert len(deleted) - 1 > 2 * LAUNCH_ITERATIONS                       # more than two launches' worth
    outs = {}
    for iterations in (1, 2, 64):
        out, total, calls = run_thin(labels, device, iterations)
        assert np.array_equal(out, want) and total == sum(deleted)
        assert calls == -(-len(deleted) // iterations)
        outs[iterations] = out
    # the counts of every single call
    t = Thinner(labels, device)
    for n in deleted:
        out, info = t.call(1)
        assert info == [0, n, n]
    t = Thinner(labels, device)
    assert t.call(10)[1] == [0, deleted[9], sum(deleted[:10])]
    assert t.call(64)[1] == [0, 0, sum(deleted[10:])]
    out, info = t.call(3)                                                  # after the fixed point: nothing runs, out is written
    assert info == [0, 0, 0] and np.array_equal(out, want)


def state_map():
    """blobs that come to rest after a few iterations and a disc that takes 40, over the seams at x = 384 and y = 96"""
    labels = noise_map((120, 420), 77, block=40, sigma=4.0)
    labels[20:105, 320:405] = disc(40, 3)
    return labels


@pytest.mark.parametrize("n", (1, 2, 5, 8, 9, 16, 17))
def test_state_after_n_iterations(n, device):
    labels = ref("state_map", state_map)
    want, deleted = ref(("state", n), lambda: thin(labels, n))
    assert deleted[-1] > 0
    out, info = Thinner(labels, device).call(n)
    assert np.array_equal(out, want) and info == [0, deleted[-1], sum(deleted)]
    t = Thinner(labels, device)                                            # the same in two calls
    t.call(1)
    if n > 1:
        out, info = t.call(n - 1)
        assert np.array_equal(out, want) and info == [0, deleted[-1], sum(deleted[1:])]


def waking_map():
    """One-pixel-wide bars in the tile left of x = 384 that hang on a thick blob in the tile right of it.  The bars are at rest
    while the blob's edge between them thins; in the 5th iteration the pixel (56, 383), where three of them meet, has lost its
    neighbours in the other tile and goes.  (Found by a search over random bars with the restatement; a bar alone never loses
    a pixel.)"""
    labels = np.zeros((112, 640), np.int32)
    labels[20:91, 384:600] = 1
    labels[52:61, 380:384] = [[1, 0, 1, 1], [1, 0, 0, 0], [0, 1, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 0],
                              [0, 1, 1, 1]]
    return labels


def test_a_tile_at_rest_wakes_when_its_halo_changes(device):
    labels = waking_map()
    want, deleted = ref("waking", lambda: thin(labels))
    early = ref("waking_early", lambda: thin(labels, 4)[0])
    assert np.array_equal(early[:, :TILE_X], labels[:, :TILE_X])           # four iterations leave the left tile alone ...
    assert np.argwhere((want != labels)[:, :TILE_X]).tolist() == [[56, 383]]       # ... and the fifth deletes in it
    for iterations in (1, 2, 3, 4, 64):                                    # launches of 1, 2, 3 and 4 iterations: the left tile rests in the first
        out, total, _ = run_thin(labels, device, iterations)
        assert np.array_equal(out, want), np.argwhere(out != want)[:5]
        assert total == sum(deleted)


def test_serpentine_through_several_tiles(device):
    labels = serpentine((230, 900), width=7, gap=4)
    out, _ = assert_skeleton(labels, device, key="serpentine")
    assert len(np.unique(np.argwhere(out)[:, 1] // TILE_X)) == 3 and len(np.unique(np.argwhere(out)[:, 0] // TILE_Y)) == 3


def test_stack_equals_its_slices(device):
    labels = noise_map((4, 50, 75), 9, block=14)
    labels[1, 10:30, 10:40], labels[2, 15:35, 20:50] = 2, 2                # one label in adjacent slices, overlapping in y and x
    out, _ = assert_skeleton(labels, device)
    for z in range(4):
        assert np.array_equal(out[z], assert_skeleton(labels[z], device)[0])


def test_one_tile_more_than_the_launch_cap(device):
    labels = np.zeros((MAX_GRID + 1, 6, 9), np.int32)
    labels[:, 1:5, 1:8] = 1
    labels[::7, 2, 3] = 0
    labels[-1, :, :] = 5
    assert_skeleton(labels, device, key="cap")


# ----------------------------------------------------------------------------------------------------------------- census

def run_census(skel, device, dist=None, nid=None):
    from cellulus_amd import _clx

    skel = np.ascontiguousarray(skel, dtype=np.int32)
    nd = skel.ndim
    Z, Y, X = (1,) * (3 - nd) + skel.shape
    nid = max(int(skel.max()) + 1, 1) if nid is None else nid
    lab = _dev(skel, device)
    d = None if dist is None else _dev(np.ascontiguousarray(dist, dtype=np.int32), device)
    words, bad = Out((nid, 10), np.int64, device), Out((1,), np.int32, device)
    lib = _clx.load()
    status = lib.clx_skeleton_census(_clx.ptr(lab), _clx.ptr(d), nd, Z, Y, X, nid, words.ptr, bad.ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return words.get(), int(bad.get()[0])


def assert_census(skel, device, dist=None, nid=None):
    want, want_bad = census(skel, dist, nid)
    got, bad = run_census(skel, device, dist, nid)
    assert bad == want_bad
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    return got


def test_census_equals_restatement(device):
    rng = np.random.default_rng(3)
    for shape, seed in (((70, 131), 1), ((3, 40, 67), 2), ((1, 64), 3), ((5, 1), 4), ((97, 385), 5)):
        labels = noise_map(shape, seed, block=12, labels=9)
        skel = skeleton(labels)
        dist = rng.integers(0, 5000, size=shape)
        for lab in (skel, labels):                                         # a thinned map; an unthinned one: blocks, dropped diagonals
            assert_census(lab, device)
            got = assert_census(lab, device, dist)
            assert got[1:, 7].sum() == dist[lab != 0].sum()
        assert got[:, 3].sum() > 0 or min(shape[-2:]) == 1             # the unthinned map has blocks


def test_census_many_ids_and_one_object(device):
    rng = np.random.default_rng(4)
    labels = rng.integers(1, 5000, size=(90, 200)).astype(np.int32)         # far more ids than a block's table holds
    labels[rng.random(labels.shape) < 0.3] = 0
    dist = rng.integers(0, DIST_INF, size=labels.shape)
    assert_census(labels, device, dist, nid=5000)
    assert_census(labels, device, dist, nid=1 << 16)
    whole = np.full((300, 333), 2, np.int32)                                # one object over the whole map
    got = assert_census(whole, device, np.full(whole.shape, DIST_INF - 1))
    assert got[2].tolist() == [300 * 333, 299 * 333 + 300 * 332, 0, 299 * 332, 0, 300 * 333 - 4, 0, 300 * 333 * (DIST_INF - 1), DIST_INF - 1, DIST_INF - 1]


def test_census_bad_bits(device):
    skel = skeleton(noise_map((40, 70), 6, labels=4))
    assert assert_census(skel, device, nid=5)[4, 0] > 0
    for lab in (np.where(skel == 4, 7, skel), np.where(skel == 4, -3, skel), np.where(skel == 4, 2 ** 31 - 1, skel)):
        got, bad = run_census(lab, device, nid=5)                          # bit 0 alone: the label is background, for its neighbours too
        assert bad == 1 and np.array_equal(got, census(np.where(skel == 4, 0, skel), nid=5)[0])
    dist = np.full(skel.shape, 9)
    y, x = np.argwhere(skel == 2)[0]
    for value in (-1, DIST_INF, 2 ** 31 - 1):
        dist[y, x] = value
        got, bad = run_census(skel, device, dist, nid=5)                   # bit 1 alone: the pixel counts, its value does not
        assert bad == 2 and got[2, 0] == (skel == 2).sum() and got[2, 7] == 9 * ((skel == 2).sum() - 1)
        assert np.array_equal(got, census(skel, dist, nid=5)[0])
    dist[skel == 0] = -7                                                   # under background nothing is read into the words
    assert run_census(skel, device, dist, nid=5)[1] == 2


# -------------------------------------------------------------------------------------------------------------- refusals

def test_rejected_arguments(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    labels = _dev(np.ones((2, 6, 70), np.int32), device)
    nbytes = int(lib.clx_label_thin_workspace(3, 2, 6, 70))
    out, info, workspace = Out((2, 6, 70), np.int32, device), Out((3,), np.int32, device), Out((nbytes + 8,), np.uint8, device)
    null, stream = ctypes.c_void_p(0), _clx.stream_ptr(device)
    good = dict(labels=_clx.ptr(labels), nd=3, Z=2, Y=6, X=70, iterations=1, resume=0, out=out.ptr, info=info.ptr, workspace=workspace.ptr,
                nbytes=nbytes)
    cases = [dict(labels=null), dict(out=null), dict(info=null), dict(workspace=null), dict(nd=1), dict(nd=4), dict(nd=2), dict(Z=0), dict(Y=0),
             dict(X=-1), dict(Z=1 << 11, Y=1 << 10, X=1 << 10), dict(iterations=0), dict(iterations=65), dict(iterations=-1), dict(resume=2),
             dict(resume=-1), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(workspace=ctypes.c_void_p(workspace.ptr.value + 4)),
             dict(out=_clx.ptr(labels))]
    for case in cases:
        a = dict(good, **case)
        status = lib.clx_label_thin(a["labels"], a["nd"], a["Z"], a["Y"], a["X"], a["iterations"], a["resume"], a["out"], a["info"],
                                    a["workspace"], a["nbytes"], stream)
        assert status == -1 and lib.clx_last_error().startswith(b"clx_label_thin: "), (case, status)
    words, bad = Out((4, 10), np.int64, device), Out((1,), np.int32, device)
    good = dict(skeleton=_clx.ptr(labels), dist=null, nd=3, Z=2, Y=6, X=70, nid=4, words=words.ptr, bad=bad.ptr)
    for case in (dict(skeleton=null), dict(words=null), dict(bad=null), dict(nd=1), dict(nd=2), dict(Z=0), dict(Y=-2), dict(X=0),
                 dict(Z=1 << 11, Y=1 << 10, X=1 << 10), dict(nid=0), dict(nid=(1 << 24) + 1), dict(nid=-1)):
        a = dict(good, **case)
        status = lib.clx_skeleton_census(a["skeleton"], a["dist"], a["nd"], a["Z"], a["Y"], a["X"], a["nid"], a["words"], a["bad"], stream)
        assert status == -1 and lib.clx_last_error().startswith(b"clx_skeleton_census: "), (case, status)
    torch.cuda.synchronize(device)
    assert all(o.untouched() for o in (out, info, workspace, words, bad))  # refused before any launch
