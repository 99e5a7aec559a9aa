"""clx_label_propagate through the C ABI against the restatements of tests/propagate_ref.py (a heap Dijkstra on (cost, id); for
the large maps the Jacobi relaxation over shifted views).  Everything is integer work: owner, cost and info[0] must be EQUAL in
every element.  Outputs and the workspace are prefilled with 0xAB bytes and sit between guard words that must stay untouched.

The constants below mirror csrc/label_propagate.hip: TileShape<2> (TY, TX) and TileShape<3> (TZ, TY, TX), the extents of a tile;
MAX_SWEEPS, the sweeps a tile makes in one round; and csrc/tile_rounds.h: TILE_MAX_GRID, the blocks of a round, beyond which a
block takes more than one tile; MAX_ROUNDS, the rounds of a call."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

from propagate_ref import COST_INF, dots_map, ref_propagate, ref_propagate_sweeps, ridge_image, serpentine
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

TILE_2D, TILE_3D = (16, 64), (8, 8, 16)
TILE_MAX_GRID, MAX_SWEEPS, MAX_ROUNDS = 1024, 32, 64


def run_propagate(seeds, mask, weight, nid, reg, limit, device, rounds=8):
    """calls with `rounds` rounds each, the first with resume = 0, until info[1] == 0 -> (owner, cost, info[0] of the first
    call, the sum of info[2], the number of calls); the guard words are checked"""
    from cellulus_amd import _clx

    seeds = np.ascontiguousarray(seeds, dtype=np.int32)
    nd = seeds.ndim
    Z, Y, X = (1,) * (3 - nd) + seeds.shape
    lib = _clx.load()
    keep = [_dev(seeds, device), None if mask is None else _dev(np.asarray(mask, dtype=np.uint8), device),
            None if weight is None else _dev(np.asarray(weight, dtype=np.int32), device)]
    nbytes = int(lib.clx_label_propagate_workspace(nd, Z, Y, X))
    assert nbytes > 8 * seeds.size
    outs = dict(owner=Out(seeds.shape, np.int32, device), cost=Out(seeds.shape, np.int32, device), info=Out((3,), np.int32, device),
                workspace=Out((nbytes,), np.uint8, device))
    flags, busy, calls = None, 0, 0
    while True:
        status = lib.clx_label_propagate(*[_clx.ptr(t) for t in keep], nd, Z, Y, X, nid, reg, -1 if limit is None else limit, rounds, int(calls > 0),
                                         outs["owner"].ptr, outs["cost"].ptr, outs["info"].ptr, outs["workspace"].ptr, nbytes, _clx.stream_ptr(device))
        assert status == 0, lib.clx_last_error()
        torch.cuda.synchronize(device)
        info = outs["info"].get()
        flags = int(info[0]) if calls == 0 else flags
        assert calls == 0 or info[0] == 0
        assert 0 <= info[2] <= rounds and (info[1] == 0 or info[2] == rounds)
        busy, calls = busy + int(info[2]), calls + 1
        if info[1] == 0:
            break
        assert busy <= seeds.size + 1, "the relaxation does not come to rest"
    outs["workspace"].get()
    return outs["owner"].get(), outs["cost"].get(), flags, busy, calls


def assert_equal(seeds, device, mask=None, weight=None, nid=None, reg=1, limit=None, ref=ref_propagate, rounds=8):
    nid = int(np.max(seeds)) + 1 if nid is None else nid
    got = run_propagate(seeds, mask, weight, nid, reg, limit, device, rounds)
    want = ref(seeds, mask, weight, nid=nid, reg=reg, limit=limit)
    assert got[2] == want[2]
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    return got


def scene(shape, seed, nseeds=None):
    """seeded (seeds, mask, weight) of `shape`: small boxes, four fifths of the pixels allowed, grey levels 0 .. 9"""
    rng = np.random.default_rng(seed)
    n = max(2, int(np.prod(shape)) // 60) if nseeds is None else nseeds
    return dots_map(shape, n, seed), (rng.random(shape) < 0.8).astype(np.uint8), rng.integers(0, 10, size=shape).astype(np.int32)


@pytest.mark.parametrize("X", (1, 3, 5, 67))
def test_widths(X, device):
    for shape in ((1, X), (19, X), (3, 9, X)):
        seeds, mask, weight = scene(shape, 10 + X)
        assert_equal(seeds, device, mask, weight)
        assert_equal(seeds, device, mask, weight, reg=0, limit=9)


@pytest.mark.parametrize("shape", [(y, x) for y in (15, 16, 17) for x in (63, 64, 65)] + list(itertools.product((7, 8, 9), (7, 8, 9), (15, 16, 17))),
                         ids=lambda s: "x".join(map(str, s)))
def test_one_below_at_and_above_a_tile(shape, device):
    tile = TILE_2D if len(shape) == 2 else TILE_3D
    assert all(abs(s - t) <= 1 for s, t in zip(shape, tile))
    seeds, mask, weight = scene(shape, sum(shape), nseeds=5)
    assert_equal(seeds, device, mask, weight)
    corner = np.zeros(shape, np.int32)                                   # one seed in the last corner: every pixel is reached from it
    corner[tuple(s - 1 for s in shape)] = 2
    owner, cost, _, _, _ = assert_equal(corner, device, ref=ref_propagate_sweeps)
    assert (owner == 2).all() and cost[(0,) * len(shape)] == cost.max()


def test_rows_and_slices_do_not_wrap(device):
    seeds = np.zeros((4, 7), np.int32)
    seeds[0, 6], seeds[2, 0] = 1, 2
    mask = np.zeros((4, 7), np.uint8)
    mask[1, 0], mask[1, 6], mask[3, 6] = 1, 1, 1                         # (1, 0) follows (0, 6) in memory; (3, 6) .. (2, 0) likewise
    owner, cost, _, _, _ = assert_equal(seeds, device, mask)
    assert owner[1, 0] == 2 and owner[1, 6] == 1 and owner[3, 6] == 0 and cost[3, 6] == COST_INF
    only = mask.copy()
    only[1, 6] = 0
    seeds[2, 0] = 0
    owner, _, _, _, _ = assert_equal(seeds, device, only)
    assert owner[1, 0] == 0 and (owner > 0).sum() == 1
    vol = np.zeros((3, 4, 17), np.int32)
    vol[0, 3, 16] = 5                                                    # the last pixel of slice 0; (1, 0, 0) follows it in memory
    open_ = np.zeros(vol.shape, np.uint8)
    open_[1, 0, 0], open_[0, 0, 0], open_[1, 3, 0], open_[2, 0, 16] = 1, 1, 1, 1
    owner, _, _, _, _ = assert_equal(vol, device, open_)
    assert (owner > 0).sum() == 1
    for tile_edge in ((17, 65), (9, 9, 17)):                             # the same at the seam of two tiles
        seeds = np.zeros(tile_edge, np.int32)
        seeds[tuple(t - 1 for t in (TILE_2D if len(tile_edge) == 2 else TILE_3D))] = 3
        assert_equal(seeds, device, reg=2, limit=40)


def test_corner_and_z_neighbours(device):
    seeds = np.zeros((3, 3), np.int32)
    seeds[1, 1] = 1
    for corner in ((0, 0), (0, 2), (2, 0), (2, 2)):
        mask = np.zeros((3, 3), np.uint8)
        mask[corner] = 1
        owner, cost, _, _, _ = assert_equal(seeds, device, mask, reg=3)
        assert owner[corner] == 1 and cost[corner] == 12
    vol = np.zeros((3, 3, 3), np.int32)
    vol[1, 1, 1] = 2
    for corner in itertools.product((0, 2), repeat=3):
        mask = np.zeros((3, 3, 3), np.uint8)
        mask[corner] = 1
        owner, cost, _, _, _ = assert_equal(vol, device, mask)
        assert owner[corner] == 2 and cost[corner] == 5 and (owner > 0).sum() == 2
    for z in (0, 2):                                                     # neighbours that differ only in z
        mask = np.zeros((3, 3, 3), np.uint8)
        mask[z, 1, 1] = 1
        owner, cost, _, _, _ = assert_equal(vol, device, mask)
        assert owner[z, 1, 1] == 2 and cost[z, 1, 1] == 3
    chain = np.zeros((9, 1, 1), np.int32)                                # a column along z through two tiles
    chain[0, 0, 0] = 1
    assert assert_equal(chain, device, reg=2)[1][8, 0, 0] == 48


def tie_map(shape=(33, 70)):
    """single-pixel seeds on a lattice 6 rows and 4 columns apart whose ids differ from their neighbours': on a flat image the
    pixels half way between two of them are ties"""
    seeds = np.zeros(shape, np.int32)
    ny, nx = len(range(0, shape[0], 6)), len(range(0, shape[1], 4))
    seeds[::6, ::4] = (np.arange(ny)[:, None] * 33 + np.arange(nx)[None, :] * 7) % 9 + 1
    return seeds


def test_ties_in_both_id_orders(device):
    seeds = tie_map()
    nid = int(seeds.max()) + 1
    turned = np.where(seeds > 0, nid - seeds, 0)
    first = assert_equal(seeds, device, nid=nid)
    second = assert_equal(turned, device, nid=nid)
    assert np.array_equal(first[1], second[1])
    assert (first[0] != np.where(second[0] > 0, nid - second[0], 0)).sum() > 50          # the map has ties between different seeds
    vol = np.zeros((5, 9, 18), np.int32)
    vol[0, 4, 2], vol[4, 4, 2], vol[2, 0, 14], vol[2, 8, 14] = 3, 2, 1, 4
    for v in (vol, np.where(vol > 0, 5 - vol, 0)):
        owner = assert_equal(v, device, nid=5)[0]
        assert owner[2, 4, 2] == min(v[0, 4, 2], v[4, 4, 2]) and owner[2, 4, 14] == min(v[2, 0, 14], v[2, 8, 14])


def test_limits(device):
    seeds = np.zeros((12, 70), np.int32)
    seeds[5, 30], seeds[10, 66] = 2, 1
    for limit in (None, 0, 1, 2, 3, 11, 12, 13, 2 ** 30 - 1):
        owner, cost, _, _, _ = assert_equal(seeds, device, limit=limit)
        if limit is not None:
            assert ((cost <= limit) | (cost == COST_INF)).all() and ((owner == 0) == (cost == COST_INF)).all()
    owner, cost, _, _, _ = assert_equal(seeds, device, limit=12)         # a limit at a pixel's cost ...
    assert owner[5, 34] == 2 and cost[5, 34] == 12 and owner[2, 33] == 2 and cost[2, 33] == 12 and owner[5, 35] == 0
    owner, cost, _, _, _ = assert_equal(seeds, device, limit=11)         # ... and one below it
    assert owner[5, 34] == 0 and cost[5, 34] == COST_INF and owner[2, 33] == 0 and owner[3, 32] == 2 and cost[3, 32] == 8
    owner, cost, _, _, _ = assert_equal(seeds, device, limit=0)
    assert np.array_equal(owner, seeds) and np.array_equal(cost == 0, seeds > 0) and (cost[seeds == 0] == COST_INF).all()


def test_ridge_the_cheaper_path_is_the_longer_one(device):
    image = ridge_image()
    seeds = np.zeros(image.shape, np.int32)
    seeds[2, 5] = 1
    owner, cost, _, _, _ = assert_equal(seeds, device, weight=image, reg=1)
    assert cost[2, 9] == 34 and owner[2, 9] == 1 and cost[2, 7] == 6 + 200               # round the wall; onto it
    owner, cost, _, _, _ = assert_equal(seeds, device, weight=image, reg=100)
    assert cost[2, 9] == 1200 + 400 and owner[2, 9] == 1                                 # across it
    wide = np.zeros((20, 140), np.int32)                                 # the same wall across the seam of two tiles
    wide[:17, 64] = 300
    seeds = np.zeros(wide.shape, np.int32)
    seeds[3, 60], seeds[19, 139] = 1, 2
    for reg in (1, 200):
        assert_equal(seeds, device, weight=wide, reg=reg)


def test_zero_cost_plateaus(device):
    seeds = np.zeros((20, 70), np.int32)
    seeds[2, 5], seeds[4:6, 30:32], seeds[15, 8], seeds[12, 33], seeds[3, 50], seeds[18, 66], seeds[10, 69] = 7, 3, 5, 6, 4, 2, 8
    mask = np.ones((20, 70), np.uint8)
    mask[:, 40], mask[9, :40] = 0, 0                                     # three components, two or three seeds in each
    owner, cost, _, _, _ = assert_equal(seeds, device, mask, reg=0)
    for part in (np.s_[:9, :40], np.s_[10:, :40], np.s_[:, 41:]):
        ids = seeds[part][seeds[part] > 0]
        free = (seeds[part] == 0) & (mask[part] > 0)
        assert len(ids) and (owner[part][free] == ids.min()).all() and not cost[part][free].any()
    assert_equal(seeds, device, mask, reg=0, limit=0)
    steps = (np.arange(70)[None, :] // 10 + np.zeros((20, 1), np.int64)).astype(np.int32)      # plateaus with steps between them
    assert_equal(seeds, device, mask, steps, reg=0)
    assert_equal(dots_map((9, 9, 20), 5, 78), device, reg=0)


@pytest.mark.parametrize("with_mask,with_weight", [(False, False), (True, False), (False, True), (True, True)])
def test_null_mask_and_weight(with_mask, with_weight, device):
    for shape in ((21, 70), (5, 10, 19)):
        seeds, mask, weight = scene(shape, 31)
        assert_equal(seeds, device, mask if with_mask else None, weight if with_weight else None, reg=2)


def test_edge_states(device):
    seeds, mask, weight = scene((18, 66), 41)
    mask[seeds > 0] = 0                                                  # every seed lies outside the mask: still a source
    owner, _, _, _, _ = assert_equal(seeds, device, mask, weight)
    assert np.array_equal(owner[seeds > 0], seeds[seeds > 0]) and (owner[(seeds == 0) & (mask > 0)] > 0).any()
    for shape in ((18, 66), (4, 9, 20), (1, 1), (1, 1, 1)):
        none = np.zeros(shape, np.int32)
        owner, cost, flags, busy, calls = assert_equal(none, device, nid=1)               # a map without seeds
        assert not owner.any() and (cost == COST_INF).all() and flags == 0 and busy == 0 and calls == 1
        full = np.full(shape, 6, np.int32)
        owner, cost, _, busy, _ = assert_equal(full, device)
        assert (owner == 6).all() and not cost.any() and busy == 0
    seeds = dots_map((18, 66), 5, 42)
    owner, cost, _, busy, _ = assert_equal(seeds, device, np.zeros((18, 66), np.uint8))   # a map whose mask is empty
    assert np.array_equal(owner, seeds) and busy == 0


def corridor_case():
    mask = serpentine((20, 150))
    seeds = np.zeros(mask.shape, np.int32)
    seeds[0, 0], seeds[18, 149] = 2, 1
    return seeds, mask, (np.arange(150)[None, :] % 7 + np.zeros((20, 1), np.int64)).astype(np.int32)


def test_serpentine_resumes_and_makes_the_same_rounds(device):
    seeds, mask, weight = corridor_case()
    assert -(-20 // TILE_2D[0]) * -(-150 // TILE_2D[1]) >= 5             # the corridor runs through six tiles
    runs = {rounds: assert_equal(seeds, device, mask, weight, rounds=rounds, ref=ref_propagate_sweeps) for rounds in (1, 2, MAX_ROUNDS)}
    assert np.array_equal(runs[1][0] > 0, mask > 0)
    assert runs[2][4] > 1 and runs[1][4] == runs[1][3] + 1               # resume = 1 was needed; one call a round, the last one idle
    assert runs[1][3] == runs[2][3] == runs[MAX_ROUNDS][3] > 5           # the same rounds changed a tile, whatever the chunks
    again = run_propagate(seeds, mask, weight, 3, 1, None, device, rounds=2)
    assert again[0].tobytes() == runs[2][0].tobytes() and again[1].tobytes() == runs[2][1].tobytes() and again[2:] == runs[2][2:]


def test_bad_ids_and_weights(device):
    seeds = dots_map((9, 70), 6, 41)
    assert assert_equal(seeds, device)[2] == 0
    for value, nid in ((-1, 7), (7, 7), (2 ** 24, 7), (-2 ** 31, 7), (6, 6)):
        dirty = seeds.copy()
        dirty[4, 33], dirty[8, 69] = value, value
        owner, cost, flags, _, _ = assert_equal(dirty, device, nid=nid)
        assert flags == 1 and owner.max() < nid and 0 < owner[4, 33] != value and 0 < cost[4, 33] < COST_INF       # entered, no seed
    for value in (-1, 65536, 2 ** 31 - 1, -2 ** 31):
        weight = np.zeros(seeds.shape, np.int32)
        weight[3, 20:50], weight[0, 0] = value, 65535
        owner, cost, flags, _, _ = assert_equal(seeds, device, weight=weight)
        assert flags == 2 and not owner[3, 20:50].any() and (cost[3, 20:50] == COST_INF).all() and owner[0, 0] > 0
        under = np.zeros(seeds.shape, np.int32)
        under[seeds == 2] = value                                        # under a seed: no source
        owner, _, flags, _, _ = assert_equal(seeds, device, weight=under)
        assert flags == 2 and not (owner == 2).any()
        hidden = np.ones(seeds.shape, np.uint8)
        hidden[3, 20:50] = 0
        hidden[seeds > 0] = 1
        unseen = np.where(seeds > 0, 0, weight)                          # neither allowed nor a seed: the weight does not count
        assert (unseen[hidden == 0] == value).all() and assert_equal(seeds, device, hidden, unseen)[2] == 0
    assert assert_equal(seeds, device, weight=np.full(seeds.shape, 65535, np.int32))[2] == 0


def test_more_tiles_than_blocks(device):
    shape = (TILE_2D[0] * 25, TILE_2D[1] * 41)
    assert (shape[0] // TILE_2D[0]) * (shape[1] // TILE_2D[1]) == TILE_MAX_GRID + 1       # one block makes a second trip
    rng = np.random.default_rng(5)
    seeds = np.zeros(shape, np.int32)
    ny, nx = shape[0] // 8, shape[1] // 8
    seeds[4::8, 4::8] = (np.arange(ny)[:, None] * 37 + np.arange(nx)[None, :] * 11) % 97 + 1      # at most 4 pixels from every pixel
    mask = (rng.random(shape) < 0.95).astype(np.uint8)
    weight = rng.integers(0, 3, size=shape).astype(np.int32)
    owner, cost, _, busy, _ = assert_equal(seeds, device, mask, weight, limit=24, ref=lambda *a, **k: ref_propagate_sweeps(*a, max_sweeps=12, **k))
    assert len(np.unique(owner)) == 98 and (owner[-16:, -64:] > 0).mean() > 0.8 and busy >= 1


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    seeds = torch.zeros(64, dtype=torch.int32, device=device)
    seeds[27] = 3
    mask, weight = torch.ones(64, dtype=torch.uint8, device=device), torch.zeros(64, dtype=torch.int32, device=device)
    exact = int(lib.clx_label_propagate_workspace(2, 1, 8, 8))
    assert exact == int(lib.clx_label_propagate_workspace(3, 2, 4, 8))
    outs = dict(owner=Out((64,), np.int32, device), cost=Out((64,), np.int32, device), info=Out((3,), np.int32, device),
                workspace=Out((exact,), np.uint8, device))
    null = ctypes.c_void_p(0)

    def propagate(nd=2, Z=1, Y=8, X=8, nid=4, reg=1, limit=-1, rounds=8, resume=0, nbytes=exact, **ptrs):
        p = {k: o.ptr for k, o in outs.items()}
        p.update(seeds=_clx.ptr(seeds), mask=_clx.ptr(mask), weight=_clx.ptr(weight))
        p.update(ptrs)
        return lib.clx_label_propagate(p["seeds"], p["mask"], p["weight"], nd, Z, Y, X, nid, reg, limit, rounds, resume, p["owner"], p["cost"],
                                       p["info"], p["workspace"], nbytes, st)

    refused = [dict(nd=1), dict(nd=4), dict(Z=2), dict(Y=0), dict(X=-8), dict(nd=3, Z=0), dict(nid=0), dict(nid=2 ** 24 + 1), dict(reg=-1),
               dict(reg=65536), dict(limit=-2), dict(limit=2 ** 30), dict(rounds=0), dict(rounds=MAX_ROUNDS + 1), dict(resume=2), dict(resume=-1),
               dict(Y=65536, X=65536, nbytes=2 ** 40), dict(nd=3, Z=2, Y=46341, X=46341, nbytes=2 ** 40), dict(nbytes=exact - 1), dict(nbytes=0),
               dict(Y=16, nbytes=exact), dict(workspace=ctypes.c_void_p(outs["workspace"].ptr.value + 2))]
    refused += [{k: null} for k in ("seeds", "owner", "cost", "info", "workspace")]
    for kw in refused:
        assert propagate(**kw) == -1, f"{kw} was accepted"
        assert lib.clx_last_error().decode().startswith("clx_label_propagate:"), kw
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    want = ref_propagate(seeds.cpu().numpy().reshape(8, 8), nid=4)
    for kw in (dict(), dict(mask=null), dict(weight=null), dict(mask=null, weight=null)):   # the same buffers, valid arguments
        assert propagate(**kw) == 0
        torch.cuda.synchronize(device)
        assert outs["info"].get().tolist() == [0, 0, 1]
        assert np.array_equal(outs["owner"].get().reshape(8, 8), want[0]) and np.array_equal(outs["cost"].get().reshape(8, 8), want[1])
    assert propagate(nd=3, Z=2, Y=4) == 0 and propagate(resume=1, rounds=1) == 0
    torch.cuda.synchronize(device)
    outs["workspace"].get()
