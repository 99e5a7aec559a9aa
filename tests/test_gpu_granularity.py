"""clx_grey_morph and clx_grey_reconstruct through the C ABI against the restatements of tests/granularity_ref.py (shifted views
for the morphology; for the reconstruction a max-heap flood, for the large maps the whole-map update iterated to its fixed
point).  Everything is integer work: out, bad and info[0] must be EQUAL in every element.  Outputs and the workspace are
prefilled with 0xAB bytes and sit between guard words that must stay untouched.

The constants below mirror csrc/grey_morph.hip: MorphShape / ReconShape, the extents of a tile (2-D: TY, TX; 3-D: TZ, TY, TX);
MORPH_STEPS (HMAX), the largest halo and so the steps of one call; MAX_SWEEPS, the sweeps a tile makes in one round; and
csrc/tile_rounds.h: TILE_MAX_GRID, the blocks of a launch, beyond which a block takes more than one tile; MAX_ROUNDS, the rounds
of a call."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

from granularity_ref import MAX_LEVEL, random_levels, ref_morph, ref_reconstruct, ref_reconstruct_sweeps, serpentine
from test_gpu_measure import Out, _dev

pytestmark = pytest.mark.gpu

MORPH_2D, MORPH_3D, MORPH_STEPS = (32, 64), (8, 8, 32), {2: 16, 3: 4}
RECON_2D, RECON_3D = (32, 256), (8, 8, 64)
TILE_MAX_GRID, MAX_SWEEPS, MAX_ROUNDS = 1024, 16, 64


def _zyx(a):
    return (1,) * (3 - a.ndim) + a.shape


def run_morph(image, mask, op, steps, device):
    from cellulus_amd import _clx

    image = np.ascontiguousarray(image, dtype=np.int32)
    keep = [_dev(image, device), None if mask is None else _dev(np.asarray(mask, dtype=np.uint8), device)]
    outs = dict(out=Out(image.shape, np.int32, device), bad=Out((1,), np.int32, device))
    lib = _clx.load()
    status = lib.clx_grey_morph(_clx.ptr(keep[0]), _clx.ptr(keep[1]), image.ndim, *_zyx(image), op, steps, outs["out"].ptr, outs["bad"].ptr,
                                _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return outs["out"].get(), int(outs["bad"].get()[0])


def assert_morph(image, device, mask=None, steps=1, ops=(0, 1)):
    got = None
    for op in ops:
        got = run_morph(image, mask, op, steps, device)
        want = ref_morph(image, mask, op, steps)
        assert got[1] == want[1], (op, steps)
        assert np.array_equal(got[0], want[0]), (op, steps, np.argwhere(got[0] != want[0])[:5])
    return got


def run_reconstruct(marker, image, mask, device, rounds=8):
    """calls with `rounds` rounds each, the first with resume = 0, until info[1] == 0 -> (out, info[0] of the first call, the sum
    of info[2], the number of calls); the guard words are checked"""
    from cellulus_amd import _clx

    image = np.ascontiguousarray(image, dtype=np.int32)
    nd, (Z, Y, X) = image.ndim, _zyx(image)
    lib = _clx.load()
    keep = [_dev(np.asarray(marker, dtype=np.int32), device), _dev(image, device),
            None if mask is None else _dev(np.asarray(mask, dtype=np.uint8), device)]
    nbytes = int(lib.clx_grey_reconstruct_workspace(nd, Z, Y, X))
    assert nbytes > 6 * image.size
    outs = dict(out=Out(image.shape, np.int32, device), info=Out((3,), np.int32, device), workspace=Out((nbytes,), np.uint8, device))
    flags, busy, calls = None, 0, 0
    while True:
        status = lib.clx_grey_reconstruct(*[_clx.ptr(t) for t in keep], nd, Z, Y, X, rounds, int(calls > 0), outs["out"].ptr, outs["info"].ptr,
                                          outs["workspace"].ptr, nbytes, _clx.stream_ptr(device))
        assert status == 0, lib.clx_last_error()
        torch.cuda.synchronize(device)
        info = outs["info"].get()
        flags = int(info[0]) if calls == 0 else flags
        assert calls == 0 or info[0] == 0
        assert 0 <= info[2] <= rounds and (info[1] == 0 or info[2] == rounds)
        busy, calls = busy + int(info[2]), calls + 1
        if info[1] == 0:
            break
        assert busy <= image.size + 1, "the reconstruction does not come to rest"
    outs["workspace"].get()
    return outs["out"].get(), flags, busy, calls


def assert_reconstruct(marker, image, device, mask=None, ref=ref_reconstruct, rounds=8):
    got = run_reconstruct(marker, image, mask, device, rounds)
    want = ref(marker, image, mask)
    assert got[1] == want[1]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    return got


def scene(shape, seed, top=40):
    """seeded (marker, image, mask): grey levels below `top`, a fifth of the pixels carry a marker, four fifths are inside"""
    rng = np.random.default_rng(seed)
    image = random_levels(rng, shape, top)
    marker = random_levels(rng, shape, top + 10) * (rng.random(shape) < 0.2)
    return marker.astype(np.int32), image, (rng.random(shape) < 0.8).astype(np.uint8)


def around(tile, extra):
    """per axis the extents one below, at and above the tile and the tile plus `extra`"""
    return [sorted({t - 1, t, t + 1, t + extra - 1, t + extra, t + extra + 1}) for t in tile]


# ---------------------------------------------------------------- clx_grey_morph

@pytest.mark.parametrize("Y", (1, 2, 3))
def test_morph_widths_1_to_67(Y, device):
    for X in range(1, 68):
        _, image, mask = scene((Y, X), 100 * Y + X, top=3000)
        assert_morph(image, device, mask if X % 2 else None, steps=1 + (X + Y) % 16)
    for X in (1, 5, 33, 67):
        _, image, mask = scene((Y + 1, 3, X), X, top=3000)
        assert_morph(image, device, mask if X % 3 else None, steps=1 + X % 4)


@pytest.mark.parametrize("nd", (2, 3))
def test_morph_shapes_around_the_tile_and_its_halo(nd, device):
    tile = MORPH_2D if nd == 2 else MORPH_3D
    sizes = around(tile, MORPH_STEPS[nd])
    shapes = set(itertools.product(*sizes)) if nd == 2 else {tuple(s if a == axis else tile[a] + 1 for a in range(3)) for axis in range(3) for s in sizes[axis]}
    assert len(shapes) == (36 if nd == 2 else 16)
    for n, shape in enumerate(sorted(shapes)):
        _, image, mask = scene(shape, n, top=60000)
        assert_morph(image, device, mask if n % 2 else None, steps=MORPH_STEPS[nd] if n % 3 else 1, ops=(n % 2,) if nd == 2 else (0, 1))


@pytest.mark.parametrize("steps", (1, 2, 15, 16))
def test_morph_diamond_is_exact_at_the_halos_last_pixel(steps, device):
    shape = (2 * MORPH_2D[0] + 6, 2 * MORPH_2D[1] + 12)
    ty, tx = MORPH_2D
    places = [(ty, tx), (ty - 1, tx - 1), (ty, 30), (ty - 1, 100), (10, tx), (50, tx - 1),                 # a tile corner, the seams
              (ty + steps, tx + steps), (ty - 1 - steps, tx - 1 - steps), (ty + steps - 1, tx + steps), (ty - steps, 20),
              (0, 0), (shape[0] - 1, shape[1] - 1), (0, shape[1] - 1)]                                     # the image corners
    yy, xx = np.indices(shape)
    for y, x in places:
        if not (0 <= y < shape[0] and 0 <= x < shape[1]):
            continue
        hole = np.full(shape, MAX_LEVEL, np.int32)
        hole[y, x] = 0
        diamond = np.abs(yy - y) + np.abs(xx - x) <= steps
        out, _ = assert_morph(hole, device, steps=steps, ops=(0,))
        assert np.array_equal(out == 0, diamond) and (out[~diamond] == MAX_LEVEL).all(), (y, x)
        out, _ = assert_morph(MAX_LEVEL - hole, device, steps=steps, ops=(1,))
        assert np.array_equal(out == MAX_LEVEL, diamond) and not out[~diamond].any(), (y, x)


@pytest.mark.parametrize("steps", (1, 2, 3, 4))
def test_morph_octahedron_across_the_seams_3d(steps, device):
    tz, ty, tx = MORPH_3D
    shape = (tz + 7, ty + 7, tx + 9)
    grid = np.indices(shape)
    for at in ((tz, ty, tx), (tz - 1, ty - 1, tx - 1), (tz + steps, ty + steps, tx + steps), (tz - 1 - steps, 3, tx - 1 - steps), (0, 0, 0),
               tuple(s - 1 for s in shape)):
        if min(at) < 0:
            continue
        hole = np.full(shape, MAX_LEVEL, np.int32)
        hole[at] = 0
        ball = sum(np.abs(g - c) for g, c in zip(grid, at)) <= steps
        out, _ = assert_morph(hole, device, steps=steps, ops=(0,))
        assert np.array_equal(out == 0, ball), at
        out, _ = assert_morph(MAX_LEVEL - hole, device, steps=steps, ops=(1,))
        assert np.array_equal(out == MAX_LEVEL, ball), at


def test_morph_rows_and_slices_do_not_wrap_and_z_neighbours(device):
    flat = np.full((4, 7), 9, np.int32)
    flat[0, 6] = 0                                                      # (1, 0) follows (0, 6) in memory
    out, _ = assert_morph(flat, device, steps=1, ops=(0,))
    assert out[1, 0] == 9 and out[0, 5] == 0 and out[1, 6] == 0
    vol = np.full((3, 4, 17), 9, np.int32)
    vol[0, 3, 16] = 0                                                   # the last pixel of slice 0; (1, 0, 0) follows it
    out, _ = assert_morph(vol, device, steps=1, ops=(0,))
    assert out[1, 0, 0] == 9 and out[1, 3, 16] == 0 and (out == 0).sum() == 4
    column = np.arange(1, 20, dtype=np.int32).reshape(19, 1, 1)          # neighbours that differ only in z, through three tiles
    for steps in (1, 4):
        out, _ = assert_morph(column, device, steps=steps)
        assert out[:, 0, 0].tolist() == [min(19, z + 1 + steps) for z in range(19)]
    only_z = np.zeros((3, 3, 3), np.uint8)
    only_z[:, 1, 1] = 1
    cube = np.arange(27, dtype=np.int32).reshape(3, 3, 3)
    out, _ = assert_morph(cube, device, only_z, steps=1, ops=(0,))
    assert out[:, 1, 1].tolist() == [4, 4, 13] and out.sum() == 21


def test_morph_masks(device):
    shape = (40, 150)
    rng = np.random.default_rng(3)
    image = random_levels(rng, shape, 60000)
    image[20, 70] = 0
    wall = np.ones(shape, np.uint8)
    wall[:, 66] = 0                                                     # a wall of one pixel beside the seam at x = 64
    for steps in (1, 5, 16):
        out, _ = assert_morph(image, device, wall, steps=steps)
        assert not out[:, 66].any()
    flat = np.full(shape, 500, np.int32)
    flat[20, 70] = 0
    out, _ = assert_morph(flat, device, wall, steps=16, ops=(0,))
    assert (out[:, :66] == 500).all() and out[20, 67] == 0               # the erosion does not see through the wall
    alone = np.zeros(shape, np.uint8)
    alone[31, 63], alone[0, 0], alone[39, 149] = 1, 1, 1                 # inside pixels all of whose neighbours are outside
    out, _ = assert_morph(image, device, alone, steps=7)
    assert np.array_equal(out, np.where(alone, image, 0))
    out, bad = assert_morph(image, device, np.zeros(shape, np.uint8), steps=3)
    assert not out.any() and bad == 0


def test_morph_bad_bit(device):
    _, image, mask = scene((35, 70), 5, top=MAX_LEVEL + 1)
    assert assert_morph(image, device, mask, steps=2)[1] == 0
    for value in (-1, MAX_LEVEL + 1, 2 ** 31 - 1, -2 ** 31):
        dirty = image.copy()
        dirty[33, 65] = value
        inside = mask.copy()
        inside[33, 65] = 1
        out, bad = assert_morph(dirty, device, inside, steps=2)
        assert bad == 1
        inside[33, 65] = 0                                              # under an outside pixel the value does not count
        assert assert_morph(dirty, device, inside, steps=2)[1] == 0
        assert assert_morph(dirty, device, None, steps=1)[1] == 1


def test_morph_more_tiles_than_blocks(device):
    shape = (2, MORPH_2D[1] * TILE_MAX_GRID + 1)
    assert -(-shape[0] // MORPH_2D[0]) * -(-shape[1] // MORPH_2D[1]) == TILE_MAX_GRID + 1      # one block makes a second trip
    image = random_levels(np.random.default_rng(8), shape, 60000)
    assert_morph(image, device, steps=3)
    assert_morph(image, device, steps=16, ops=(0,))


def test_morph_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    image = torch.arange(64, dtype=torch.int32, device=device)
    mask = torch.ones(64, dtype=torch.uint8, device=device)
    outs = dict(out=Out((64,), np.int32, device), bad=Out((1,), np.int32, device))
    null = ctypes.c_void_p(0)

    def morph(nd=2, Z=1, Y=8, X=8, op=0, steps=1, **ptrs):
        p = {k: o.ptr for k, o in outs.items()}
        p.update(image=_clx.ptr(image), mask=_clx.ptr(mask))
        p.update(ptrs)
        return lib.clx_grey_morph(p["image"], p["mask"], nd, Z, Y, X, op, steps, p["out"], p["bad"], st)

    refused = [dict(nd=1), dict(nd=4), dict(Z=2), dict(Y=0), dict(X=-8), dict(nd=3, Z=0), dict(op=2), dict(op=-1), dict(steps=0), dict(steps=17),
               dict(nd=3, Z=2, Y=4, steps=5), dict(Y=65536, X=65536), dict(nd=3, Z=2, Y=46341, X=46341), dict(out=_clx.ptr(image)),
               dict(out=_clx.ptr(mask))]
    refused += [{k: null} for k in ("image", "out", "bad")]
    for kw in refused:
        assert morph(**kw) == -1, f"{kw} was accepted"
        assert lib.clx_last_error().decode().startswith("clx_grey_morph:"), kw
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    host = image.cpu().numpy().reshape(8, 8)
    for kw in (dict(), dict(mask=null), dict(op=1, steps=16), dict(nd=3, Z=2, Y=4, steps=4)):       # the same buffers, valid arguments
        assert morph(**kw) == 0
        torch.cuda.synchronize(device)
        shape = (2, 4, 8) if kw.get("nd") == 3 else (8, 8)
        want = ref_morph(host.reshape(shape), None, kw.get("op", 0), kw.get("steps", 1))
        assert outs["bad"].get().tolist() == [0] and np.array_equal(outs["out"].get().reshape(shape), want[0])


# ---------------------------------------------------------------- clx_grey_reconstruct

@pytest.mark.parametrize("Y", (1, 2, 3))
def test_reconstruct_widths_1_to_67(Y, device):
    for X in range(1, 68):
        marker, image, mask = scene((Y, X), 100 * Y + X)
        assert_reconstruct(marker, image, device, mask if X % 2 else None)
    for X in (1, 5, 33, 67):
        marker, image, mask = scene((Y + 1, 3, X), X)
        assert_reconstruct(marker, image, device, mask if X % 3 else None)


@pytest.mark.parametrize("nd", (2, 3))
def test_reconstruct_shapes_around_the_tile_and_its_halo(nd, device):
    tile = RECON_2D if nd == 2 else RECON_3D
    sizes = around(tile, 2)
    shapes = set(itertools.product(*sizes)) if nd == 2 else {tuple(s if a == axis else tile[a] + 1 for a in range(3)) for axis in range(3) for s in sizes[axis]}
    for n, shape in enumerate(sorted(shapes)):
        marker, image, mask = scene(shape, n, top=8)
        assert_reconstruct(marker, image, device, mask if n % 2 else None)
        corner = np.zeros(shape, np.int32)                              # one marker in the last corner of a flat image: it fills the map
        corner[tuple(s - 1 for s in shape)] = 7
        out = assert_reconstruct(corner, np.full(shape, 9, np.int32), device, ref=ref_reconstruct_sweeps if nd == 3 else ref_reconstruct)[0]
        assert (out == 7).all()


def test_reconstruct_markers(device):
    rng = np.random.default_rng(21)
    for shape in ((40, 300), (10, 12, 70)):
        image = random_levels(rng, shape, 30)
        above = image + random_levels(rng, shape, 5) * (rng.random(shape) < 0.1)        # above the image somewhere: cut to it
        out, _, busy, _ = assert_reconstruct(above, image, device)
        assert np.array_equal(out, image) and busy == 0
        out, _, busy, calls = assert_reconstruct(np.zeros(shape, np.int32), image, device)
        assert not out.any() and busy == 0 and calls == 1
        out, _, busy, _ = assert_reconstruct(image, image, device)
        assert np.array_equal(out, image) and busy == 0
        assert_reconstruct(np.maximum(image - 3, 0), image, device)                     # h-maxima: the domes are cut by 3


def test_reconstruct_plateaus_bridges_and_doors(device):
    ty, tx = RECON_2D
    shape = (2 * ty + 6, 2 * tx + 8)
    image = np.full(shape, 5, np.int32)
    image[ty - 12:ty + 13, tx - 50:tx + 50] = 30                        # a plateau over the corner of four tiles
    image[3:8, 40:tx + 100], image[10:ty + 20, 70:75] = 22, 26          # plateaus across the seam in x and the seam in y
    marker = np.zeros(shape, np.int32)
    marker[ty + 12, tx + 49], marker[5, 41], marker[ty + 19, 72] = 30, 22, 26            # each touched at one pixel
    out = assert_reconstruct(marker, image, device)[0]
    assert np.array_equal(out, image)
    bridge = np.zeros(shape, np.int32)
    bridge[20, 10:tx - 2], bridge[20, tx - 2:tx + 2], bridge[20, tx + 2:tx + 90] = 20, 7, 25                 # a bridge of lower value between two tiles
    marker = np.zeros(shape, np.int32)
    marker[20, 10] = 20
    out = assert_reconstruct(marker, bridge, device)[0]
    assert out[20, tx - 3] == 20 and (out[20, tx - 2:tx + 90] == 7).all() and out.sum() == 20 * (tx - 12) + 7 * 92
    flat, wall = np.full(shape, 9, np.int32), np.ones(shape, np.uint8)
    wall[:, tx] = 0
    seed = np.zeros(shape, np.int32)
    seed[0, 0] = 9
    out = assert_reconstruct(seed, flat, device, wall)[0]
    assert (out[:, :tx] == 9).all() and not out[:, tx:].any()
    wall[ty + 1, tx] = 1                                                # a door of one pixel
    out = assert_reconstruct(seed, flat, device, wall)[0]
    assert np.array_equal(out, np.where(wall, 9, 0))


def corridor_case():
    path = serpentine((36, 600))
    image = np.where(path, 100, 0).astype(np.int32)
    image[path & (np.arange(600)[None, :] % 50 == 25)] = 60              # the corridor narrows: the value falls along it
    marker = np.zeros(image.shape, np.int32)
    marker[0, 0] = 100
    return marker, image


def test_reconstruct_serpentine_resumes_and_makes_the_same_rounds(device):
    marker, image = corridor_case()
    assert -(-36 // RECON_2D[0]) * -(-600 // RECON_2D[1]) >= 6           # the corridor runs through six tiles
    runs = {rounds: assert_reconstruct(marker, image, device, rounds=rounds) for rounds in (1, 2, MAX_ROUNDS)}
    assert np.array_equal(runs[1][0] > 0, image > 0) and runs[1][0][34, 0] == 60
    assert runs[2][3] > 1 and runs[1][3] == runs[1][2] + 1               # resume = 1 was needed; one call a round, the last one idle
    assert runs[1][2] == runs[2][2] == runs[MAX_ROUNDS][2] > 5           # the same rounds changed a tile, whatever the chunks
    again = run_reconstruct(marker, image, None, device, rounds=2)
    assert again[0].tobytes() == runs[2][0].tobytes() and again[1:] == runs[2][1:]
    as_mask = assert_reconstruct(marker, np.where(image > 0, 100, 50).astype(np.int32), device, (image > 0).astype(np.uint8), rounds=MAX_ROUNDS)
    assert np.array_equal(as_mask[0], np.where(image > 0, 100, 0))       # the same corridor cut by the mask from a bright image


def test_reconstruct_a_tile_at_rest_wakes_when_the_rise_reaches_its_seam(device):
    tx = RECON_2D[1]
    shape = (3, 4 * tx + 10)
    image = np.full(shape, 3, np.int32)
    image[1] = 50                                                       # a bright row through five tiles
    image[1, 2 * tx + 5] = 40
    marker = np.zeros(shape, np.int32)
    marker[1, shape[1] - 1] = 50                                         # tile 0 is at rest from round 0 on and sleeps until the rise arrives
    out, _, busy, _ = assert_reconstruct(marker, image, device, rounds=1)
    assert out[1, 0] == 40 and out[1, -1] == 50 and (out[0] == 3).all() and busy >= 5
    assert_reconstruct(marker, image, device, rounds=MAX_ROUNDS)


def test_reconstruct_extra_rounds_change_nothing(device):
    from cellulus_amd import _clx

    marker, image, mask = scene((40, 300), 77)
    image_d, marker_d, mask_d = _dev(image, device), _dev(marker, device), _dev(mask, device)
    lib = _clx.load()
    nbytes = int(lib.clx_grey_reconstruct_workspace(2, 1, 40, 300))
    outs = dict(out=Out(image.shape, np.int32, device), info=Out((3,), np.int32, device), workspace=Out((nbytes,), np.uint8, device))
    want = ref_reconstruct(marker, image, mask)[0]
    seen = []
    for resume, rounds in ((0, MAX_ROUNDS), (1, 1), (1, 2), (1, MAX_ROUNDS)):
        assert lib.clx_grey_reconstruct(_clx.ptr(marker_d), _clx.ptr(image_d), _clx.ptr(mask_d), 2, 1, 40, 300, rounds, resume, outs["out"].ptr,
                                        outs["info"].ptr, outs["workspace"].ptr, nbytes, _clx.stream_ptr(device)) == 0
        torch.cuda.synchronize(device)
        seen.append(outs["info"].get().tolist())
        assert np.array_equal(outs["out"].get(), want)
    assert seen[0][1] == 0 and 0 < seen[0][2] < MAX_ROUNDS and seen[1:] == [[0, 0, 0]] * 3


def test_reconstruct_columns_open_only_along_z(device):
    shape = (19, 5, 70)
    image = np.zeros(shape, np.int32)
    image[:, 2, 3], image[:, 4, 66], image[9, 2, 3] = 80, 90, 30          # two columns along z through three tiles, one with a neck
    marker = np.zeros(shape, np.int32)
    marker[0, 2, 3], marker[18, 4, 66] = 80, 90
    out = assert_reconstruct(marker, image, device)[0]
    assert out[:, 2, 3].tolist() == [80] * 9 + [30] * 10 and (out[:, 4, 66] == 90).all() and out.sum() == 80 * 9 + 30 * 10 + 90 * 19
    mask = np.zeros(shape, np.uint8)
    mask[:, 1, 1] = 1
    flat = np.full(shape, 11, np.int32)
    seed = np.zeros(shape, np.int32)
    seed[7, 1, 1] = 11
    assert assert_reconstruct(seed, flat, device, mask)[0].sum() == 11 * 19


def test_reconstruct_more_tiles_than_blocks(device):
    shape = (2, RECON_2D[1] * TILE_MAX_GRID + 1)
    assert -(-shape[0] // RECON_2D[0]) * -(-shape[1] // RECON_2D[1]) == TILE_MAX_GRID + 1      # one block makes a second trip
    rng = np.random.default_rng(9)
    image = random_levels(rng, shape, 6)
    marker = image * (rng.random(shape) < 0.3)
    out, _, busy, _ = assert_reconstruct(marker, image, device, ref=lambda *a: ref_reconstruct_sweeps(*a)[:2])
    assert busy >= 1 and (out != np.minimum(marker, image)).sum() > shape[1] // 10              # a tenth of a row's pixels rose, at least


def test_reconstruct_bad_bits(device):
    marker, image, mask = scene((35, 300), 6)
    assert assert_reconstruct(marker, image, device, mask)[1] == 0
    for value in (-1, MAX_LEVEL + 1, 2 ** 31 - 1, -2 ** 31):
        inside = mask.copy()
        inside[33, 257], inside[2, 2] = 1, 1
        dirty_m, dirty_i = marker.copy(), image.copy()
        dirty_m[33, 257], dirty_i[2, 2] = value, value
        assert assert_reconstruct(dirty_m, image, device, inside)[1] == 1
        out, flags, _, _ = assert_reconstruct(marker, dirty_i, device, inside)
        assert flags == 2 and out[2, 2] == 0
        assert assert_reconstruct(dirty_m, dirty_i, device, inside)[1] == 3
        assert assert_reconstruct(dirty_m, dirty_i, device, None)[1] == 3
        inside[33, 257], inside[2, 2] = 0, 0                              # under outside pixels the values do not count
        assert assert_reconstruct(dirty_m, dirty_i, device, inside)[1] == 0
    top = np.full((35, 300), MAX_LEVEL, np.int32)
    assert assert_reconstruct(top, top, device)[1] == 0


def test_reconstruct_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    image = torch.arange(64, dtype=torch.int32, device=device)
    marker = torch.zeros(64, dtype=torch.int32, device=device)
    marker[27] = 40
    mask = torch.ones(64, dtype=torch.uint8, device=device)
    exact = int(lib.clx_grey_reconstruct_workspace(2, 1, 8, 8))
    assert exact == int(lib.clx_grey_reconstruct_workspace(3, 2, 4, 8)) == 4 * (16 + 64) + 4 * 64 + 2 * 4 + 2 * 64
    for shape in ((1, 1, 8, 8), (4, 1, 8, 8), (2, 2, 8, 8), (2, 1, 0, 8), (3, 0, 8, 8), (2, 1, 65536, 65536), (3, 2, 46341, 46341)):
        assert int(lib.clx_grey_reconstruct_workspace(*shape)) == 0
    outs = dict(out=Out((64,), np.int32, device), info=Out((3,), np.int32, device), workspace=Out((exact,), np.uint8, device))
    null = ctypes.c_void_p(0)

    def reconstruct(nd=2, Z=1, Y=8, X=8, rounds=8, resume=0, nbytes=exact, **ptrs):
        p = {k: o.ptr for k, o in outs.items()}
        p.update(marker=_clx.ptr(marker), image=_clx.ptr(image), mask=_clx.ptr(mask))
        p.update(ptrs)
        return lib.clx_grey_reconstruct(p["marker"], p["image"], p["mask"], nd, Z, Y, X, rounds, resume, p["out"], p["info"], p["workspace"], nbytes, st)

    refused = [dict(nd=1), dict(nd=4), dict(Z=2), dict(Y=0), dict(X=-8), dict(nd=3, Z=0), dict(rounds=0), dict(rounds=MAX_ROUNDS + 1), dict(resume=2),
               dict(resume=-1), dict(Y=65536, X=65536, nbytes=2 ** 40), dict(nd=3, Z=2, Y=46341, X=46341, nbytes=2 ** 40), dict(nbytes=exact - 1),
               dict(nbytes=0), dict(Y=16, nbytes=exact), dict(workspace=ctypes.c_void_p(outs["workspace"].ptr.value + 2)),
               dict(out=_clx.ptr(marker)), dict(out=_clx.ptr(image)), dict(out=_clx.ptr(mask))]
    refused += [{k: null} for k in ("marker", "image", "out", "info", "workspace")]
    for kw in refused:
        assert reconstruct(**kw) == -1, f"{kw} was accepted"
        assert lib.clx_last_error().decode().startswith("clx_grey_reconstruct:"), kw
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    want = ref_reconstruct(marker.cpu().numpy().reshape(8, 8), image.cpu().numpy().reshape(8, 8))[0]
    for kw in (dict(), dict(mask=null)):                                 # the same buffers, valid arguments
        assert reconstruct(**kw) == 0
        torch.cuda.synchronize(device)
        assert outs["info"].get().tolist() == [0, 0, 1]
        assert np.array_equal(outs["out"].get().reshape(8, 8), want)
    assert reconstruct(nd=3, Z=2, Y=4) == 0 and reconstruct(resume=1, rounds=1) == 0
    torch.cuda.synchronize(device)
    outs["workspace"].get()
