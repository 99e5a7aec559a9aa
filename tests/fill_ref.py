"""The fill stage's definitions restated with scipy: scipy.ndimage.label(labels == 0, face structure) gives the components,
and per component the border test, the dilation ring, the unique values on it and the area decide.  Neither tiles nor runs
nor a union-find.  Also the maps the tests share: worked by hand (HAND), and seeded families."""

import numpy as np
from scipy import ndimage


def face_structure(nd, planewise=False):
    s = ndimage.generate_binary_structure(nd, 1)
    if planewise:
        s[0], s[2] = False, False                                        # no z neighbours
    return s


def ref_holes(labels, max_size=None, planewise=False):
    """-> (out int32, rows int64 (n, 4) = (first, owner, area, kept) sorted by first, info [holes, pixels filled, components, 0])"""
    labels = np.asarray(labels)
    nd, shape = labels.ndim, labels.shape
    assert nd in (2, 3) and not (planewise and nd == 2)
    structure = face_structure(nd, planewise)
    comp, n = ndimage.label(labels == 0, structure)
    out = labels.astype(np.int64).copy()
    rows, filled = [], 0
    border_axes = range(1, 3) if planewise else range(nd)
    for c, box in enumerate(ndimage.find_objects(comp), start=1):
        grown = tuple(slice(max(b.start - 1, 0), min(b.stop + 1, s)) for b, s in zip(box, shape))
        inside = comp[grown] == c
        where = np.argwhere(inside) + [g.start for g in grown]
        if any((where[:, a] == 0).any() or (where[:, a] == shape[a] - 1).any() for a in border_axes):
            continue
        ring = ndimage.binary_dilation(inside, structure) & ~inside
        around = np.unique(labels[grown][ring])
        assert len(around) and (around != 0).all()                       # a component is maximal: its ring holds no zero
        if len(around) != 1:
            continue
        area = int(inside.sum())
        kept = max_size is not None and max_size >= 0 and area > max_size
        rows.append((int(np.ravel_multi_index(tuple(where[0]), shape)), int(around[0]), area, int(kept)))
        if not kept:
            out[grown][inside] = around[0]
            filled += area
    rows = np.array(sorted(rows), dtype=np.int64).reshape(-1, 4)
    return out.astype(np.int32), rows, [len(rows), filled, n, 0]


def ref_hole_table(labels, max_size=None, planewise=False):
    rows = ref_holes(labels, max_size, planewise)[1]
    nd = np.ndim(labels)
    table = {"owner": rows[:, 1]}
    where = np.unravel_index(rows[:, 0], np.shape(labels))
    for axis, c in zip("zyx"[3 - nd:], where):
        table[f"first_{axis}"] = np.asarray(c, dtype=np.int64)
    table["area"], table["filled"] = rows[:, 2], 1 - rows[:, 3]
    return table


def ref_fill_table(labels, max_size=None, planewise=False):
    """the columns of fill_table from one mask per object"""
    labels = np.asarray(labels)
    out, rows, _ = ref_holes(labels, max_size, planewise)
    ids = np.unique(labels[labels != 0]).astype(np.int64)
    of = [rows[rows[:, 1] == i] for i in ids]
    column = (lambda f: np.array([f(i, r) for i, r in zip(ids, of)], dtype=np.int64).reshape(-1))
    return {"label": ids, "area_before": column(lambda i, r: (labels == i).sum()), "area": column(lambda i, r: (out == i).sum()),
            "holes_filled": column(lambda i, r: (r[:, 3] == 0).sum()), "filled_area": column(lambda i, r: r[r[:, 3] == 0, 2].sum()),
            "largest_hole": column(lambda i, r: r[:, 2].max() if len(r) else 0), "holes_kept": column(lambda i, r: (r[:, 3] == 1).sum())}


# ---------------------------------------------------------------------------------------------------------------------------
# maps worked by hand: name -> (labels, planewise, the pixels filled with their value {index: value}, components, rows)
# ---------------------------------------------------------------------------------------------------------------------------
def _ones(shape, zeros=(), others=()):
    m = np.ones(shape, np.int32)
    for p in zeros:
        m[p] = 0
    for p, v in others:
        m[p] = v
    return m


def _hand():
    cases = {}
    # two zero regions that touch only diagonally; (0, 0) reaches the border, (1, 1) does not: two components, one hole
    cases["diagonal_touch"] = (_ones((5, 5), [(0, 0), (1, 1)]), False, {(1, 1): 1}, 2, [(6, 1, 1, 0)])
    # a diagonal neighbour of another label does not count: still a hole of 1
    cases["diagonal_other_label"] = (_ones((5, 5), [(2, 2)], [((1, 1), 2)]), False, {(2, 2): 1}, 1, [(12, 1, 1, 0)])
    # a face neighbour of another label: a gap between two labels, not a hole
    cases["face_other_label"] = (_ones((5, 5), [(2, 2)], [((2, 3), 2)]), False, {}, 1, [])
    ring = [(y, x) for y in (2, 3, 4) for x in (2, 3, 4) if (y, x) != (3, 3)]
    cases["ring_same_island"] = (_ones((7, 7), ring), False, {p: 1 for p in ring}, 1, [(16, 1, 8, 0)])
    cases["ring_other_island"] = (_ones((7, 7), ring, [((3, 3), 2)]), False, {}, 1, [])
    # components that reach the border through one side only (x = X-1, y = Y-1, x = 0, y = 0), the lone corner, and one hole
    sides = [(1, 4), (1, 5), (1, 6), (5, 2), (6, 2), (3, 0), (3, 1), (0, 2), (1, 2), (6, 6)]
    hole = [(3, 3), (3, 4), (4, 3)]
    cases["one_side_each"] = (_ones((7, 7), sides + hole), False, {p: 1 for p in hole}, 6, [(24, 1, 3, 0)])
    cases["zeros_only"] = (np.zeros((5, 6), np.int32), False, {}, 1, [])
    cases["no_zero"] = (np.full((5, 6), 3, np.int32), False, {}, 0, [])
    # values are compared, never an index: the smallest and the largest int32 and one above 2^24
    wide = np.zeros((5, 9), np.int64)
    wide[:, 0:3], wide[:, 3:6], wide[:, 6:9] = -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1
    wide[2, 1] = wide[2, 4] = wide[2, 7] = 0
    cases["extreme_values"] = (wide.astype(np.int32), False, {(2, 1): -2 ** 31, (2, 4): 2 ** 31 - 1, (2, 7): 2 ** 24 + 1}, 3,
                               [(19, -2 ** 31, 1, 0), (22, 2 ** 31 - 1, 1, 0), (25, 2 ** 24 + 1, 1, 0)])
    # rows and slices never wrap: (1, 4) and (2, 0) follow each other in memory
    cases["row_ends"] = (_ones((4, 5), [(1, 4), (2, 0)]), False, {}, 2, [])
    cases["slice_ends"] = (_ones((3, 3, 4), [(0, 2, 3), (1, 0, 0)]), False, {}, 2, [])
    cases["cavity"] = (_ones((5, 5, 5), [(2, 2, 2)]), False, {(2, 2, 2): 1}, 1, [(62, 1, 1, 0)])
    cases["cavity_planewise"] = (_ones((5, 5, 5), [(2, 2, 2)]), True, {(2, 2, 2): 1}, 1, [(62, 1, 1, 0)])
    shaft = [(0, 2, 2), (1, 2, 2), (2, 2, 2)]                            # the cavity opened along z by a shaft of one voxel
    cases["cavity_open_along_z"] = (_ones((5, 5, 5), shaft), False, {}, 1, [])
    cases["cavity_open_along_z_planewise"] = (_ones((5, 5, 5), shaft), True, {p: 1 for p in shaft}, 3, [(12, 1, 1, 0), (37, 1, 1, 0), (62, 1, 1, 0)])
    torus = np.zeros((5, 7, 7), np.int32)                                # a slab with a tunnel along z, in background
    torus[1:4, 1:6, 1:6] = 4
    torus[1:4, 3, 3] = 0
    cases["torus_tunnel"] = (torus, False, {}, 1, [])
    cases["torus_tunnel_planewise"] = (torus, True, {(z, 3, 3): 4 for z in (1, 2, 3)}, 2 + 3 * 2, [(49 * z + 24, 4, 1, 0) for z in (1, 2, 3)])
    cases["one_slice"] = (_ones((1, 5, 5), [(0, 2, 2)]), False, {}, 1, [])              # z = 0 is the border
    cases["one_slice_planewise"] = (_ones((1, 5, 5), [(0, 2, 2)]), True, {(0, 2, 2): 1}, 1, [(12, 1, 1, 0)])
    return cases


HAND = _hand()


def hand_result(name):
    """-> (labels, planewise, out, rows, info) as worked by hand"""
    labels, planewise, filled, ncomp, rows = HAND[name]
    out = labels.copy()
    for p, v in filled.items():
        out[p] = v
    return labels, planewise, out, np.array(rows, dtype=np.int64).reshape(-1, 4), [len(rows), len(filled), ncomp, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# seeded families
# ---------------------------------------------------------------------------------------------------------------------------
def random_map(shape, seed, block=4, nlabels=3, knock=0.2):
    """blocks of `block` pixels a side of one random label 0 .. nlabels each, with a fifth of the pixels knocked out: holes of
    one label, gaps between two, nested pieces and components on the border"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, nlabels + 1, size=tuple(-(-s // block) for s in shape))
    fine = coarse
    for axis in range(len(shape)):
        fine = np.repeat(fine, block, axis=axis)
    fine = fine[tuple(slice(0, s) for s in shape)].astype(np.int32)
    fine[rng.random(shape) < knock] = 0
    return fine


def discs_map(shape, seed, knock=0.2):
    """four isolated discs (balls), each a label of its own, with a fifth of their pixels knocked out: no enclosed component
    touches a second label"""
    rng = np.random.default_rng(seed)
    nd = len(shape)
    grid = np.indices(shape)
    out = np.zeros(shape, np.int32)
    r = min(shape[-2:]) // 4 - 2
    centres = [(shape[-2] // 4, shape[-1] // 4), (shape[-2] // 4, 3 * shape[-1] // 4), (3 * shape[-2] // 4, shape[-1] // 4),
               (3 * shape[-2] // 4, 3 * shape[-1] // 4)]
    for i, (cy, cx) in enumerate(centres):
        d = (grid[-2] - cy) ** 2 + (grid[-1] - cx) ** 2
        if nd == 3:
            d = d + (grid[0] - shape[0] // 2) ** 2
        out[d <= r * r] = i + 1
    out[(rng.random(shape) < knock) & (out > 0)] = 0
    return out


def serpentine_hole(rows=10, width=150):
    """ones around one corridor of zeros `rows` rows long that turns at alternating ends: a long union chain"""
    m = np.ones((2 * rows + 1, width), np.int32)
    for k in range(rows):
        m[2 * k + 1, 1:width - 1] = 0
        if k:
            m[2 * k, width - 2 if k % 2 else 1] = 0
    return m


def comb_hole(height=12, width=140):
    """U-shaped arms: columns of zeros that only meet in the last row of the hole"""
    m = np.ones((height, width), np.int32)
    m[1:height - 1, 2:width - 2:2] = 0
    m[height - 2, 2:width - 2] = 0
    return m


def spiral_hole(n=41):
    """a corridor of zeros that winds inwards between walls of ones, one pixel wide"""
    m = np.ones((n, n), np.int32)
    y, x, dy, dx = 1, 1, 0, 1
    m[y, x] = 0
    while True:
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        if 1 <= ny < n - 1 and 1 <= nx < n - 1 and m[ny, nx] == 1 and m[ahead] == 1:
            y, x = ny, nx
            m[y, x] = 0
            continue
        dy, dx = dx, -dy                                                 # turn right
        ny, nx = y + dy, x + dx
        if not (1 <= ny < n - 1 and 1 <= nx < n - 1 and m[ny, nx] == 1 and m[ny + dy, nx + dx] == 1):
            return m
