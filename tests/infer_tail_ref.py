"""NumPy / SciPy restatement of the inference tail entry points (csrc/edt.hip, greedy.hip, evaluate.hip, seeds.hip and the
run pipeline of cc_label.hip) and the inputs their tests share.  No device, no libclx.  Everything here is integer or
bit-exact float64 work; the grow/shrink and EDT references are the oracle's (scipy's EDT)."""

import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ======================================================================================================= clx_grow_shrink
GS_TILE = {2: (1, 32, 64), 3: (8, 8, 32)}       # GsTile<ND>: TZ, TY, TX
GS_LDS_LIMIT = 150 * 1024
GS_MAX_HALO_BITS, GS_MAX_HALO_TILE = 16, 24
GS_PHANTOM_THREADS = 1024 * 256                 # grow_shrink_phantom: at most 1024 blocks of 256 threads


def gs_halo(grow, shrink):
    g1 = grow - 1 if grow > 0 else 0
    s1 = shrink - 1 if shrink > 0 else 0
    return g1, s1, g1 + s1


def gs_smem_bytes(nd, grow, shrink):
    """gs_smem_bytes<ND> of csrc/edt.hip: the LDS request of grow_shrink_tile_kernel"""
    TZ, TY, TX = GS_TILE[nd]
    g1, s1, H = gs_halo(grow, shrink)
    hz = 1 if nd == 3 else 0
    Z0, Y0, X0 = TZ + 2 * H * hz, TY + 2 * H, TX + 2 * H
    Z1, Y1, X1 = TZ + 2 * s1 * hz, TY + 2 * s1, TX + 2 * s1
    return ((Z0 * Y0 * X0 + 15) & ~15) + ((Z1 * Y1 * X1 + 15) & ~15) + 2 * (((Z0 * Y0 * X1 + 7) & ~7) + Z0 * Y1 * X1 + 8)


def gs_path(shape, grow, shrink, seg_lead=0, ws_lead=0):
    """the dispatch of clx_grow_shrink: "bits4" / "bits" (bit rows, by the kernel that packs the rows), "tile2" / "tile3"
    (grow_shrink_tile_kernel) or "generic" (the capped EDT passes).  seg_lead / ws_lead: bytes past a 16-byte boundary."""
    Z, Y, X = (1,) * (3 - len(shape)) + tuple(shape)
    g1, s1, H = gs_halo(grow, shrink)
    three_d = Z > 1
    if not three_d and H <= GS_MAX_HALO_BITS and ws_lead % 16 == 0:
        return "bits4" if X % 4 == 0 and seg_lead % 16 == 0 else "bits"
    smem = gs_smem_bytes(3 if three_d else 2, grow, shrink)
    if H <= GS_MAX_HALO_TILE and smem <= GS_LDS_LIMIT and seg_lead % 16 == 0 and ws_lead % 16 == 0:
        return "tile3" if three_d else "tile2"
    return "generic"


def gs_images(shape, seed=7):
    """name -> int32 label image: empty, full, densities 0.003 / 0.05 / 0.6 with ids 1..8, 7-pixel blocks of ids 0..2, one
    foreground pixel in each corner, a full image with one background pixel"""
    rng = np.random.default_rng(seed + sum(shape))
    images = {"empty": np.zeros(shape, np.int32), "full": np.ones(shape, np.int32)}
    for density in (0.003, 0.05, 0.6):
        images[f"density{density}"] = ((rng.random(shape) < density) * rng.integers(1, 9, size=shape)).astype(np.int32)
    blocks = np.kron(rng.integers(0, 3, size=tuple(-(-s // 7) for s in shape)), np.ones((7,) * len(shape), int))
    images["blocks"] = blocks[tuple(slice(0, s) for s in shape)].astype(np.int32)
    corners = np.zeros(shape, np.int32)
    for k, idx in enumerate(np.ndindex(*(2,) * len(shape))):
        corners[tuple(-i for i in idx)] = k + 1                 # index 0 or -1 along every axis
    images["corners"] = corners
    hole = np.full(shape, 5, np.int32)
    hole[tuple((2 * s) // 3 for s in shape)] = 0
    images["one_background"] = hole
    return images


def _gs_cases():
    """case id -> dict(path, shape, grow, shrink, seg_lead, ws_lead, images).  The id starts with the dispatch path the
    case is meant to take; images: "all" (gs_images) or "full" (the all-foreground image only)."""
    cases = {}

    def add(path, shape, grow, shrink, seg_lead=0, ws_lead=0, images="all", tag=""):
        name = f"{path}-{grow}_{shrink}-" + "x".join(map(str, shape)) + tag
        assert name not in cases
        cases[name] = dict(path=path, shape=shape, grow=grow, shrink=shrink, seg_lead=seg_lead, ws_lead=ws_lead, images=images)

    for grow, shrink in ((10, 9), (9, 10), (13, 13), (12, 14), (1, 25), (25, 1)):      # 17 <= H <= 24: the 2-D tile kernel
        for shape in ((1, 5), (33, 65), (70, 131), (97, 256)):
            add("tile2", shape, grow, shrink)
    for grow, shrink in ((9, 9), (1, 17), (17, 1)):                                     # H = 16: 32 rows per wavefront
        add("bits4", (70, 132), grow, shrink)
        add("bits", (70, 132), grow, shrink, seg_lead=4, tag="-seg4")
        add("bits", (33, 65), grow, shrink)
    for grow, shrink in ((7, 5), (2, 8), (12, 2)):                                      # 149 584 / 151 504 / 152 160 B of LDS
        for shape in ((9, 9, 33), (3, 17, 70)):
            add("tile3", shape, grow, shrink)
    for grow, shrink in ((9, 4), (4, 7), (6, 6)):                                       # 156 400 / 156 672 / 162 592 B: too much
        for shape in ((9, 9, 33), (3, 17, 70)):
            add("generic", shape, grow, shrink)
    add("generic", (9, 9, 33), 3, 6, seg_lead=4, tag="-seg4")
    add("generic", (33, 65), 3, 6, ws_lead=8, tag="-ws8")
    add("generic", (9, 9, 33), 3, 6, ws_lead=8, tag="-ws8")
    add("bits", (515, 521), 3, 6, images="full", tag="-phantom")
    add("tile2", (515, 521), 13, 13, images="full", tag="-phantom")
    add("tile3", (20, 120, 115), 3, 6, images="full", tag="-phantom")
    # planes larger than one grid of the phantom pass: the voxels it clears in slice 1 are reached on its second trip only
    add("tile3", (2, 520, 510), 3, 6, images="full", tag="-phantom")
    return cases


GS_CASES = _gs_cases()

# ============================================================================================================ clx_edt_sq
EDT_SHAPES = [(1, 1), (1, 40), (40, 1), (2, 2, 2), (3, 1, 40), (5, 33, 65)]
EDT_CAPS = [0, 1, 2, 3, 7, 100]                 # 0: unlimited; 100: larger than every extent
EDT_BIG = (2050, 2049)                          # 4 200 450 pixels: past the 16384 x 256 threads of one grid
EDT_GRID_THREADS = 16384 * 256


def edt_masks(shape, seed=3):
    """name -> uint8 mask: all ones (no zero anywhere: scipy's phantom zero), all zeros, one zero in each corner, one
    non-zero pixel, density 0.5"""
    rng = np.random.default_rng(seed + sum(shape))
    masks = {"ones": np.ones(shape, np.uint8), "zeros": np.zeros(shape, np.uint8)}
    corners = np.ones(shape, np.uint8)
    for idx in np.ndindex(*(2,) * len(shape)):
        corners[tuple(-i for i in idx)] = 0
    masks["corner_zeros"] = corners
    single = np.zeros(shape, np.uint8)
    single[tuple(s // 2 for s in shape)] = 1
    masks["one_nonzero"] = single
    masks["density0.5"] = (rng.random(shape) < 0.5).astype(np.uint8)
    return masks


# ==================================================================================================== clx_greedy_cluster
GREEDY_BLOCK = 1024                             # threads of the one workgroup
GREEDY_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000]
GREEDY_TYPES = [(np.float32, 2), (np.float32, 3), (np.float64, 2), (np.float64, 3)]
GREEDY_MARGIN = 1e-5                            # see test_cpu_infer_tail.test_greedy_margin_of_every_case


def greedy_points_ref(emb, seedmap, bw, min_object_size, seed_thresh, min_unclustered_sum, dtype, log=None):
    """the loop of oracle.infer_oracle.greedy_cluster on a point set: emb (ND, n), seedmap (n,), arithmetic in `dtype`.
    -> (instance (n,) int32, n_objects, n_iterations).  log (a dict, optional) receives: margin = the smallest
    |exp(-acc) - 0.5| met, evaluated in float64; seeds = the picked indices; size_rejects, ratio_rejects, exact_half =
    the numbers of proposals refused for their size, for a ratio below 1/2 and for a ratio of exactly 1/2."""
    dt = np.dtype(dtype).type
    e = np.asarray(emb, dtype=dt)
    sm = np.asarray(seedmap, dtype=dt)
    nd, n = e.shape
    assert sm.shape == (n,)
    unclustered = np.ones(n, dtype=np.int64)
    inst = np.zeros(n, dtype=np.int32)
    count, iterations = 1, 0
    two_bw2 = dt(2 * (bw ** 2))
    two_bw2_64 = 2.0 * (float(bw) ** 2)
    info = dict(margin=np.inf, seeds=[], size_rejects=0, ratio_rejects=0, exact_half=0)
    while unclustered.sum() > min_unclustered_sum:
        s = sm * unclustered.astype(dt)
        seed = int(np.argmax(s))
        if float(s[seed]) < seed_thresh:
            break
        iterations += 1
        info["seeds"].append(seed)
        center = e[:, seed:seed + 1]
        unclustered[seed] = 0
        acc = np.zeros(n, dtype=dt)
        acc64 = np.zeros(n, dtype=np.float64)
        for d in range(nd):
            df = e[d] - center[d]
            acc = acc + (df * df) / two_bw2
            df64 = e[d].astype(np.float64) - np.float64(center[d, 0])
            acc64 += df64 * df64 / two_bw2_64
        info["margin"] = min(info["margin"], float(np.abs(np.exp(-acc64) - 0.5).min()))
        proposal = np.exp(dt(-1) * acc) > dt(0.5)
        n_prop, n_unc = int(proposal.sum()), int(unclustered[proposal].sum())
        if n_prop > min_object_size:
            if np.float32(n_unc) / np.float32(n_prop) > 0.5:
                inst[proposal] = count
                count += 1
            elif 2 * n_unc == n_prop:
                info["exact_half"] += 1
            else:
                info["ratio_rejects"] += 1
        else:
            info["size_rejects"] += 1
        unclustered[proposal] = 0
    if log is not None:
        log.update(info)
    return inst, count - 1, iterations


def greedy_cloud(n, nd, dtype, seed):
    """n points on the lattice of multiples of 1/4 (exact in float32) in a box that holds about four points per unit
    volume, and n distinct seed scores in [0.05, 1).  -> (emb (nd, n), seedmap (n,))"""
    rng = np.random.default_rng(seed)
    side = max(2.0, (max(n, 1) / 4.0) ** (1.0 / nd))
    emb = rng.integers(0, int(4 * side) + 1, size=(nd, n)).astype(np.float64) / 4.0
    score = 0.05 + 0.95 * (rng.permutation(n) + 0.5) / max(n, 1)
    return emb.astype(dtype), score.astype(dtype)


def greedy_ties(nd, dtype):
    """2049 points whose seed map has equal maxima 0.875 at {3, 67, 1027} -- one step apart, so the pick of 3 clusters all
    three -- and then equal maxima 0.75 at {1500, 476}.  The picks must be 3, then 476: the points TIE_WITNESSES (low
    scores, never seeds) lie two steps from 3 / 476 and one step from 67, 1027 / 1500, inside the ball of the wrong pick
    only, so a wrong pick shows in the instance map."""
    emb, score = greedy_cloud(2049, nd, dtype, 41)
    score = (score * dtype(0.5)).astype(dtype)                  # everything else below 0.5
    p, q, r = TIE_WITNESSES
    emb[:, [3, 67, 1027, p, q]] = 200.0
    emb[0, 67] += 1.0
    emb[1, 1027] += 1.0
    emb[0, p] += 2.0                                            # beside 67
    emb[1, q] += 2.0                                            # beside 1027
    emb[:, [476, 1500, 2000, r]] = 300.0                        # 2000 keeps its low score: two of the three are unclustered
    emb[0, 1500] += 1.0
    emb[0, r] += 2.0                                            # beside 1500
    score[[3, 67, 1027]] = 0.875
    score[[1500, 476]] = 0.75
    return emb, score


TIE_WITNESSES = (10, 11, 12)


def greedy_rejections(nd, dtype):
    """a point set (bandwidth GREEDY_BW, min_object_size 4) in which the reference refuses one proposal for its size, one
    for a ratio below 1/2 and one for a ratio of exactly 1/2, followed by a cloud of 1400 points far away.  The ball of
    GREEDY_BW has radius^2 < 2.3428: a point 1.5 from a centre is inside, one 2.75 from it outside.
      A (0, 0) x5 score 0.99 + 10 points at (1.5, 0): accepted; then B (2.75, 0) x3: proposal = 10 clustered + 3 -> 2 / 13
      C (20, 0) x5 score 0.98 + 4 points at (21.5, 0): accepted; then D (22.75, 0) x6: proposal = 4 clustered + 6 -> 5 / 10
      E (40, 0) x3: 3 points, not more than min_object_size"""
    groups = [((0.0, 0.0), 5, 0.99), ((1.5, 0.0), 10, 0.30), ((2.75, 0.0), 3, 0.97),
              ((20.0, 0.0), 5, 0.98), ((21.5, 0.0), 4, 0.31), ((22.75, 0.0), 6, 0.96), ((40.0, 0.0), 3, 0.95)]
    pts, sc = [], []
    for (x, y), k, s in groups:
        for j in range(k):
            pts.append((x, y) + (0.0,) * (nd - 2))
            sc.append(s - 0.001 * j)                            # the first point of a group is its seed
    cloud, cscore = greedy_cloud(1400, nd, np.float64, 43)
    emb = np.concatenate([np.array(pts).T, cloud + 100.0], axis=1)
    score = np.concatenate([np.array(sc), cscore * 0.9])
    order = np.random.default_rng(44).permutation(emb.shape[1])  # the constructed points spread over the threads
    return emb[:, order].astype(dtype), score[order].astype(dtype)


GREEDY_BW = 1.3


def _greedy_cases():
    """case id -> dict(build = (function, args), bw, min_object_size, seed_thresh, min_unclustered_sum); the four
    (dtype, ND) instantiations are applied by the tests"""
    cases = {}
    for n in GREEDY_SIZES:
        cases[f"n{n}"] = dict(build=(greedy_cloud, (n,), 100 + n), bw=GREEDY_BW, min_object_size=3, seed_thresh=0.2,
                              min_unclustered_sum=0)
    cases["constant_seedmap"] = dict(build=("constant", (2049,), 7), bw=GREEDY_BW, min_object_size=3, seed_thresh=0.5,
                                     min_unclustered_sum=0)
    cases["ties"] = dict(build=(greedy_ties, (), None), bw=GREEDY_BW, min_object_size=0, seed_thresh=0.6, min_unclustered_sum=0)
    cases["rejections"] = dict(build=(greedy_rejections, (), None), bw=GREEDY_BW, min_object_size=4, seed_thresh=0.0,
                               min_unclustered_sum=0)
    for mus in (0, 5, 1500):
        cases[f"min_unclustered{mus}"] = dict(build=(greedy_cloud, (1500,), 9), bw=GREEDY_BW, min_object_size=3,
                                              seed_thresh=0.0, min_unclustered_sum=mus)
    cases["seed_thresh_above_all"] = dict(build=(greedy_cloud, (1500,), 9), bw=GREEDY_BW, min_object_size=3, seed_thresh=2.0,
                                          min_unclustered_sum=0)
    cases["integer_lattice_bw7"] = dict(build=("integer", (3000,), 11), bw=7.0, min_object_size=10, seed_thresh=0.3,
                                        min_unclustered_sum=0)
    return cases


GREEDY_CASES = _greedy_cases()


def greedy_inputs(name, dtype, nd):
    """-> (emb (nd, n), seedmap (n,)) of GREEDY_CASES[name] for one instantiation"""
    fn, args, seed = GREEDY_CASES[name]["build"]
    if fn == "constant":
        emb, score = greedy_cloud(args[0], nd, dtype, seed)
        return emb, np.full_like(score, 0.75)
    if fn == "integer":
        rng = np.random.default_rng(seed)
        n = args[0]
        emb = rng.integers(0, 60, size=(nd, n)).astype(dtype)
        return emb, (0.05 + 0.95 * (rng.permutation(n) + 0.5) / n).astype(dtype)
    if seed is None:
        return fn(nd, dtype)
    return fn(*args, nd, dtype, seed)


_greedy_ref_cache = {}


def greedy_ref(name, dtype, nd):
    """(instance, n_objects, n_iterations, log) of a case, computed once"""
    key = (name, np.dtype(dtype).name, nd)
    if key not in _greedy_ref_cache:
        c = GREEDY_CASES[name]
        emb, score = greedy_inputs(name, dtype, nd)
        log = {}
        inst, n_obj, n_it = greedy_points_ref(emb, score, c["bw"], c["min_object_size"], c["seed_thresh"], c["min_unclustered_sum"],
                                              dtype, log)
        _greedy_ref_cache[key] = (inst, n_obj, n_it, log)
    return _greedy_ref_cache[key]


# ======================================================================== clx_label_presence / clx_joint_histogram
EVAL_SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
EVAL_GRID_THREADS = 2048 * 256
PRESENCE_BIG = EVAL_GRID_THREADS * 4 + 4 * 300 + 3          # the loop repeats for 300 threads, plus a 3-pixel tail
JOINT_BIG = EVAL_GRID_THREADS * 8 + 8 * 300 + 5
NID = 1 << 16


def sparse_ids(seed, k=40):
    """k ids in [0, 65536), 0 and 65535 among them"""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(1, NID - 1), size=k - 2, replace=False)
    return np.concatenate([[0, NID - 1], ids]).astype(np.int32)


def label_maps(n, seed):
    """name -> (pred, gt), int32 maps of n pixels: constant; alternating every pixel in pred only / in gt only / in both;
    runs of 3 and of 5 (they straddle the 4- and 8-pixel groups of the kernels); blocky random with sparse ids"""
    i = np.arange(n)
    ids = sparse_ids(seed)
    rng = np.random.default_rng(seed + 1)
    const = np.full(n, 9, np.int32)
    alt = np.where(i % 2 == 0, 3, 60000).astype(np.int32)
    maps = {"constant": (const, np.full(n, 4, np.int32)),
            "alternating_pred": (alt, const),
            "alternating_gt": (const, alt),
            "alternating_both": (alt, np.where(i % 2 == 0, 65535, 0).astype(np.int32)),
            "runs_3_5": (ids[(i // 3) % len(ids)], ids[(i // 5) % len(ids)]),
            "runs_5_3": (ids[(i // 5) % len(ids)], ids[(i // 3) % len(ids)])}
    nb13, nb17 = n // 13 + 1, n // 17 + 1
    maps["blocky"] = (np.repeat(ids[rng.integers(0, len(ids), nb13)], 13)[:n], np.repeat(ids[rng.integers(0, len(ids), nb17)], 17)[:n])
    return {k: (np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(g, dtype=np.int32)) for k, (p, g) in maps.items()}


def presence_prefill(nid=NID):
    """a pattern of 0s and 1s"""
    return ((np.arange(nid) * 7) % 5 == 0).astype(np.int32)


def ref_presence(lab, nid, present_in):
    """-> (present, bad): present_in with a 1 at every id of `lab` in [0, nid); bad = 1 if any id lies outside"""
    ids = np.unique(lab).astype(np.int64)
    ok = (ids >= 0) & (ids < nid)
    present = np.array(present_in, dtype=np.int32, copy=True)
    present[ids[ok]] = 1
    return present, int(not ok.all())


def row_col_maps(nrow, ncol, nid=NID):
    """non-identity, many-to-one id -> row and id -> column tables"""
    ids = np.arange(nid, dtype=np.int64)
    return ((ids * 7 + 3) % nrow).astype(np.int32), ((ids * 5 + 1) % ncol).astype(np.int32)


def joint_prefill(nrow, ncol):
    """a known non-zero pattern"""
    return ((np.arange(nrow * ncol, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1000) + np.uint64(1)).reshape(nrow, ncol)


def ref_joint(pred, gt, prow, gcol, ncol, joint_in):
    """joint_in + the counts of (prow[pred], gcol[gt]), by one np.bincount of the combined index"""
    nrow = joint_in.shape[0]
    cell = prow[pred].astype(np.int64) * ncol + gcol[gt].astype(np.int64)
    return joint_in + np.bincount(cell, minlength=nrow * ncol).astype(np.uint64).reshape(nrow, ncol)


def ref_joint_histogram(pred, gt):
    """(pred ids, gt ids, joint int64) as joint_histogram_on_device returns them: np.unique + np.bincount"""
    p_ids, p_inv = np.unique(pred, return_inverse=True)
    g_ids, g_inv = np.unique(gt, return_inverse=True)
    cell = np.asarray(p_inv).ravel().astype(np.int64) * len(g_ids) + np.asarray(g_inv).ravel()
    return p_ids, g_ids, np.bincount(cell, minlength=len(p_ids) * len(g_ids)).reshape(len(p_ids), len(g_ids)).astype(np.int64)


# ====================================================== clx_offset_magnitude / clx_gaussian_filter_f64 / clx_negate_f64
SEEDS_GRID_THREADS = 16384 * 256
SEEDS_BIG = SEEDS_GRID_THREADS + 777
GAUSS_RADII = [0, 1, 8, 20]
GAUSS_EXTENTS = [1, 2, 3, 5, 17]


def gauss_shapes():
    """every 2-D shape with extents from GAUSS_EXTENTS, and every 3-D one whose first extent is above 1: the entry point
    takes (Z, Y, X) and Z = 1 IS its 2-D filter, so the volumes with Z = 1 are the 2-D cases"""
    two = [(y, x) for y in GAUSS_EXTENTS for x in GAUSS_EXTENTS]
    three = [(z, y, x) for z in GAUSS_EXTENTS if z > 1 for y in GAUSS_EXTENTS for x in GAUSS_EXTENTS]
    return two + three


def gauss_weights(radius, kind, seed=5):
    """centre-first half of a symmetric filter of 2 radius + 1 taps: "gaussian" = gaussian_weights of sigma radius / 4
    (sigma 0.25 for radius 0 and 1), "random" = positive random weights"""
    if kind == "gaussian":
        x = np.arange(-radius, radius + 1)
        sigma = max(radius, 1) / 4.0
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        phi = phi / phi.sum()
        return np.ascontiguousarray(phi[radius:])
    return np.random.default_rng(seed + radius).random(radius + 1) + 0.01


def ref_gaussian(img, w):
    """scipy.ndimage.correlate1d per axis, in axis order, mode "reflect", with the full symmetric weight vector"""
    from scipy.ndimage import correlate1d

    full = np.concatenate([w[:0:-1], w])
    out = np.asarray(img, dtype=np.float64)
    for ax in range(out.ndim):
        out = correlate1d(out, full, axis=ax, mode="reflect")
    return out


def ref_magnitude(emb):
    """sqrt((x0^2 + x1^2) + x2^2 ...) in float64, summed in channel order"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = emb[0] * emb[0]
        for c in range(1, emb.shape[0]):
            s = s + emb[c] * emb[c]
        return np.sqrt(s)


def magnitude_values(nd, n, seed):
    """(nd, n) float64: normal values of both signs, and in the first pixels 0, -0.0, a denormal, 1e200 (its square
    overflows to inf, as in NumPy), negatives and NaN in every channel position"""
    rng = np.random.default_rng(seed)
    emb = rng.normal(size=(nd, n)) * 10.0
    tiny = np.nextafter(0.0, 1.0)
    special = [0.0, -0.0, tiny, -tiny, 1e200, -1e200, -3.0, np.nan, 1e-170, 1e154]
    k = 0
    for v in special:                                           # one pixel per (value, channel), the other channels normal
        for c in range(nd):
            if k < n:
                emb[c, k] = v
                k += 1
    for v in (0.0, -0.0, tiny, 1e-170, 1e154, -1e200, np.nan):  # ... and pixels with the value in every channel
        if k < n:
            emb[:, k] = v
            k += 1
    return emb


def negate_values(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=n)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, np.nextafter(0.0, 1.0), -np.nextafter(0.0, 1.0)]
    v[:min(n, len(special))] = special[:n]
    if n > len(special):
        v[-1] = -0.0
    return v


# =================================================================================================== clx_cc_label_filter
CC_GRID_THREADS = 8192 * 256
CC_BIG = (33, 250, 260)                         # 2 145 000 voxels, 41 250 row segments of 64: both past one grid


def cc_big_volume(seed=13):
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 3, size=tuple(-(-s // 7) for s in CC_BIG)), np.ones((7, 7, 7), int))
    return blocks[tuple(slice(0, s) for s in CC_BIG)].astype(np.int32)


BOX_SIZES = (1, 4, 9, 30)


def cc_boxes(nd):
    """isolated boxes of 1, 4, 9 and 30 pixels with ids 1..4.  2-D: (20, 24), 16-byte rows; 3-D: (6, 12, 13)"""
    if nd == 2:
        seg = np.zeros((20, 24), np.int32)
        seg[1, 1], seg[3:5, 4:6], seg[8:11, 10:13], seg[13:18, 16:22] = 1, 2, 3, 4
    else:
        seg = np.zeros((6, 12, 13), np.int32)
        seg[0, 0, 0], seg[2, 2:4, 3:5], seg[4, 6:9, 7:10], seg[0:2, 8:11, 0:5] = 1, 2, 3, 4
    assert tuple(int((seg == i).sum()) for i in (1, 2, 3, 4)) == BOX_SIZES
    return seg


def cc_extreme_labels(nd):
    """touching stripes of the labels -1, INT_MIN, INT_MAX and 1 (all foreground, all distinct) beside background"""
    shape = (12, 16) if nd == 2 else (4, 9, 16)
    seg = np.zeros(shape, np.int32)
    seg[..., 0:3], seg[..., 3:6], seg[..., 6:9], seg[..., 9:12] = -1, INT_MIN, INT_MAX, 1
    seg[..., 5:7, 14] = -1                                      # a second, small component of -1
    seg[..., 0, 13] = INT_MIN                                   # a single pixel / line of INT_MIN
    return seg
