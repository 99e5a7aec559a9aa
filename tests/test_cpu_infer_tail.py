"""CPU tier of the inference-tail tests (no kernel is launched): the references of tests/infer_tail_ref.py against the
oracle and against independent NumPy / SciPy statements, the dispatch path every grow/shrink case id names, the distance of
every greedy case from the 0.5 threshold, and the conditions the inputs of the GPU tier claim (sizes past one grid, ties,
refused proposals)."""

import numpy as np
import pytest

import infer_tail_ref as R
from oracle import infer_oracle as IO


# ======================================================================================================= clx_grow_shrink
def test_gs_lds_requests_are_the_ones_the_dispatch_switches_on():
    table = {(7, 5): 149584, (2, 8): 151504, (12, 2): 152160, (9, 4): 156400, (4, 7): 156672, (6, 6): 162592}
    for (grow, shrink), want in table.items():
        assert R.gs_smem_bytes(3, grow, shrink) == want
        assert (want <= R.GS_LDS_LIMIT) == ((grow, shrink) in ((7, 5), (2, 8), (12, 2)))
        assert R.gs_halo(grow, shrink)[2] <= R.GS_MAX_HALO_TILE          # the LDS request alone decides
    assert R.gs_smem_bytes(2, 25, 1) <= R.GS_LDS_LIMIT and R.gs_smem_bytes(2, 1, 25) <= R.GS_LDS_LIMIT
    assert max(R.gs_smem_bytes(3, g, s) for g, s in ((3, 6), (1, 1), (0, 0), (0, 3), (2, 0), (6, 3), (-1, 4))) == 109824


@pytest.mark.parametrize("name", list(R.GS_CASES))
def test_gs_case_takes_the_path_its_id_names(name):
    c = R.GS_CASES[name]
    assert name.startswith(c["path"] + "-")
    assert R.gs_path(c["shape"], c["grow"], c["shrink"], c["seg_lead"], c["ws_lead"]) == c["path"]
    H = R.gs_halo(c["grow"], c["shrink"])[2]
    if c["path"] == "tile2":
        assert 17 <= H <= 24
    if c["path"] in ("bits", "bits4") and not name.endswith("-phantom"):
        assert H == 16 and 64 - 2 * H == 32                                # rows_per_wave at its smallest
    if c["path"] == "bits4":
        assert R.gs_path(c["shape"], c["grow"], c["shrink"], 4, 0) == "bits"   # the same image 4 bytes on: the other kernel


def test_gs_cases_cover_every_path_and_every_fallback():
    paths = {c["path"] for c in R.GS_CASES.values()}
    assert paths == {"bits4", "bits", "tile2", "tile3", "generic"}
    generic = [c for c in R.GS_CASES.values() if c["path"] == "generic"]
    assert any(c["seg_lead"] and len(c["shape"]) == 3 for c in generic)
    assert any(c["ws_lead"] and len(c["shape"]) == 2 for c in generic) and any(c["ws_lead"] and len(c["shape"]) == 3 for c in generic)
    assert any(c["path"] == "bits" and c["seg_lead"] and c["shape"][1] % 4 == 0 for c in R.GS_CASES.values())
    # the existing pairs of test_gpu_infer.py never reach the 2-D tile kernel
    for grow, shrink in ((3, 6), (1, 1), (0, 0), (0, 3), (2, 0), (6, 3), (-1, 4), (9, 9), (14, 14)):
        assert R.gs_path((97, 131), grow, shrink) in ("bits", "generic")
    for shape in ((33, 65), (70, 131), (97, 256)):                          # more than one 32 x 64 tile, ragged in x or y
        assert shape[0] > 32 and shape[1] > 64 and (shape[0] % 32 or shape[1] % 64)


def test_gs_phantom_cases_are_past_one_grid_and_one_clears_on_the_second_trip():
    phantom = {n: c for n, c in R.GS_CASES.items() if c["images"] == "full"}
    assert {c["path"] for c in phantom.values()} == {"bits", "tile2", "tile3"}
    second_trip = []
    for name, c in phantom.items():
        assert int(np.prod(c["shape"])) > R.GS_PHANTOM_THREADS
        full = np.ones(c["shape"], np.int32)
        ref = IO.grow_shrink(full, c["grow"], c["shrink"])
        cleared = np.flatnonzero(ref.reshape(-1) == 0)
        assert len(cleared) > 0                                             # scipy's phantom zero clears the first corner
        if cleared.max() >= R.GS_PHANTOM_THREADS:
            second_trip.append(name)
    # The phantom distance is (first axis + 1)^2 + others^2: in 2-D and in a volume of small planes every cleared pixel has
    # a raster index below 262 144.  Only a volume whose planes are larger than one grid has any on the second trip.
    assert second_trip == ["tile3-3_6-2x520x510-phantom"]


def test_gs_images():
    for shape in ((1, 5), (33, 65), (9, 9, 33)):
        images = R.gs_images(shape)
        assert list(images) == ["empty", "full", "density0.003", "density0.05", "density0.6", "blocks", "corners", "one_background"]
        assert not images["empty"].any() and images["full"].all()
        assert (images["one_background"] == 0).sum() == 1
        corners = images["corners"]
        assert (corners != 0).sum() == int(np.prod([min(s, 2) for s in shape]))
        for idx in np.ndindex(*(2,) * len(shape)):
            assert corners[tuple(-i for i in idx)] != 0
        assert all(im.dtype == np.int32 and im.shape == shape for im in images.values())
        assert 1 <= images["density0.6"].max() <= 8 and (images["density0.6"].max() == 8 or shape == (1, 5))


# ============================================================================================================ clx_edt_sq
def test_edt_fixtures():
    assert int(np.prod(R.EDT_BIG)) > R.EDT_GRID_THREADS
    assert max(R.EDT_CAPS) > max(max(s) for s in R.EDT_SHAPES)
    for shape in R.EDT_SHAPES:
        masks = R.edt_masks(shape)
        assert masks["ones"].all() and not masks["zeros"].any() and masks["one_nonzero"].sum() == 1
        assert (IO.edt_sq(masks["zeros"]) == 0).all()
        ref = IO.edt_sq(masks["ones"])                                      # the phantom zero at index -1 of the first axis
        idx = np.indices(shape)
        assert np.array_equal(ref, (idx[0] + 1) ** 2 + sum(idx[k] ** 2 for k in range(1, len(shape))))
        for idx in np.ndindex(*(2,) * len(shape)):
            assert masks["corner_zeros"][tuple(-i for i in idx)] == 0


# ==================================================================================================== clx_greedy_cluster
def test_greedy_points_ref_equals_the_oracle_on_an_image():
    rng = np.random.default_rng(5)
    for nd, shape, dtype in ((2, (24, 30), np.float32), (3, (6, 12, 14), np.float64), (3, (6, 12, 14), np.float32)):
        centres = np.array([[s * f for s in shape] for f in (0.25, 0.7)])
        grids = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"))      # axis order
        nearest = np.argmin([sum((grids[a] - c[a]) ** 2 for a in range(nd)) for c in centres], axis=0)
        pred = np.zeros((nd + 1,) + shape)
        for c in range(nd):                                                 # channel 0 = x = the last axis
            ax = nd - 1 - c
            pred[c] = centres[nearest][..., ax] - grids[ax] + np.round(rng.normal(size=shape) * 4) / 4
        pred[nd] = rng.random(shape)
        pred = pred.astype(dtype)
        mask = rng.random(shape) < 0.8
        want = IO.greedy_cluster(pred, mask, 2.3, 5, seed_thresh=0.3, min_unclustered_sum=2)
        assert want.max() >= 2
        # the oracle's preparation, then the point loop
        dt = np.float32 if (nd == 2 or pred.dtype != np.float64) else np.float64
        p = pred.astype(dt)
        emb = p[:nd].copy()
        for c in range(nd):
            ax = nd - 1 - c
            view = [1] * nd
            view[ax] = shape[ax]
            emb[c] = emb[c] + np.linspace(0, shape[ax] - 1, shape[ax], dtype=np.float32).reshape(view)
        sm = p[nd]
        sm = ((sm - sm.max()) / (sm.min() - sm.max())).astype(dt)
        inst, n_obj, n_it = R.greedy_points_ref(emb[:, mask], sm[mask], 2.3, 5, 0.3, 2, dt)
        got = np.zeros(shape, np.int64)
        got[mask] = inst
        assert np.array_equal(got, want)
        assert n_obj == want.max() and n_it >= n_obj


@pytest.mark.parametrize("dtype,nd", R.GREEDY_TYPES, ids=lambda v: getattr(v, "__name__", str(v)))
@pytest.mark.parametrize("name", list(R.GREEDY_CASES))
def test_greedy_margin_of_every_case(name, dtype, nd):
    """The device expf / exp and NumPy's are each within a few ulp of the true value, about 2e-7 near 0.5 in float32: a
    point whose exp(-acc) lies closer to 0.5 than that may fall on either side.  Every case keeps 1e-5 clear."""
    emb, score = R.greedy_inputs(name, dtype, nd)
    assert emb.dtype == dtype and score.dtype == dtype and emb.shape == (nd, len(score))
    assert np.array_equal(emb * 4, np.round(emb * 4))                       # the lattice of multiples of 1/4
    assert np.array_equal(emb.astype(np.float32).astype(dtype), emb)        # exact in float32
    inst, n_obj, n_it, log = R.greedy_ref(name, dtype, nd)
    assert log["margin"] > R.GREEDY_MARGIN, log["margin"]
    assert n_obj == inst.max(initial=0) and n_it == len(log["seeds"])


@pytest.mark.parametrize("dtype,nd", R.GREEDY_TYPES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_greedy_cases_are_what_they_claim(dtype, nd):
    # sizes: below, at and above the 64 lanes and the 1024 threads; both ends of the loop are met
    assert {0, 1, 63, 64, 65, 1023, 1024, 1025} <= set(R.GREEDY_SIZES)
    inst, n_obj, n_it, log = R.greedy_ref("n0", dtype, nd)
    assert (len(inst), n_obj, n_it) == (0, 0, 0)
    inst, n_obj, n_it, log = R.greedy_ref("n5000", dtype, nd)
    assert n_obj > 20 and n_it > n_obj and (inst == 0).any()                # left by the seed threshold with points unclustered
    # constant seed map: every pick is the lowest unclustered index
    emb, score = R.greedy_inputs("constant_seedmap", dtype, nd)
    assert len(set(score.tolist())) == 1
    inst, n_obj, n_it, log = R.greedy_ref("constant_seedmap", dtype, nd)
    assert log["seeds"][0] == 0 and log["seeds"] == sorted(log["seeds"]) and n_it > 30
    c = R.GREEDY_CASES["constant_seedmap"]
    unclustered = np.ones(len(score), bool)
    for seed in log["seeds"]:                                               # replay: each seed is the first still unclustered
        assert seed == int(np.flatnonzero(unclustered)[0])
        d2 = ((emb.astype(np.float64) - emb[:, seed:seed + 1].astype(np.float64)) ** 2).sum(axis=0)
        unclustered[np.exp(-d2 / (2 * c["bw"] ** 2)) > 0.5] = False
    # ties: equal maxima in one thread's elements (3, 1027), across wavefronts (3, 67), then 476 before 1500
    emb, score = R.greedy_inputs("ties", dtype, nd)
    assert score[3] == score[67] == score[1027] == score.max()
    rest = np.delete(score, [3, 67, 1027])
    assert score[1500] == score[476] == rest.max() and (np.delete(score, [3, 67, 1027, 1500, 476]) < 0.5).all()
    assert 1027 % R.GREEDY_BLOCK == 3 and 67 // 64 != 3 // 64
    inst, n_obj, n_it, log = R.greedy_ref("ties", dtype, nd)
    assert log["seeds"] == [3, 476] and n_obj == 2
    assert set(np.flatnonzero(inst == 1)) == {3, 67, 1027} and set(np.flatnonzero(inst == 2)) == {476, 1500, 2000}
    # ... and any other pick would have shown: each witness lies in the ball of a wrong maximum only
    radius2 = 2 * R.GREEDY_BW ** 2 * np.log(2)
    dist2 = lambda a, b: float(((emb[:, a].astype(np.float64) - emb[:, b].astype(np.float64)) ** 2).sum())      # noqa: E731
    p, q, r = R.TIE_WITNESSES
    for right, wrong, witness in ((3, 67, p), (3, 1027, q), (476, 1500, r)):
        assert dist2(right, witness) > radius2 > dist2(wrong, witness) and dist2(right, wrong) < radius2
        assert inst[witness] == 0 and score[witness] < 0.5
    # refused proposals
    inst, n_obj, n_it, log = R.greedy_ref("rejections", dtype, nd)
    assert log["size_rejects"] >= 1 and log["ratio_rejects"] >= 1 and log["exact_half"] >= 1
    emb, score = R.greedy_inputs("rejections", dtype, nd)
    first = [int(np.flatnonzero((emb[0] == x) & (emb[1] == 0))[np.argmax(score[(emb[0] == x) & (emb[1] == 0)])])
             for x in (0.0, 20.0, 2.75, 22.75, 40.0)]
    assert log["seeds"][:5] == first                                        # A, C accepted; B (2 / 13), D (5 / 10), E (3 points)
    assert n_obj >= 2 and (inst[emb[0] == 2.75] == 0).all() and (inst[emb[0] == 22.75] == 0).all() and (inst[emb[0] == 40.0] == 0).all()
    assert (inst[emb[0] == 1.5] == 1).all() and (inst[emb[0] == 21.5] == 2).all()
    # min_unclustered_sum and the seed threshold
    n = 1500
    its = [R.greedy_ref(f"min_unclustered{m}", dtype, nd)[2] for m in (0, 5, n)]
    assert its[0] >= its[1] > its[2] == 0
    assert R.greedy_ref("seed_thresh_above_all", dtype, nd)[1:3] == (0, 0)


# ======================================================================== clx_label_presence / clx_joint_histogram
def test_eval_sizes_repeat_the_loops():
    assert R.PRESENCE_BIG // 4 > R.EVAL_GRID_THREADS and R.PRESENCE_BIG % 4 == 3
    assert R.JOINT_BIG // 8 > R.EVAL_GRID_THREADS and R.JOINT_BIG % 8 == 5
    assert {n % 4 for n in R.EVAL_SMALL} == {0, 1, 2, 3} and {n % 8 for n in R.EVAL_SMALL} >= {0, 1, 7}


@pytest.mark.parametrize("n", [1, 17, 4099])
def test_eval_references_equal_the_oracle(n):
    for name, (pred, gt) in R.label_maps(n, 3).items():
        assert pred.shape == gt.shape == (n,) and pred.min() >= 0 and pred.max() < R.NID, name
        p_ids, g_ids, joint = R.ref_joint_histogram(pred, gt)
        o_p, o_g, o_joint = IO.joint_histogram(pred, gt)
        assert np.array_equal(p_ids, o_p) and np.array_equal(g_ids, o_g) and np.array_equal(joint, o_joint), name
        # presence = np.unique; the row / column tables fold the joint histogram
        prefill = R.presence_prefill()
        present, bad = R.ref_presence(pred, R.NID, prefill)
        assert bad == 0 and np.array_equal(present, np.maximum(prefill, np.isin(np.arange(R.NID), p_ids).astype(np.int32)))
        assert set(np.unique(prefill).tolist()) == {0, 1}
        for nrow, ncol in ((37, 11), (5, 1)):
            prow, gcol = R.row_col_maps(nrow, ncol)
            assert not np.array_equal(prow[:nrow], np.arange(nrow))
            table = R.ref_joint(pred, gt, prow, gcol, ncol, R.joint_prefill(nrow, ncol))
            want = R.joint_prefill(nrow, ncol).astype(np.int64)
            np.add.at(want, (prow[pred], gcol[gt]), 1)
            assert np.array_equal(table.astype(np.int64), want) and (R.joint_prefill(nrow, ncol) > 0).all(), name
    for poison in (-1, R.INT_MIN, R.NID, R.INT_MAX):
        lab = np.array([3, poison, 5], dtype=np.int32)
        present, bad = R.ref_presence(lab, R.NID, np.zeros(R.NID, np.int32))
        assert bad == 1 and np.array_equal(np.flatnonzero(present), [3, 5])


# ====================================================== clx_offset_magnitude / clx_gaussian_filter_f64 / clx_negate_f64
def test_ref_gaussian_equals_scipy_gaussian_filter_and_an_explicit_padded_sum():
    from scipy.ndimage import gaussian_filter

    from cellulus_amd.detect import gaussian_weights

    rng = np.random.default_rng(2)
    w, radius = gaussian_weights(2.0)
    assert radius == 8
    for shape in ((17, 5), (3, 17, 2), (1, 40)):
        img = rng.random(shape)
        assert np.array_equal(R.ref_gaussian(img, w).view(np.uint64), gaussian_filter(img, sigma=2).view(np.uint64))
    # radius > 2 x extent: several reflection periods.  np.pad "symmetric" is scipy's "reflect" (d c b a | a b c d)
    for n in (1, 2, 3, 5):
        for radius in (1, 8, 20):
            w = R.gauss_weights(radius, "random")
            line = rng.random(n)
            padded = np.pad(line, radius, mode="symmetric")
            want = np.array([line[c] * w[0] + sum((padded[radius + c - j] + padded[radius + c + j]) * w[j] for j in range(1, radius + 1))
                             for c in range(n)])
            got = R.ref_gaussian(line.reshape(1, n), np.array([1.0]))       # radius 0 with weight 1: the identity
            assert np.array_equal(got.reshape(-1), line)
            got = R.ref_gaussian(line, w)
            assert np.allclose(got, want, rtol=1e-13, atol=0)
    shapes = R.gauss_shapes()
    assert len(shapes) == 25 + 100 and all(len(s) == 2 or s[0] > 1 for s in shapes)
    assert any(max(R.GAUSS_RADII) > 2 * min(s) for s in shapes)
    for radius in R.GAUSS_RADII:
        for kind in ("gaussian", "random"):
            w = R.gauss_weights(radius, kind)
            assert w.shape == (radius + 1,) and (w > 0).all()


def test_magnitude_and_negate_fixtures():
    assert R.SEEDS_BIG > R.SEEDS_GRID_THREADS
    for nd in (1, 2, 3, 4):
        emb = R.magnitude_values(nd, 300, nd)
        want = R.ref_magnitude(emb)
        with np.errstate(over="ignore", invalid="ignore"):
            plain = np.sqrt(np.add.reduce(emb * emb, axis=0))
        ok = ~np.isnan(want)
        assert np.array_equal(want[ok], plain[ok]) and np.array_equal(np.isnan(want), np.isnan(plain))
        assert np.isinf(want).any() and np.isnan(want).any() and (want == 0).any()
        assert np.array_equal(np.isnan(want), np.isnan(emb).any(axis=0))
    v = R.negate_values(100, 1)
    bits = v.view(np.uint64)
    assert {0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000} <= set(bits.tolist())
    assert np.isnan(v).sum() == 2 and len({int(b) >> 63 for b in bits[np.isnan(v)]}) == 2       # NaNs of both signs
    assert np.array_equal((-v).view(np.uint64), bits ^ np.uint64(1 << 63))


# =================================================================================================== clx_cc_label_filter
def test_cc_fixtures():
    Z, Y, X = R.CC_BIG
    assert Z * Y * X > R.CC_GRID_THREADS and Z * Y * ((X + 63) // 64) * 64 > R.CC_GRID_THREADS
    for nd in (2, 3):
        seg = R.cc_boxes(nd)
        assert seg.shape[-1] % 4 == 0 or nd == 3
        full = IO.size_filter(seg, 1)
        assert full.max() == 4                                              # isolated: four components
        sizes = sorted(np.bincount(full.reshape(-1))[1:].tolist())
        assert tuple(sizes) == R.BOX_SIZES
        assert IO.size_filter(seg, 9).max() == 2 and IO.size_filter(seg, 10).max() == 1       # the threshold is inclusive
        ext = R.cc_extreme_labels(nd)
        assert {-1, R.INT_MIN, R.INT_MAX, 1, 0} == set(np.unique(ext).tolist())
        lab = IO.size_filter(ext, 1)
        assert lab.max() == 6 and (lab[ext != 0] > 0).all() and (lab[ext == 0] == 0).all()   # touching stripes stay apart
