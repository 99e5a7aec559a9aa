"""The inference tail through the C ABI on every dispatch path: clx_grow_shrink / clx_edt_sq (csrc/edt.hip),
clx_greedy_cluster (greedy.hip), clx_label_presence / clx_joint_histogram (evaluate.hip), clx_offset_magnitude /
clx_gaussian_filter_f64 / clx_negate_f64 (seeds.hip) and the run pipeline of clx_cc_label_filter (cc_label.hip) against
NumPy / SciPy (tests/infer_tail_ref.py, oracle/infer_oracle.py).  Every comparison is EQUALITY (integers, or float64 bit
patterns).  Outputs and workspaces are prefilled with 0xAB bytes unless a test says otherwise; outputs sit between guard
words that are checked after every call.  tests/test_cpu_infer_tail.py holds what the inputs claim about themselves."""

import ctypes

import numpy as np
import pytest
import torch

import infer_tail_ref as R
from oracle import infer_oracle as IO
from test_gpu_measure import GUARD, Out, _dev

pytestmark = pytest.mark.gpu

NULL = ctypes.c_void_p(0)
AB32 = 0xABABABAB


def _lib():
    from cellulus_amd import _clx
    return _clx.load()


def _stream(device):
    from cellulus_amd import _clx
    return _clx.stream_ptr(device)


def _ptr(t):
    from cellulus_amd import _clx
    return _clx.ptr(t)


def _zyx(shape):
    return (1,) * (3 - len(shape)) + tuple(shape)


def _bytes(host, device):
    return torch.from_numpy(np.ascontiguousarray(host).reshape(-1).view(np.uint8).copy()).to(device)


def _set(out, host):
    """replace the 0xAB prefill of an Out by the bytes of `host` (the guard zones stay)"""
    host = np.ascontiguousarray(host, dtype=out.dtype)
    assert host.nbytes == out.nbytes
    out.buf[GUARD:GUARD + out.nbytes] = _bytes(host, out.buf.device)


class InOut:
    """a device array that a call reads and writes: the bytes of `host`, `lead` bytes past a 16-byte boundary, between
    two 0xAB guard zones"""

    def __init__(self, host, device, lead=0):
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, self.nbytes = host.shape, host.dtype, host.nbytes
        self.lo = GUARD + lead
        self.buf = torch.full((self.lo + self.nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.lo:self.lo + self.nbytes] = _bytes(host, device)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo)

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[:self.lo] == 0xAB).all() and (host[self.lo + self.nbytes:] == 0xAB).all(), "guard words overwritten"
        return host[self.lo:self.lo + self.nbytes].copy().view(self.dtype).reshape(self.shape)


class Workspace:
    """`nbytes` of 0xAB starting `lead` bytes past a 16-byte boundary, followed by a guard zone"""

    def __init__(self, nbytes, device, lead=0):
        self.nbytes, self.lead = int(nbytes), lead
        self.buf = torch.full((lead + self.nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.lead)

    def check(self):
        edge = self.buf.cpu().numpy()
        assert (edge[:self.lead] == 0xAB).all() and (edge[self.lead + self.nbytes:] == 0xAB).all(), "written outside the workspace"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ======================================================================================================= clx_grow_shrink
_gs_ref_cache = {}


def _gs_ref(shape, grow, shrink, image_name, seg):
    key = (shape, grow, shrink, image_name)
    if key not in _gs_ref_cache:
        _gs_ref_cache[key] = IO.grow_shrink(seg, grow, shrink)
    return _gs_ref_cache[key]


def run_grow_shrink(seg, grow, shrink, device, seg_lead=0, ws_lead=0):
    """clx_grow_shrink in place on a copy of `seg`; the workspace has the size cellulus_amd.segment gives it"""
    Z, Y, X = _zyx(seg.shape)
    image = InOut(seg.astype(np.int32), device, seg_lead)
    ws = Workspace(9 * seg.size + 128, device, ws_lead)
    assert image.ptr.value % 16 == seg_lead and ws.ptr.value % 16 == ws_lead
    status = _lib().clx_grow_shrink(image.ptr, Z, Y, X, grow, shrink, ws.ptr, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    ws.check()
    return image.get()


@pytest.mark.parametrize("name", list(R.GS_CASES))
def test_grow_shrink_equals_scipy_on_the_named_path(name, device):
    """the case id names the dispatch path (checked on the CPU tier): bits4 / bits = gs_bits4_kernel / gs_bits_kernel +
    gs_rows_kernel, tile2 / tile3 = grow_shrink_tile_kernel<2> / <3>, generic = the capped EDT passes"""
    c = R.GS_CASES[name]
    shape, grow, shrink = c["shape"], c["grow"], c["shrink"]
    images = R.gs_images(shape) if c["images"] == "all" else {"full": np.ones(shape, np.int32)}
    cleared = 0
    for image_name, seg in images.items():
        want = _gs_ref(shape, grow, shrink, image_name, seg)
        got = run_grow_shrink(seg, grow, shrink, device, c["seg_lead"], c["ws_lead"])
        assert np.array_equal(got, want), image_name
        cleared += int((want != seg).sum())
    assert cleared > 0 or shrink <= 1                                       # (a distance below 1 holds on background only)


def test_grow_shrink_rejects_bad_arguments(device):
    seg = R.gs_images((33, 65))["blocks"]
    lib, st = _lib(), _stream(device)
    image = InOut(seg, device)
    ws = Workspace(9 * seg.size + 128, device)
    good = dict(seg=image.ptr, Z=1, Y=33, X=65, ws=ws.ptr)
    bad = [dict(seg=NULL), dict(ws=NULL), dict(Z=0), dict(Y=0), dict(X=0), dict(X=-65), dict(Z=16384), dict(Y=16384),
           dict(X=16384), dict(X=20000)]
    for change in bad:
        a = dict(good, **change)
        status = lib.clx_grow_shrink(a["seg"], a["Z"], a["Y"], a["X"], 3, 6, a["ws"], st)
        torch.cuda.synchronize(device)
        assert status != 0, change
        assert lib.clx_last_error().decode().startswith("clx_grow_shrink"), change
        assert np.array_equal(image.get(), seg), change
        assert bool((ws.buf == 0xAB).all().item()), change
    a = good
    assert lib.clx_grow_shrink(a["seg"], a["Z"], a["Y"], a["X"], 3, 6, a["ws"], st) == 0
    torch.cuda.synchronize(device)
    assert np.array_equal(image.get(), IO.grow_shrink(seg, 3, 6))


# ============================================================================================================ clx_edt_sq
def run_edt(mask, cap, device):
    Z, Y, X = _zyx(mask.shape)
    lib = _lib()
    md = _dev(mask.astype(np.uint8), device)
    out = Out(mask.shape, np.int32, device)
    ws = Workspace(lib.clx_edt_workspace(mask.size), device)
    status = lib.clx_edt_sq(_ptr(md), out.ptr, Z, Y, X, cap, ws.ptr, _stream(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    ws.check()
    return out.get()


def check_edt(got, ref, cap, all_ones):
    """exact where ref < cap^2, >= cap^2 elsewhere; cap 0 = unlimited; a mask without any zero gets scipy's phantom
    distances whatever the cap"""
    if cap <= 0 or all_ones:
        assert np.array_equal(got, ref)
        return
    near = ref < cap * cap
    assert np.array_equal(got[near], ref[near])
    assert (got[~near] >= cap * cap).all()


@pytest.mark.parametrize("shape", R.EDT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_equals_scipy_under_every_cap(shape, device):
    for mask_name, mask in R.edt_masks(shape).items():
        ref = IO.edt_sq(mask)
        for cap in R.EDT_CAPS:
            got = run_edt(mask, cap, device)
            try:
                check_edt(got, ref, cap, mask_name == "ones")
            except AssertionError as e:
                raise AssertionError(f"mask {mask_name}, cap {cap}") from e
        if cap > max(shape) and mask_name != "ones":                       # a cap beyond every extent caps nothing
            assert np.array_equal(got, ref), mask_name


def test_edt_sq_past_one_grid(device):
    mask = (np.random.default_rng(8).random(R.EDT_BIG) < 0.5).astype(np.uint8)
    assert np.array_equal(run_edt(mask, 0, device), IO.edt_sq(mask))


# ==================================================================================================== clx_greedy_cluster
GREEDY_IDS = ["f32-2", "f32-3", "f64-2", "f64-3"]


def run_greedy(emb, score, bw, min_object_size, seed_thresh, min_unclustered_sum, device):
    """-> (instance (max(n, 1),) int32, result (2,) int32); instance and result start as 0xAB bytes"""
    nd, n = emb.shape
    is64 = 1 if emb.dtype == np.float64 else 0
    emb_d = _dev(emb if n else np.zeros((nd, 1), emb.dtype), device)
    score_d = _dev(score if n else np.zeros(1, emb.dtype), device)
    ws = Workspace(2 * (n + 16), device)
    instance, result = Out((max(n, 1),), np.int32, device), Out((2,), np.int32, device)
    status = _lib().clx_greedy_cluster(_ptr(emb_d), _ptr(score_d), n, nd, is64, float(bw), int(min_object_size), float(seed_thresh),
                                       int(min_unclustered_sum), ws.ptr, instance.ptr, result.ptr, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    ws.check()
    return instance.get(), result.get()


@pytest.mark.parametrize("dtype,nd", R.GREEDY_TYPES, ids=GREEDY_IDS)
@pytest.mark.parametrize("name", list(R.GREEDY_CASES))
def test_greedy_cluster_equals_the_reference_loop(name, dtype, nd, device):
    c = R.GREEDY_CASES[name]
    emb, score = R.greedy_inputs(name, dtype, nd)
    want, n_objects, n_iterations, log = R.greedy_ref(name, dtype, nd)
    n = emb.shape[1]
    instance, result = run_greedy(emb, score, c["bw"], c["min_object_size"], c["seed_thresh"], c["min_unclustered_sum"], device)
    assert result.tolist() == [n_objects, n_iterations]
    assert np.array_equal(instance[:n], want)
    if n == 0:
        assert instance.view(np.uint32)[0] == AB32                          # nothing to write: the prefill stays


def test_greedy_cluster_rejects_bad_arguments(device):
    emb, score = R.greedy_inputs("n65", np.float32, 2)
    n = emb.shape[1]
    lib, st = _lib(), _stream(device)
    emb_d, score_d = _dev(emb, device), _dev(score, device)
    ws = Workspace(2 * (n + 16), device)
    instance, result = Out((n,), np.int32, device), Out((2,), np.int32, device)
    good = dict(emb=_ptr(emb_d), score=_ptr(score_d), n=n, nd=2, bw=R.GREEDY_BW, ws=ws.ptr, instance=instance.ptr, result=result.ptr)
    bad = [dict(emb=NULL), dict(score=NULL), dict(ws=NULL), dict(instance=NULL), dict(result=NULL), dict(n=-1), dict(nd=4),
           dict(nd=1), dict(bw=0.0), dict(bw=-1.0)]

    def call(a):
        return lib.clx_greedy_cluster(a["emb"], a["score"], a["n"], a["nd"], 0, a["bw"], 3, 0.2, 0, a["ws"], a["instance"],
                                      a["result"], st)

    for change in bad:
        status = call(dict(good, **change))
        torch.cuda.synchronize(device)
        assert status != 0, change
        assert lib.clx_last_error().decode().startswith("clx_greedy_cluster"), change
        assert instance.untouched() and result.untouched() and bool((ws.buf == 0xAB).all().item()), change
    assert call(good) == 0
    torch.cuda.synchronize(device)
    want, n_objects, n_iterations, _ = R.greedy_ref("n65", np.float32, 2)
    assert np.array_equal(instance.get(), want) and result.get().tolist() == [n_objects, n_iterations]


# ======================================================================== clx_label_presence / clx_joint_histogram
def run_presence(lab, nid, present_in, device):
    """-> (present, bad); `present` starts as present_in, `bad` as 0 (the kernel only ever sets them)"""
    lab_d = _dev(lab, device)
    assert lab_d.data_ptr() % 16 == 0
    present, bad = Out((nid,), np.int32, device), Out((1,), np.int32, device)
    _set(present, present_in)
    _set(bad, np.zeros(1, np.int32))
    status = _lib().clx_label_presence(_ptr(lab_d), lab.size, nid, present.ptr, bad.ptr, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return present.get(), int(bad.get()[0])


def run_joint(pred, gt, prow, gcol, ncol, joint_in, device):
    """-> the table, which starts as joint_in"""
    pred_d, gt_d, prow_d, gcol_d = (_dev(a, device) for a in (pred, gt, prow, gcol))
    joint = Out(joint_in.shape, np.uint64, device)
    _set(joint, joint_in)
    status = _lib().clx_joint_histogram(_ptr(pred_d), _ptr(gt_d), pred.size, _ptr(prow_d), _ptr(gcol_d), ncol, joint.ptr,
                                        _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return joint.get()


@pytest.mark.parametrize("n", R.EVAL_SMALL)
def test_label_presence_and_joint_histogram_small_maps(n, device):
    prefill = R.presence_prefill()
    for name, (pred, gt) in R.label_maps(n, n).items():
        for lab in (pred, gt):
            want, _ = R.ref_presence(lab, R.NID, prefill)
            got, bad = run_presence(lab, R.NID, prefill, device)
            assert bad == 0 and np.array_equal(got, want), name
        for nrow, ncol in ((37, 11), (5, 1)):
            prow, gcol = R.row_col_maps(nrow, ncol)
            table = R.joint_prefill(nrow, ncol)
            got = run_joint(pred, gt, prow, gcol, ncol, table, device)
            assert np.array_equal(got, R.ref_joint(pred, gt, prow, gcol, ncol, table)), (name, nrow, ncol)


def test_label_presence_past_one_grid(device):
    n = R.PRESENCE_BIG
    lab = R.label_maps(n, 21)["blocky"][0].copy()
    lab[4 * R.EVAL_GRID_THREADS + 100:4 * R.EVAL_GRID_THREADS + 104] = 12346    # ids that occur on the second trip only ...
    lab[n - 1] = 54321                                                      # ... and in the 3-pixel tail only
    assert not np.isin([12346, 54321], R.sparse_ids(21)).any()
    prefill = R.presence_prefill()
    want, _ = R.ref_presence(lab, R.NID, prefill)
    assert want[12346] == 1 and want[54321] == 1 and prefill[12346] == 0 and prefill[54321] == 0
    got, bad = run_presence(lab, R.NID, prefill, device)
    assert bad == 0 and np.array_equal(got, want)
    # a bad id in the tail; on the second trip as the first pixel of a 16-byte group, and as the third
    for where, poison in ((n - 2, R.NID), (4 * R.EVAL_GRID_THREADS + 48, -1), (4 * R.EVAL_GRID_THREADS + 50, -1)):
        poisoned = lab.copy()
        poisoned[where] = poison
        want, ref_bad = R.ref_presence(poisoned, R.NID, prefill)
        got, bad = run_presence(poisoned, R.NID, prefill, device)
        assert ref_bad == 1 and bad == 1 and np.array_equal(got, want), where


def test_joint_histogram_past_one_grid(device):
    n = R.JOINT_BIG
    pred, gt = R.label_maps(n, 22)["blocky"]
    for nrow, ncol in ((37, 11),):
        prow, gcol = R.row_col_maps(nrow, ncol)
        table = R.joint_prefill(nrow, ncol)
        want = R.ref_joint(pred, gt, prow, gcol, ncol, table)
        assert int((want - table).sum()) == n
        got = run_joint(pred, gt, prow, gcol, ncol, table, device)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("nid", [R.NID, 100])
def test_label_presence_ids_outside_the_table_set_bad_and_nothing_else(nid, device):
    prefill = R.presence_prefill(nid)
    for n in (3, 17):                                                       # the 1-3 pixel tail alone; vector body + tail
        base = (np.arange(n) % 7).astype(np.int32) * 9
        want, bad = R.ref_presence(base, nid, prefill)
        got, got_bad = run_presence(base, nid, prefill, device)
        assert bad == 0 and got_bad == 0 and np.array_equal(got, want)
        for poison in (-1, R.INT_MIN, nid, R.INT_MAX):
            for where in range(n):
                lab = base.copy()
                lab[where] = poison
                want, bad = R.ref_presence(lab, nid, prefill)
                got, got_bad = run_presence(lab, nid, prefill, device)
                assert bad == 1 and got_bad == 1 and np.array_equal(got, want), (poison, where)


def test_presence_and_joint_reject_bad_arguments(device):
    lib, st = _lib(), _stream(device)
    pred, gt = R.label_maps(17, 5)["blocky"]
    pred_d, gt_d = _dev(pred, device), _dev(gt, device)
    off_d = _dev(pred, device, offset=1)                                    # 4 bytes past a 16-byte boundary
    assert off_d.data_ptr() % 16 == 4
    present, bad = Out((R.NID,), np.int32, device), Out((1,), np.int32, device)
    for lab, n, nid, p, b in ((off_d, 17, R.NID, present.ptr, bad.ptr), (pred_d, 0, R.NID, present.ptr, bad.ptr),
                              (pred_d, -17, R.NID, present.ptr, bad.ptr), (pred_d, 17, 0, present.ptr, bad.ptr),
                              (None, 17, R.NID, present.ptr, bad.ptr), (pred_d, 17, R.NID, NULL, bad.ptr),
                              (pred_d, 17, R.NID, present.ptr, NULL)):
        status = lib.clx_label_presence(_ptr(lab) if lab is not None else NULL, n, nid, p, b, st)
        torch.cuda.synchronize(device)
        assert status != 0 and lib.clx_last_error().decode().startswith("clx_label_presence")
        assert present.untouched() and bad.untouched()
    prow, gcol = R.row_col_maps(5, 3)
    prow_d, gcol_d = _dev(prow, device), _dev(gcol, device)
    joint = Out((5, 3), np.uint64, device)
    good = dict(pred=_ptr(pred_d), gt=_ptr(gt_d), n=17, prow=_ptr(prow_d), gcol=_ptr(gcol_d), ncol=3, joint=joint.ptr)
    bad_args = [dict(pred=_ptr(off_d)), dict(gt=_ptr(off_d)), dict(n=0), dict(n=-1), dict(ncol=0), dict(ncol=-3), dict(pred=NULL),
                dict(gt=NULL), dict(prow=NULL), dict(gcol=NULL), dict(joint=NULL)]
    for change in bad_args:
        a = dict(good, **change)
        status = lib.clx_joint_histogram(a["pred"], a["gt"], a["n"], a["prow"], a["gcol"], a["ncol"], a["joint"], st)
        torch.cuda.synchronize(device)
        assert status != 0 and lib.clx_last_error().decode().startswith("clx_joint_histogram"), change
        assert joint.untouched(), change


def test_joint_histogram_on_device_takes_a_contiguous_slice_at_an_odd_offset(device):
    from cellulus_amd.evaluate import joint_histogram_on_device

    pred, gt = R.label_maps(37 * 53 + 1, 6)["blocky"]
    a, b = torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device)
    for lead in (1, 2, 3):
        pa, pb = a.reshape(-1)[lead:], b.reshape(-1)[lead:]
        assert pa.is_contiguous() and pa.data_ptr() % 16 == 4 * lead
        got = joint_histogram_on_device(pa, pb)
        want = R.ref_joint_histogram(pred[lead:], gt[lead:])
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), lead
    got = joint_histogram_on_device(a.reshape(-1)[1:], b[:-1])             # one operand aligned, one not
    want = R.ref_joint_histogram(pred[1:], gt[:-1])
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ====================================================== clx_offset_magnitude / clx_gaussian_filter_f64 / clx_negate_f64
def run_gaussian(img, w, device):
    Z, Y, X = _zyx(img.shape)
    img_d, w_d = _dev(img, device), _dev(w, device)
    out, tmp = Out(img.shape, np.float64, device), Out(img.shape, np.float64, device)
    status = _lib().clx_gaussian_filter_f64(_ptr(img_d), out.ptr, tmp.ptr, Z, Y, X, _ptr(w_d), len(w) - 1, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    tmp.get()                                                               # (guard words of the scratch image)
    return out.get()


@pytest.mark.parametrize("kind", ["gaussian", "random"])
@pytest.mark.parametrize("radius", R.GAUSS_RADII)
def test_gaussian_filter_equals_scipy_correlate1d(radius, kind, device):
    """extents 1, 2, 3, 5 and 17 on every axis: with radius 8 and 20 the reflection runs through several periods"""
    rng = np.random.default_rng(radius)
    w = R.gauss_weights(radius, kind)
    for shape in R.gauss_shapes():
        img = rng.random(shape) * 10.0 + 0.5
        want = R.ref_gaussian(img, w)
        got = run_gaussian(img, w, device)
        assert np.array_equal(_bits(got), _bits(want)), shape


def test_gaussian_filter_rejects_aliased_buffers_and_bad_arguments(device):
    lib, st = _lib(), _stream(device)
    img = np.random.default_rng(0).random((5, 17))
    w = R.gauss_weights(8, "gaussian")
    img_d, w_d = _dev(img, device), _dev(w, device)
    out, tmp = Out(img.shape, np.float64, device), Out(img.shape, np.float64, device)
    good = dict(img=_ptr(img_d), out=out.ptr, tmp=tmp.ptr, Z=1, Y=5, X=17, w=_ptr(w_d), radius=8)
    bad = [dict(out=_ptr(img_d)), dict(tmp=_ptr(img_d)), dict(tmp=out.ptr), dict(out=tmp.ptr), dict(img=NULL), dict(out=NULL),
           dict(tmp=NULL), dict(w=NULL), dict(Z=0), dict(Y=0), dict(X=-17), dict(radius=-1)]
    for change in bad:
        a = dict(good, **change)
        status = lib.clx_gaussian_filter_f64(a["img"], a["out"], a["tmp"], a["Z"], a["Y"], a["X"], a["w"], a["radius"], st)
        torch.cuda.synchronize(device)
        assert status != 0 and lib.clx_last_error().decode().startswith("clx_gaussian_filter_f64"), change
        assert out.untouched() and tmp.untouched(), change
        assert np.array_equal(img_d.cpu().numpy().reshape(img.shape), img), change


def run_magnitude(emb, device):
    nd, n = emb.shape
    emb_d = _dev(emb, device)
    out = Out((n,), np.float64, device)
    status = _lib().clx_offset_magnitude(_ptr(emb_d), out.ptr, nd, n, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return out.get()


def run_negate(v, device):
    v_d = _dev(v, device)
    out = Out(v.shape, np.float64, device)
    status = _lib().clx_negate_f64(_ptr(v_d), out.ptr, v.size, _stream(device))
    assert status == 0, _lib().clx_last_error()
    torch.cuda.synchronize(device)
    return out.get()


@pytest.mark.parametrize("nd", [1, 2, 3, 4])
def test_offset_magnitude_equals_the_sequential_sum(nd, device):
    """zeros of both signs, denormals, values whose squares overflow (inf, like NumPy), negatives and NaN"""
    for n in (1, 7, 300):
        emb = R.magnitude_values(nd, n, 10 * nd + n)
        assert np.array_equal(_bits(run_magnitude(emb, device)), _bits(R.ref_magnitude(emb))), n


def test_negate_flips_the_sign_bit_only(device):
    for n in (1, 5, 100):
        v = R.negate_values(n, n)
        assert np.array_equal(_bits(run_negate(v, device)), _bits(v) ^ np.uint64(1 << 63)), n
        assert np.array_equal(_bits(-v), _bits(v) ^ np.uint64(1 << 63))


def test_magnitude_and_negate_past_one_grid(device):
    n = R.SEEDS_BIG
    emb = R.magnitude_values(2, n, 3)
    emb[0, -3:] = [np.nan, 1e200, -0.0]                                     # on the second trip
    assert np.array_equal(_bits(run_magnitude(emb, device)), _bits(R.ref_magnitude(emb)))
    v = R.negate_values(n, 4)
    v[-4:] = [np.nan, -np.inf, 0.0, -0.0]
    assert np.array_equal(_bits(run_negate(v, device)), _bits(v) ^ np.uint64(1 << 63))


def test_magnitude_and_negate_reject_bad_arguments(device):
    lib, st = _lib(), _stream(device)
    emb = R.magnitude_values(2, 9, 1)
    emb_d = _dev(emb, device)
    out = Out((9,), np.float64, device)
    for args in ((NULL, out.ptr, 2, 9), (_ptr(emb_d), NULL, 2, 9), (_ptr(emb_d), out.ptr, 0, 9), (_ptr(emb_d), out.ptr, 2, 0),
                 (_ptr(emb_d), out.ptr, 2, -9)):
        assert lib.clx_offset_magnitude(*args, st) != 0
        torch.cuda.synchronize(device)
        assert lib.clx_last_error().decode().startswith("clx_offset_magnitude") and out.untouched()
    for args in ((NULL, out.ptr, 9), (_ptr(emb_d), NULL, 9), (_ptr(emb_d), out.ptr, 0), (_ptr(emb_d), out.ptr, -1)):
        assert lib.clx_negate_f64(*args, st) != 0
        torch.cuda.synchronize(device)
        assert lib.clx_last_error().decode().startswith("clx_negate_f64") and out.untouched()


# =================================================================================================== clx_cc_label_filter
def run_cc(seg, min_size, device):
    """clx_cc_label_filter with a 16-byte-aligned `out`: the label-list pipeline in 2-D, the run pipeline in 3-D"""
    lib = _lib()
    Z, Y, X = _zyx(seg.shape)
    lab = _dev(seg.astype(np.int32), device)
    out, ncomp = Out(seg.shape, np.int32, device), Out((1,), np.int32, device)
    assert out.ptr.value % 16 == 0
    ws = Workspace(lib.clx_cc_workspace(seg.size), device)
    status = lib.clx_cc_label_filter(_ptr(lab), out.ptr, Z, Y, X, min_size, ncomp.ptr, ws.ptr, _stream(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    ws.check()
    return out.get(), int(ncomp.get()[0])


@pytest.fixture(scope="module")
def cc_big():
    return R.cc_big_volume()


@pytest.mark.parametrize("min_size", [1, 50])
def test_cc_run_pipeline_past_one_grid(min_size, cc_big, device):
    want = IO.size_filter(cc_big, min_size)
    got, n = run_cc(cc_big, min_size, device)
    assert np.array_equal(got, want)
    assert n == want.max() and n > 1


@pytest.mark.parametrize("nd", [2, 3])
def test_cc_size_threshold_is_inclusive(nd, device):
    seg = R.cc_boxes(nd)
    sizes = dict(zip((1, 2, 3, 4), R.BOX_SIZES))
    for min_size, kept in ((9, (3, 4)), (10, (4,)), (0, (1, 2, 3, 4)), (-3, (1, 2, 3, 4)), (1, (1, 2, 3, 4)), (30, (4,)), (31, ())):
        want = IO.size_filter(seg, max(min_size, 1))
        got, n = run_cc(seg, min_size, device)
        assert np.array_equal(got, want), min_size
        assert n == len(kept) and np.array_equal(got != 0, np.isin(seg, kept)), min_size
        assert all(sizes[i] >= min_size for i in kept)


@pytest.mark.parametrize("nd", [2, 3])
def test_cc_extreme_label_values_are_foreground_and_distinct(nd, device):
    seg = R.cc_extreme_labels(nd)
    for min_size in (1, 3):
        want = IO.size_filter(seg, min_size)
        got, n = run_cc(seg, min_size, device)
        assert np.array_equal(got, want) and n == want.max(), min_size
    got, n = run_cc(seg, 1, device)
    assert n == 6 and np.array_equal(got != 0, seg != 0)
