"""Plain float64 NumPy restatements of the operations in csrc/meanshift.hip — the reference side of
test_cpu_meanshift.py and test_gpu_meanshift.py.  Nothing here imports the product.

Every elementwise step is one IEEE operation per element (NumPy never fuses a multiply with an add), in the order
the kernels and sklearn's _mean_shift_single_seed take them; only the ORDER in which the members of a seed are summed
is a free parameter (`order`), and on lattice data it cannot matter."""

import numpy as np


def ref_prepare(emb, std, thr):
    """emb (ND, *spatial), std (*spatial), any float type -> (points (nfg, ND) f64, raster index (nfg,) i32,
    emb_after (ND, *spatial) f64).  Foreground: float64(std) < thr, strict (NaN is background); component 0 += x (last
    axis), 1 += y, 2 += z — over EVERY pixel, which is what the float64 entry writes back."""
    emb = np.asarray(emb)
    nd, spatial = emb.shape[0], emb.shape[1:]
    assert len(spatial) == nd
    after = emb.astype(np.float64)
    for c in range(nd):
        ax = nd - 1 - c
        shape = [1] * nd
        shape[ax] = spatial[ax]
        after[c] = after[c] + np.arange(spatial[ax], dtype=np.float64).reshape(shape)
    with np.errstate(invalid="ignore"):
        fg = np.asarray(std).astype(np.float64).reshape(-1) < np.float64(thr)
    index = np.flatnonzero(fg).astype(np.int32)
    points = np.ascontiguousarray(after.reshape(nd, -1)[:, index].T)
    return points, index, after


def _member_sum(x, order):
    if len(x) == 0:
        return np.float64(0.0)
    if order == "forward":
        return np.cumsum(x)[-1]                  # cumsum is the sequential left-to-right sum
    if order == "backward":
        return np.cumsum(x[::-1])[-1]
    assert order == "pairwise"
    return np.sum(x)


def _iterate(fit, seeds, bw, max_iter, order, want_margin):
    fit = np.ascontiguousarray(fit, dtype=np.float64)
    seeds = np.ascontiguousarray(seeds, dtype=np.float64)
    ns, nd = seeds.shape
    fit = fit.reshape(-1, nd)
    bw = np.float64(bw)
    bw2 = bw * bw
    stop = np.float64(1e-3) * bw
    centres = np.empty((ns, nd), np.float64)
    counts = np.empty(ns, np.int32)
    iters = np.empty(ns, np.int32)
    m_member = np.full(ns, np.inf)
    m_stop = np.full(ns, np.inf)
    for s in range(ns):
        with np.errstate(over="ignore", invalid="ignore"):          # (seeds at 1e300: d2 is inf, and inf <= bw2 is false)
            mean = seeds[s].copy()
            completed = members = 0
            while True:
                d2 = np.zeros(len(fit))
                for c in range(nd):
                    df = fit[:, c] - mean[c]
                    d2 = d2 + df * df
                inside = d2 <= bw2
                if want_margin and len(fit):
                    m_member[s] = min(m_member[s], np.abs(d2 - bw2).min())
                members = int(inside.sum())
                if members == 0:
                    break
                shift2 = np.float64(0.0)
                for c in range(nd):
                    nm = _member_sum(fit[inside, c], order) / np.float64(members)
                    df = nm - mean[c]
                    shift2 = shift2 + df * df
                    mean[c] = nm
                shift = np.sqrt(shift2)
                if want_margin:
                    m_stop[s] = min(m_stop[s], abs(shift - stop))
                if shift <= stop or completed == max_iter:
                    break
                completed += 1
            centres[s] = mean
            counts[s] = members
            iters[s] = completed
    return centres, counts, iters, m_member, m_stop


def ref_iterate(fit, seeds, bw, max_iter, order="forward"):
    """The loop of sklearn's _mean_shift_single_seed per seed -> (centres (ns, ND), counts, iters): members are the
    fit points with d2 <= bw*bw (d2 accumulated over the components in order), the new mean is sum / count per
    component, the loop stops when no point is a member, when sqrt(shift2) <= 1e-3*bw, or when `max_iter` iterations
    were completed.  counts = members of the last query, iters = completed iterations."""
    return _iterate(fit, seeds, bw, max_iter, order, False)[:3]


def ref_margin(fit, seeds, bw, max_iter, order="forward"):
    """Per seed: (the smallest |d2 - bw^2| over all points and iterations, the smallest |sqrt(shift2) - 1e-3 bw| over
    all iterations) — how far every decision of ref_iterate was from flipping (inf where none was taken)."""
    return _iterate(fit, seeds, bw, max_iter, order, True)[3:]


def ref_bucket(points, origin, cell, dims):
    """Counting sort by uniform-grid cell: cell coordinate floor((x - origin) / cell) — a division — clamped into
    `dims` = (nx, ny, nz), cell id x fastest.  -> (points in stable cell order, cell_start (ncells + 1) i32)."""
    points = np.asarray(points, dtype=np.float64)
    n, nd = points.shape
    cid = np.zeros(n, np.int64)
    stride = 1
    for c in range(nd):
        k = np.floor((points[:, c] - np.float64(origin[c])) / np.float64(cell))
        cid += stride * np.clip(k, 0, dims[c] - 1).astype(np.int64)
        stride *= dims[c]
    ncells = int(np.prod(dims))
    order = np.argsort(cid, kind="stable")
    start = np.zeros(ncells + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(cid, minlength=ncells))
    return points[order], start


def ref_assign(points, centres):
    """1 + the first minimum of d2 over the centres (the smallest id among equals)."""
    points = np.asarray(points, dtype=np.float64)
    centres = np.asarray(centres, dtype=np.float64)
    n, nd = points.shape
    best = np.full(n, np.inf)
    arg = np.zeros(n, np.int32)
    for k0 in range(0, len(centres), 256):
        blk = centres[k0:k0 + 256]
        d2 = np.zeros((n, len(blk)))
        for c in range(nd):
            df = points[:, c:c + 1] - blk[None, :, c]
            d2 = d2 + df * df
        a = d2.argmin(axis=1)                     # first minimum of the block
        v = d2[np.arange(n), a]
        take = v < best                           # strict: an earlier block's equal distance stays
        arg[take] = (k0 + a[take]).astype(np.int32)
        best[take] = v[take]
    return arg + 1
