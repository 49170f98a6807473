"""numpy float32 restatement of the range queries (rt_spheres_within_count / _fill, rt_contact_pairs_count / _fill) over a prepared scene's L
(oracle_lib.OracleScene(...).arrays() or Prepared.bvh_arrays()), built on proximity_ref's gaps / point_ok / max_dist_ok.

Sphere j is selected for point i iff gaps(L, p)[i, j] <= the point's bound and j >= first[i] (first absent: 0).  The answer is CSR:
offsets [m + 1] int64 (offsets[0] = 0, row i at [offsets[i], offsets[i + 1])), index [total] int32 in ASCENDING j within a row, gap [total]
float32.  A point with a non-finite component, or a bound outside [0, 1e9], has an empty row.  Brute force over all spheres: no tree.

Contact pairs are the self-query: point i is the centre of L[i], its bound float32(radius_i) + float32(margin) (one float32 addition),
first = i + 1: pair (i, j), i < j, iff gaps(L, c_i)[j] <= that bound -- evaluated from the lower index only.

within() forms the (points x spheres) gap matrix in chunks.  within_near() is for the 10^6-sphere floor and the larger random scenes, modelled on
proximity_ref.nearest_near: it evaluates the same gaps only over the spheres near the point along x and z (a selected sphere is within
gap + r of the point in every coordinate, up to rounding far below the margin), found through a uniform x/z grid whose cell is the largest
reach, so it needs bounded bounds.  The CPU suite holds the two forms equal.
"""
import numpy as np

import proximity_ref as P

F = np.float32


def _inputs(L, points, max_dist, first):
    L = np.asarray(L, dtype=F)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    m = p.shape[0]
    md = P._bounds(m, max_dist)
    ok = P.point_ok(p) & P.max_dist_ok(md)
    if first is None:
        fi = np.zeros(m, np.int64)
    else:
        fi = np.asarray(first).astype(np.int64)
        assert fi.shape == (m,)
    return L, p, m, md, ok, fi


def _csr(m, rows, cols, g):
    """rows ascending, cols ascending within a row"""
    offsets = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=offsets[1:])
    return offsets, cols.astype(np.int32), g.astype(F)


def within(L, points, max_dist, first=None, chunk=None):
    """(offsets [m + 1] int64, index [total] int32, gap [total] float32); max_dist a scalar or an [m] array; first None or an [m] integer array"""
    L, p, m, md, ok, fi = _inputs(L, points, max_dist, first)
    n = L.shape[0]
    if chunk is None:
        chunk = max(1, min(256, (1 << 22) // n))
    j = np.arange(n, dtype=np.int64)
    rows, cols, gs = [], [], []
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        g = P.gaps(L, p[s:e])
        with np.errstate(invalid="ignore"):
            sel = (g <= md[s:e, None]) & (j[None, :] >= fi[s:e, None]) & ok[s:e, None]
        r, c = np.nonzero(sel)
        rows.append(r + s)
        cols.append(c)
        gs.append(g[r, c])
    if not rows:
        return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, F)
    return _csr(m, np.concatenate(rows), np.concatenate(cols), np.concatenate(gs))


def _pair_gaps(L, p, pi, sj):
    """proximity_ref.gaps's expression, element by element: the gaps of the points p[pi] to the spheres L[sj] (the CPU suite holds within_near,
    which goes through here, equal to within, which goes through gaps)"""
    with np.errstate(all="ignore"):
        dx = p[pi, 0] - L[sj, 0]
        dy = p[pi, 1] - L[sj, 1]
        dz = p[pi, 2] - L[sj, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz) - L[sj, 6]


def within_near(L, points, max_dist, first=None, chunk=1 << 15):
    """within() restricted, point by point, to the spheres near it along x and z (see the module docstring); every valid bound must be modest"""
    L, p, m, md, ok, fi = _inputs(L, points, max_dist, first)
    r_max = float(np.max(L[:, 6]))
    c_max = float(np.max(np.abs(L[:, :3])))
    pm = np.where(ok, np.max(np.abs(np.where(np.isfinite(p), p, 0)).astype(np.float64), axis=1), 0.0)
    reach = np.where(ok, md.astype(np.float64), 0.0) + r_max
    reach = reach + 2.0 ** -10 * (reach + c_max + pm) + 1e-30
    cell = float(reach.max()) if m else 1.0
    x0, z0 = float(L[:, 0].min()), float(L[:, 2].min())
    cx = np.floor((L[:, 0].astype(np.float64) - x0) / cell).astype(np.int64)
    cz = np.floor((L[:, 2].astype(np.float64) - z0) / cell).astype(np.int64)
    ncx, ncz = int(cx.max()) + 1, int(cz.max()) + 1
    key = cx * ncz + cz
    by_cell = np.argsort(key, kind="stable")
    keys = key[by_cell]
    rows, cols, gs = [], [], []
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        who = np.nonzero(ok[s:e])[0] + s
        if who.size == 0:
            continue
        # (a sphere within `reach` <= cell of the point along an axis lies in the point's cell or a neighbour; points far outside clip to
        # a cell beyond the grid, whose neighbours are empty or the grid's edge)
        pcx = np.clip(np.floor((p[who, 0].astype(np.float64) - x0) / cell), -2, ncx + 1).astype(np.int64)
        pcz = np.clip(np.floor((p[who, 2].astype(np.float64) - z0) / cell), -2, ncz + 1).astype(np.int64)
        pi_all, sj_all = [], []
        for ax in (-1, 0, 1):
            for az in (-1, 0, 1):
                qx, qz = pcx + ax, pcz + az
                inside = (qx >= 0) & (qx < ncx) & (qz >= 0) & (qz < ncz)
                k = np.where(inside, qx * ncz + qz, -1)
                a = np.searchsorted(keys, k, side="left")
                b = np.where(inside, np.searchsorted(keys, k, side="right"), a)
                ln = b - a
                tot = int(ln.sum())
                if tot == 0:
                    continue
                rep = np.repeat(np.arange(who.size), ln)
                pos = a[rep] + (np.arange(tot) - np.repeat(np.cumsum(ln) - ln, ln))
                pi_all.append(who[rep])
                sj_all.append(by_cell[pos])
        if not pi_all:
            continue
        pi, sj = np.concatenate(pi_all), np.concatenate(sj_all)
        g = _pair_gaps(L, p, pi, sj)
        with np.errstate(invalid="ignore"):
            sel = (g <= md[pi]) & (sj >= fi[pi])
        pi, sj, g = pi[sel], sj[sel], g[sel]
        o = np.lexsort((sj, pi))
        rows.append(pi[o])
        cols.append(sj[o])
        gs.append(g[o])
    if not rows:
        return np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, F)
    return _csr(m, np.concatenate(rows), np.concatenate(cols), np.concatenate(gs))


def contact_bounds(L, margin):
    """the self-query's per-sphere bound: float32(radius) + float32(margin), one float32 addition"""
    with np.errstate(all="ignore"):
        return np.asarray(L, dtype=F)[:, 6] + F(margin)


def contact_pairs(L, margin, near=False):
    """(pairs [total, 2] int32 in ascending (i, j), i < j; gap [total] float32: centre i to the surface of j).  near: through within_near"""
    L = np.asarray(L, dtype=F)
    n = L.shape[0]
    fn = within_near if near else within
    off, idx, gap = fn(L, L[:, :3], contact_bounds(L, margin), first=np.arange(1, n + 1))
    i = np.repeat(np.arange(n, dtype=np.int32), np.diff(off))
    return np.stack([i, idx], axis=1).astype(np.int32).reshape(-1, 2), gap


def sort_rows_by_gap(offsets, index, gap):
    """the rows re-ordered by (gap, j): proximity_ref.nearest's order"""
    rows = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    o = np.lexsort((index, gap, rows))
    return index[o], gap[o]
