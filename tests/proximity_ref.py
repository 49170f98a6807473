"""numpy float32 restatement of rt_nearest_spheres / rt_nearest_spheres_ranged over a prepared scene's L (oracle_lib.OracleScene(...).arrays()
or Prepared.bvh_arrays()).

For a point p and sphere j of L (centre c, radius r) the gap is, in exactly this float32 arithmetic,
    dx = p.x - c.x; dy = p.y - c.y; dz = p.z - c.z;   gap = sqrt((dx*dx + dy*dy) + dz*dz) - r
Sphere j is selected iff gap <= max_dist; the selected spheres are ordered by (gap, j).  Per point: count = the number selected, then the
first min(count, k) as index j and gap; slots past it are -1 and 0.0.  A point with a non-finite component, or (per-point bounds) a bound
outside [0, 1e9], selects nothing.  This is brute force over all spheres: no tree is involved.

nearest() forms the full (points x spheres) gap matrix in chunks of points.  nearest_near() is for the 10^6-sphere floor: per point it
computes the same gaps over the spheres whose centre lies within max_dist + r_max + a wide margin of the point along x and z (a selected
sphere is within gap + r of the point in every coordinate, up to rounding far below the margin), so it needs a bounded max_dist.  The CPU
suite holds the two equal on small scenes.
"""
import numpy as np

F = np.float32
KMAX = 32
TMAX = F(1e9)


def gaps(L, p):
    """[m, n] float32 gaps of the points p [m, 3] to the spheres L [n, >= 7]"""
    L = np.asarray(L, dtype=F)
    p = np.asarray(p, dtype=F)
    with np.errstate(all="ignore"):
        dx = p[:, None, 0] - L[None, :, 0]
        dy = p[:, None, 1] - L[None, :, 1]
        dz = p[:, None, 2] - L[None, :, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz) - L[None, :, 6]


def max_dist_ok(m):
    m = np.asarray(m, dtype=F)
    with np.errstate(invalid="ignore"):
        return (m >= 0) & (m <= TMAX)


def point_ok(p):
    return np.isfinite(np.asarray(p, dtype=F)).all(axis=1)


def _bounds(m, max_dist):
    if np.ndim(max_dist) == 0:
        return np.full(m, F(max_dist), F)
    md = np.asarray(max_dist, dtype=F)
    assert md.shape == (m,)
    return md


def _select(g, j, md, k):
    """count, index, gap of one chunk: g [m, c] gaps of the candidate spheres j [c] (or [m, c]); md [m] bounds"""
    m = g.shape[0]
    jj = np.broadcast_to(j, g.shape)
    with np.errstate(invalid="ignore"):
        sel = g <= md[:, None]
    count = sel.sum(axis=1).astype(np.int32)
    key = np.where(sel, g, F(np.inf))
    order = np.lexsort((jj, key), axis=1)[:, :k]
    rows = np.arange(m)[:, None]
    have = sel[rows, order]
    index = np.full((m, k), -1, np.int32)
    gap = np.zeros((m, k), F)
    kk = order.shape[1]
    index[:, :kk] = np.where(have, jj[rows, order], -1)
    gap[:, :kk] = np.where(have, g[rows, order], F(0))
    return count, index, gap


def nearest(L, points, max_dist, k, chunk=256):
    """(count [m] int32, index [m, k] int32, gap [m, k] float32); max_dist a scalar or an [m] array (per-point bounds)"""
    L = np.asarray(L, dtype=F)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    m, n = p.shape[0], L.shape[0]
    md = _bounds(m, max_dist)
    ok = point_ok(p) & max_dist_ok(md)
    count = np.zeros(m, np.int32)
    index = np.full((m, k), -1, np.int32)
    gap = np.zeros((m, k), F)
    j = np.arange(n)
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        c, i, g = _select(gaps(L, p[s:e]), j, np.where(ok[s:e], md[s:e], F(-1)), k)
        count[s:e], index[s:e], gap[s:e] = c, i, g
    count[~ok] = 0
    index[~ok] = -1
    gap[~ok] = 0
    return count, index, gap


def nearest_near(L, points, max_dist, k):
    """nearest() restricted, point by point, to the spheres near it along x and z (see the module docstring); every bound must be finite."""
    L = np.asarray(L, dtype=F)
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    m = p.shape[0]
    md = _bounds(m, max_dist)
    ok = point_ok(p) & max_dist_ok(md)
    by_x = np.argsort(L[:, 0].astype(np.float64), kind="stable")
    xs = L[by_x, 0].astype(np.float64)
    r_max = float(np.max(L[:, 6]))
    c_max = float(np.max(np.abs(L[:, :3])))
    count = np.zeros(m, np.int32)
    index = np.full((m, k), -1, np.int32)
    gap = np.zeros((m, k), F)
    for i in np.nonzero(ok)[0]:
        reach = float(md[i]) + r_max
        reach += 2.0 ** -10 * (reach + c_max + float(np.max(np.abs(p[i])))) + 1e-30
        a = int(np.searchsorted(xs, float(p[i, 0]) - reach, side="left"))
        b = int(np.searchsorted(xs, float(p[i, 0]) + reach, side="right"))
        cand = by_x[a:b]
        cand = cand[np.abs(L[cand, 2].astype(np.float64) - float(p[i, 2])) <= reach]
        cand = np.sort(cand)
        if cand.size == 0:
            continue
        c, ix, g = _select(gaps(L[cand], p[i:i + 1]), cand, md[i:i + 1], k)
        count[i], index[i], gap[i] = c[0], ix[0], g[0]
    return count, index, gap
