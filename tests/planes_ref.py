"""numpy float32 restatement of the plane-set queries (rt_spheres_in_planes_count / _fill) over a prepared scene's L (oracle_lib.OracleScene(...)
.arrays() or Prepared.bvh_arrays()), built on proximity_ref's helpers with within_ref's CSR assembly, the way boxes_ref is.

A query is K planes {a, b, c, d}, inside a x + b y + c z + d >= 0.  Each is normalised once, and for sphere j of L (centre c, radius r) the gap
is, in exactly this float32 arithmetic,
    len = sqrt((a*a + b*b) + c*c);   nx = a/len; ny = b/len; nz = c/len; w = d/len
    depth_k = ((nx*c.x + ny*c.y) + nz*c.z) + w
    gap = fmax(fmax(... fmax(0, -depth_0) ..., -depth_{K-2}), -depth_{K-1}) - r          (planes in the caller's order)
Sphere j is selected for query i iff gap <= the query's margin and j >= first[i] (first absent: 0).  The answer is within_ref's CSR: offsets
[m + 1] int64, index [total] int32 in ASCENDING j within a row, gap [total] float32.  A plane is valid iff a, b, c, d are finite,
2^-40 <= len <= 2^40 and the four quotients are finite; a margin is valid iff 0 <= margin <= 1e9 (-0.0 is 0.0); a query with an invalid plane
or margin has an empty row.  Brute force over all spheres: no tree.
"""
import numpy as np

import proximity_ref as P
import within_ref as W

F = np.float32
U = 2.0 ** -24


def _planes(planes):
    p = np.ascontiguousarray(planes, dtype=F)
    assert p.ndim == 3 and p.shape[2] == 4 and 1 <= p.shape[1] <= 8, p.shape
    return p


def normalise(planes):
    """([m, K, 4] float32 rows {nx, ny, nz, w}, [m, K] float32 len)"""
    p = _planes(planes)
    with np.errstate(all="ignore"):
        a, b, c = p[..., 0], p[..., 1], p[..., 2]
        ln = np.sqrt((a * a + b * b) + c * c)
        return p / ln[..., None], ln


def plane_ok(planes):
    """[m, K] bool: the validity of every plane"""
    p = _planes(planes)
    q, ln = normalise(p)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(axis=2) & (ln >= F(2.0 ** -40)) & (ln <= F(2.0 ** 40)) & np.isfinite(q).all(axis=2)


def gaps(L, planes):
    """[m, n] float32 gaps of the plane sets [m, K, 4] to the spheres L [n, >= 7] (np.fmax: fmaxf's rule for a NaN operand)"""
    L = np.asarray(L, dtype=F)
    q, _ = normalise(planes)
    e = np.zeros((q.shape[0], L.shape[0]), F)
    with np.errstate(all="ignore"):
        for k in range(q.shape[1]):
            nx, ny, nz, w = (q[:, None, k, s] for s in range(4))
            depth = ((nx * L[None, :, 0] + ny * L[None, :, 1]) + nz * L[None, :, 2]) + w
            e = np.fmax(e, -depth)
        return e - L[None, :, 6]


def in_planes(L, planes, margin, first=None, chunk=None):
    """(offsets [m + 1] int64, index [total] int32, gap [total] float32); margin a scalar or an [m] array; first None or an [m] integer array"""
    L = np.asarray(L, dtype=F)
    p = _planes(planes)
    m, n = p.shape[0], L.shape[0]
    mg = P._bounds(m, margin)
    ok = plane_ok(p).all(axis=1) & P.max_dist_ok(mg)
    fi = np.zeros(m, np.int64) if first is None else np.asarray(first).astype(np.int64)
    assert fi.shape == (m,)
    if chunk is None:
        chunk = max(1, min(256, (1 << 22) // n))
    j = np.arange(n, dtype=np.int64)
    rows, cols, gs = [], [], []
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        g = gaps(L, p[s:e])
        with np.errstate(invalid="ignore"):
            sel = (g <= mg[s:e, None]) & (j[None, :] >= fi[s:e, None]) & ok[s:e, None]
        r, c = np.nonzero(sel)
        rows.append(r + s)
        cols.append(c)
        gs.append(g[r, c])
    if not rows:
        return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, F)
    return W._csr(m, np.concatenate(rows), np.concatenate(cols), np.concatenate(gs))


def depths64(L, planes):
    """[m, K, n] float64 depths of the centres inside the exactly normalised planes, from the float32 inputs"""
    L = np.asarray(L, dtype=np.float64)
    p = _planes(planes).astype(np.float64)
    q = p / np.sqrt((p[..., :3] ** 2).sum(axis=2))[..., None]
    return np.einsum("mkc,nc->mkn", q[..., :3], L[:, :3]) + q[..., 3][..., None]


def gaps64(L, planes):
    """the gaps in float64 (the reference of the CPU suite's accuracy check)"""
    return np.maximum((-depths64(L, planes)).max(axis=1), 0.0) - np.asarray(L, dtype=np.float64)[None, :, 6]


def gap_error_bound(L, planes):
    """[m, n] float64: the bound (R1) of query_core.h on |gaps - gaps64|: u (8.8 |c| + 5.8 max_k |w_k| + r) + 2^-62"""
    L = np.asarray(L, dtype=np.float64)
    p = _planes(planes).astype(np.float64)
    w = np.abs(p[..., 3] / np.sqrt((p[..., :3] ** 2).sum(axis=2))).max(axis=1)
    c = np.sqrt((L[:, :3] ** 2).sum(axis=1))
    return U * (8.8 * c[None, :] + 5.8 * w[:, None] + L[None, :, 6]) + 2.0 ** -62


def box_planes(boxes):
    """[m, 6, 4]: the boxes [m, 6] {lo.xyz, hi.xyz} as their six planes (1,0,0,-lo.x), (0,1,0,-lo.y), (0,0,1,-lo.z), (-1,0,0,hi.x), (0,-1,0,hi.y),
    (0,0,-1,hi.z): len is exactly 1 and every -depth is boxes_ref's per-axis excess, bit for bit"""
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 6)
    p = np.zeros((b.shape[0], 6, 4), F)
    for k in range(3):
        p[:, k, k], p[:, k, 3] = 1.0, -b[:, k]
        p[:, 3 + k, k], p[:, 3 + k, 3] = -1.0, b[:, 3 + k]
    return p


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _through(n, x):
    """planes with inward normals n [.., 3] through the points x [.., 3]"""
    return np.concatenate([n, -(n * x).sum(axis=-1, keepdims=True)], axis=-1)


def random_planes(L, m, K, seed):
    """[m, K, 4] float32: m queries of K planes in and around the scene, by i % 8: 0, 4 random half-spaces through the scene; 1 a slab; 2, 5 an
    oriented box; 3, 6 a frustum from a point in or around the scene; 7 contradictory planes (an empty region).  A shape of more than K planes
    keeps its first K, one of fewer repeats its last plane; every plane is scaled by a power of two between 2^-3 and 2^3 (the normalisation
    works)."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    lo, hi = L[:, :3].min(axis=0), L[:, :3].max(axis=0)
    ext = float(np.max(hi - lo))
    out = np.zeros((m, K, 4), np.float64)
    for i in range(m):
        at = L[rng.integers(0, L.shape[0]), :3] + rng.uniform(-4.0, 4.0, 3)
        kind = i % 8
        if kind in (0, 4):
            n = _unit(rng.normal(size=(K, 3)))
            pl = _through(n, at + rng.uniform(-0.05, 0.05, (K, 3)) * ext)
        elif kind == 1:
            n = _unit(rng.normal(size=3))
            half = rng.uniform(0.0, 0.05) * ext
            pl = np.stack([_through(n, at - half * n), _through(-n, at + half * n)])
        elif kind in (2, 5):
            rot = _rotation(rng)
            half = rng.uniform(0.0, 1.0, 3) ** 2 * 0.25 * ext
            pl = np.stack([_through(s * rot[k], at - s * half[k] * rot[k]) for s in (1.0, -1.0) for k in range(3)])
        elif kind in (3, 6):
            rot = _rotation(rng)
            apex = lo + rng.uniform(-0.5, 1.5, 3) * (hi - lo)
            tx, ty = np.tan(np.radians(rng.uniform(2.0, 35.0, 2)))
            near, far = rng.uniform(0.0, 0.1) * ext, rng.uniform(0.2, 2.0) * ext
            f, r, u = rot
            pl = np.stack([_through(_unit(f * tx + r), apex), _through(_unit(f * tx - r), apex), _through(_unit(f * ty + u), apex),
                           _through(_unit(f * ty - u), apex), _through(f, apex + near * f), _through(-f, apex + far * f)])
        else:
            n = _unit(rng.normal(size=3))
            pl = np.stack([_through(n, at), _through(-n, at - rng.uniform(1.0, 5.0) * n)])
        pl = pl[:K]
        pl = np.concatenate([pl, np.repeat(pl[-1:], K - pl.shape[0], axis=0)])
        out[i] = pl * 2.0 ** rng.integers(-3, 4, (K, 1))
    return np.ascontiguousarray(out, dtype=F)
