"""numpy float32 restatement of the box queries (rt_spheres_in_boxes_count / _fill) over a prepared scene's L (oracle_lib.OracleScene(...)
.arrays() or Prepared.bvh_arrays()), built on proximity_ref's helpers with within_ref's CSR assembly.

For a box {lo, hi} and sphere j of L (centre c, radius r) the gap is, in exactly this float32 arithmetic,
    ex = max(max(lo.x - c.x, c.x - hi.x), 0);  ey, ez likewise;   gap = sqrt((ex*ex + ey*ey) + ez*ez) - r
Sphere j is selected for box i iff gap <= the box's margin and j >= first[i] (first absent: 0).  The answer is within_ref's CSR: offsets
[m + 1] int64, index [total] int32 in ASCENDING j within a row, gap [total] float32.  A box is valid iff its six components are finite and
lo_k <= hi_k for every k (zero extent is valid); a margin is valid iff 0 <= margin <= 1e9 (-0.0 is 0.0); an invalid box or margin has an
empty row.  Brute force over all spheres: no tree.  With lo == hi == p the expression is proximity_ref.gaps's, bit for bit.
"""
import numpy as np

import proximity_ref as P
import within_ref as W

F = np.float32


def box_ok(b):
    b = np.asarray(b, dtype=F).reshape(-1, 6)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b).all(axis=1) & (b[:, :3] <= b[:, 3:]).all(axis=1)


def gaps(L, boxes):
    """[m, n] float32 gaps of the boxes [m, 6] to the spheres L [n, >= 7] (np.fmax: fmaxf's rule for a NaN operand)"""
    L = np.asarray(L, dtype=F)
    b = np.asarray(boxes, dtype=F).reshape(-1, 6)
    zero = F(0)
    with np.errstate(all="ignore"):
        e = [np.fmax(np.fmax(b[:, None, k] - L[None, :, k], L[None, :, k] - b[:, None, 3 + k]), zero) for k in range(3)]
        return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) - L[None, :, 6]


def in_boxes(L, boxes, margin, first=None, chunk=None):
    """(offsets [m + 1] int64, index [total] int32, gap [total] float32); margin a scalar or an [m] array; first None or an [m] integer array"""
    L = np.asarray(L, dtype=F)
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 6)
    m, n = b.shape[0], L.shape[0]
    mg = P._bounds(m, margin)
    ok = box_ok(b) & P.max_dist_ok(mg)
    fi = np.zeros(m, np.int64) if first is None else np.asarray(first).astype(np.int64)
    assert fi.shape == (m,)
    if chunk is None:
        chunk = max(1, min(256, (1 << 22) // n))
    j = np.arange(n, dtype=np.int64)
    rows, cols, gs = [], [], []
    for s in range(0, m, chunk):
        e = min(m, s + chunk)
        g = gaps(L, b[s:e])
        with np.errstate(invalid="ignore"):
            sel = (g <= mg[s:e, None]) & (j[None, :] >= fi[s:e, None]) & ok[s:e, None]
        r, c = np.nonzero(sel)
        rows.append(r + s)
        cols.append(c)
        gs.append(g[r, c])
    if not rows:
        return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, F)
    return W._csr(m, np.concatenate(rows), np.concatenate(cols), np.concatenate(gs))


def gaps64(L, boxes):
    """the same gaps in float64 from the float32 inputs (the reference of the CPU suite's accuracy check)"""
    L = np.asarray(L, dtype=np.float64)
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    e = [np.maximum(np.maximum(b[:, None, k] - L[None, :, k], L[None, :, k] - b[:, None, 3 + k]), 0.0) for k in range(3)]
    return np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - L[None, :, 6]


def random_boxes(L, m, seed, max_half=0.25, zero_every=8):
    """m boxes in and around the scene: centres at sphere centres displaced by up to 4 units per axis, half-extents u^3 * max_half * extent per
    axis (u uniform in [0, 1): mixed sizes, mostly small); every zero_every-th box is degenerate (lo == hi) and the one after it flat in y"""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=F)
    ext = float(np.max(L[:, :3].max(axis=0) - L[:, :3].min(axis=0)))
    c = L[rng.integers(0, L.shape[0], m), :3].astype(np.float64) + rng.uniform(-4.0, 4.0, (m, 3))
    half = rng.uniform(0.0, 1.0, (m, 3)) ** 3 * max_half * ext
    if zero_every:
        half[::zero_every] = 0.0
        half[1::zero_every, 1] = 0.0
    lo, hi = (c - half).astype(F), (c + half).astype(F)
    return np.ascontiguousarray(np.concatenate([np.minimum(lo, hi), np.maximum(lo, hi)], axis=1))


def degenerate(points):
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([p, p], axis=1))
