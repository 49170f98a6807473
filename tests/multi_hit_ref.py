"""numpy float32 restatement of rt_multi_hit_rays / rt_multi_hit_rays_ranged over the oracle's {L, I}, on top of ray_query_ref.RefScene.

The crossings of ray r over (t_min, t_max) are every (t, j, root) with leaf j visited (RefScene.visited: every inner ancestor's box passes
aabb_hit over the interval -- occlusion_ref's leaves) and t root 1 or root 2 of sphere_hit L[j] r (RefScene.roots) strictly inside the
interval.  Ordered by t, then j, then root (a lexicographic sort).  Per ray: count = the number of crossings, and the first min(count, k)
of them as (index j, root, {t, p.xyz, normal.xyz}) with p = o + t d, normal = (1 / radius) (p - centre); slots past it are -1, 0 and
seven zeros.  Per-ray bounds follow interval_ref: a ray whose interval fails interval_ok has no crossing.

multi_hit tests every (ray, node) and every (ray, sphere) pair, which is out of reach for a scene of 10^6 spheres (ctx.floor(1000, 6000)).
multi_hit_walk computes the same with the same float32 arithmetic over the pairs a breadth-first walk reaches: a node is tested only when
its parent passed, so a leaf is reached iff every inner ancestor passed.  The CPU suite holds the two equal on the small scenes.
"""
import numpy as np

from interval_ref import _bounds, interval_ok
from occlusion_ref import _inside
from ray_query_ref import dot

F = np.float32
KMAX = 32


def multi_hit(ref, o, d, t_min, t_max, k, chunk=256):
    """(count [n] int32, index [n, k] int32, root [n, k] uint8, hit [n, k, 7] float32); t_min / t_max scalars or [n] arrays."""
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    nr, ns = o.shape[0], ref.n
    lo_all, hi_all = _bounds(nr, t_min, t_max)
    ok_all = interval_ok(lo_all, hi_all)
    count = np.zeros(nr, np.int32)
    index = np.full((nr, k), -1, np.int32)
    root = np.zeros((nr, k), np.uint8)
    hit = np.zeros((nr, k, 7), F)
    jj = np.concatenate([np.arange(ns), np.arange(ns)])                  # columns: root 1 of every sphere, then root 2
    rr = np.concatenate([np.full(ns, 1), np.full(ns, 2)]).astype(np.uint8)
    for s in range(0, nr, chunk):
        e = min(nr, s + chunk)
        ok = ok_all[s:e]
        # (an invalid ray's bounds are replaced by an empty interval; its crossings are dropped below anyway)
        lo = np.where(ok, lo_all[s:e], F(0))[:, None]
        hi = np.where(ok, hi_all[s:e], F(0))[:, None]
        oo, dd = o[s:e], d[s:e]
        vis = ref.visited(oo, dd, lo, hi) & ok[:, None]
        r1, r2, pos = ref.roots(oo, dd)
        t = np.concatenate([r1, r2], axis=1)
        inside = np.concatenate([vis & pos & _inside(r1, lo, hi), vis & pos & _inside(r2, lo, hi)], axis=1)
        count[s:e] = inside.sum(axis=1)
        key_t = np.where(inside, t, F(np.inf))                           # (crossings are finite: t < t_max <= 1e9)
        m = e - s
        order = np.lexsort((np.broadcast_to(rr, (m, 2 * ns)), np.broadcast_to(jj, (m, 2 * ns)), key_t), axis=1)[:, :k]
        rows = np.arange(m)[:, None]
        have = inside[rows, order]
        tk = np.where(have, t[rows, order], F(0)).astype(F)
        jk = jj[order]
        with np.errstate(all="ignore"):
            p = oo[:, None, :] + tk[:, :, None] * dd[:, None, :]         # point_at_param
            nrm = ref.inv_rad[jk][:, :, None] * (p - ref.pos[jk])        # scale (1.0/s.radius) (p - s.pos)
        kk = order.shape[1]
        index[s:e, :kk] = np.where(have, jk, -1)
        root[s:e, :kk] = np.where(have, rr[order], 0)
        hit[s:e, :kk, 0] = tk
        hit[s:e, :kk, 1:4] = np.where(have[:, :, None], p, F(0))
        hit[s:e, :kk, 4:7] = np.where(have[:, :, None], nrm, F(0))
    return count, index, root, hit


def _pair_boxes(bmin, bmax, o, d, lo, hi):
    """RefScene._boxes for one (ray, node) pair per row: o, d, bmin, bmax [m, 3], lo, hi [m]."""
    tmin, tmax = lo.astype(F), hi.astype(F)
    ok = np.ones(o.shape[0], bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = (F(1.0) / d[:, a]).astype(F)
            t0 = (bmin[:, a] - o[:, a]) * inv
            t1 = (bmax[:, a] - o[:, a]) * inv
            neg = inv < 0
            t0s, t1s = np.where(neg, t1, t0), np.where(neg, t0, t1)
            tmin = np.fmax(t0s, tmin)
            tmax = np.fmin(t1s, tmax)
            ok &= ~(tmax <= tmin)
    return ok


def _pair_roots(pos, rad, o, d):
    """RefScene.roots for one (ray, sphere) pair per row."""
    ocx, ocy, ocz = o[:, 0] - pos[:, 0], o[:, 1] - pos[:, 1], o[:, 2] - pos[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        a = dot(dx, dy, dz, dx, dy, dz)
        b = dot(ocx, ocy, ocz, dx, dy, dz)
        c = dot(ocx, ocy, ocz, ocx, ocy, ocz) - rad * rad
        disc = b * b - a * c
        sq = np.sqrt(disc)
        r1 = (-b - sq) / a
        r2 = (-b + sq) / a
    return r1, r2, ~(disc <= 0)


def multi_hit_walk(arrays, o, d, t_min, t_max, k):
    """multi_hit over the pairs a breadth-first walk of the BVH {L, I} (`arrays`: OracleScene.arrays() / Prepared.bvh_arrays()) reaches."""
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    L = np.asarray(arrays["L"], dtype=F)
    pos, rad = L[:, 0:3], L[:, 6]
    inv_rad = (F(1.0) / rad).astype(F)
    bmin, bmax = np.asarray(arrays["bmin"], dtype=F), np.asarray(arrays["bmax"], dtype=F)
    kids = np.stack([np.asarray(arrays["left"], np.int64), np.asarray(arrays["right"], np.int64)], axis=1)   # >= 0 inner, -2 - j leaf j
    nr = o.shape[0]
    lo_all, hi_all = _bounds(nr, t_min, t_max)
    ok = interval_ok(lo_all, hi_all)
    ray = np.nonzero(ok)[0]
    node = np.zeros(ray.size, np.int64)
    lr, lj = [], []                                   # the (ray, leaf) pairs reached
    while ray.size:
        p = _pair_boxes(bmin[node], bmax[node], o[ray], d[ray], lo_all[ray], hi_all[ray])
        ray, node = ray[p], node[p]
        c = kids[node]                                # [m, 2]
        rr = np.repeat(ray, 2)
        cc = c.reshape(-1)
        leaf = cc < 0
        lr.append(rr[leaf])
        lj.append(-2 - cc[leaf])
        ray, node = rr[~leaf], cc[~leaf]
    pr = np.concatenate(lr) if lr else np.zeros(0, np.int64)
    pj = np.concatenate(lj) if lj else np.zeros(0, np.int64)
    r1, r2, good = _pair_roots(pos[pj], rad[pj], o[pr], d[pr])
    lo, hi = lo_all[pr], hi_all[pr]
    cr = np.concatenate([pr, pr])
    cj = np.concatenate([pj, pj])
    ct = np.concatenate([r1, r2]).astype(F)
    croot = np.concatenate([np.full(pr.size, 1), np.full(pr.size, 2)]).astype(np.uint8)
    keep = np.concatenate([good & _inside(r1, lo, hi), good & _inside(r2, lo, hi)])
    cr, cj, ct, croot = cr[keep], cj[keep], ct[keep], croot[keep]
    order = np.lexsort((croot, cj, ct, cr))           # by ray, then (t, j, root)
    cr, cj, ct, croot = cr[order], cj[order], ct[order], croot[order]
    count = np.bincount(cr, minlength=nr).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    slot = np.arange(cr.size) - first[cr]             # the crossing's rank within its ray
    sel = slot < k
    cr, cj, ct, croot, slot = cr[sel], cj[sel], ct[sel], croot[sel], slot[sel]
    index = np.full((nr, k), -1, np.int32)
    root = np.zeros((nr, k), np.uint8)
    hit = np.zeros((nr, k, 7), F)
    with np.errstate(all="ignore"):
        p = o[cr] + ct[:, None] * d[cr]               # point_at_param
        nrm = inv_rad[cj][:, None] * (p - pos[cj])
    index[cr, slot] = cj
    root[cr, slot] = croot
    hit[cr, slot, 0] = ct
    hit[cr, slot, 1:4] = p
    hit[cr, slot, 4:7] = nrm
    return count, index, root, hit
