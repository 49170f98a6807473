"""numpy float32 restatement of rt_sweep_spheres / rt_sweep_spheres_ranged over the oracle's {L, I}, on top of ray_query_ref.RefScene.

A query is a ray {o, d}, a radius rq and an interval (t_min, t_max): a sphere of radius rq whose centre is o at t = 0 and moves by d per unit t.
For sphere j (centre c, radius r): R = r + rq, t1 / t2 the two roots of sphere_hit of the ray against (c, R) (ray_query_ref's arithmetic with R
for the radius; a discriminant <= 0 gives nothing).  contact_rule: t1 > t_min -> the entry contact tau = t1, start 0, accepted iff t1 < t_max;
otherwise t2 > t_min and t_min < t_max -> the overlap at the start, tau = t_min + 0.0, start 1; otherwise none.  Every compare is False on a NaN.

Sphere j is consulted iff every inner node on its root path passes aabb_hit over (t_min, t_max) on its box widened by rq per component,
fl(bmin - rq) and fl(bmax + rq).  exclude[i] == j skips sphere j for query i.  The contacts are ordered by (tau, j).  Per query: count (all
contacts) and the first min(count, k) as index j, start and {tau, p.xyz, normal.xyz} with p = o + tau d, normal = (1 / R) (p - c); slots past
it are -1, 0 and seven zeros.  A query whose interval fails interval_ok or whose radius fails max_dist_ok has no contact.

sweep tests every (query, node) and every (query, sphere) pair; sweep_walk computes the same with the same elementwise arithmetic over the
pairs a breadth-first walk reaches (for the 10^6-sphere floor).  The CPU suite holds the two equal.  sweep_brute is the per-sphere rule over
ALL spheres, no tree: what the tree-defined answer is compared against.
"""
import numpy as np

from interval_ref import _bounds, interval_ok
from proximity_ref import max_dist_ok
from ray_query_ref import dot

F = np.float32
KMAX = 32


def _radii(n, radius):
    """[n] float32, -0.0 made +0.0 (one float32 addition, as the kernel's)"""
    with np.errstate(invalid="ignore"):
        return (np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=F), (n,))) + F(0)).astype(F)


def query_ok(lo, hi, rq):
    return interval_ok(lo, hi) & max_dist_ok(rq)


def box_pass(ox, oy, oz, dx, dy, dz, bmin, bmax, rq, lo, hi):
    """aabb_hit (ray.fut:53-70) over (lo, hi) of the box (bmin, bmax) widened by rq; every argument broadcasts against the others, bmin / bmax
    are (x, y, z) triples"""
    with np.errstate(all="ignore"):
        tmin, tmax = lo, hi
        ok = True
        for oa, da, b0, b1 in ((ox, dx, bmin[0], bmax[0]), (oy, dy, bmin[1], bmax[1]), (oz, dz, bmin[2], bmax[2])):
            inv = (F(1.0) / da).astype(F)
            t0 = ((b0 - rq) - oa) * inv
            t1 = ((b1 + rq) - oa) * inv
            neg = inv < 0
            tmin = np.fmax(np.where(neg, t1, t0), tmin)   # f32.max: the non-NaN operand
            tmax = np.fmin(np.where(neg, t0, t1), tmax)
            ok = ok & ~(tmax <= tmin)
    return ok


def swept_roots(ox, oy, oz, dx, dy, dz, px, py, pz, rad, rq):
    """(t1, t2, discriminant > 0, R) of the ray against the sphere (p, R = rad + rq); broadcasts"""
    with np.errstate(all="ignore"):
        R = rad + rq
        ocx, ocy, ocz = ox - px, oy - py, oz - pz
        a = dot(dx, dy, dz, dx, dy, dz)
        b = dot(ocx, ocy, ocz, dx, dy, dz)
        c = dot(ocx, ocy, ocz, ocx, ocy, ocz) - R * R
        disc = b * b - a * c
        sq = np.sqrt(disc)
        t1 = (-b - sq) / a
        t2 = (-b + sq) / a
    return t1, t2, ~(disc <= 0), R


def contact_rule(t1, t2, good, lo, hi):
    """(kind: 0 none, 1 entry contact, 2 overlap at the start; tau float32, 0 where there is none)"""
    with np.errstate(invalid="ignore"):
        past = t1 > lo
        entry = good & past & (t1 < hi)
        start = good & ~past & (t2 > lo) & (lo < hi)
        tau = np.where(entry, t1, np.where(start, lo + F(0), F(0))).astype(F)
    return np.where(entry, 1, np.where(start, 2, 0)).astype(np.uint8), tau


def _queries(o, d, radius, t_min, t_max, exclude):
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    n = o.shape[0]
    lo, hi = _bounds(n, t_min, t_max)
    rq = _radii(n, radius)
    ok = query_ok(lo, hi, rq)
    ex = np.full(n, -1, np.int64) if exclude is None else np.asarray(exclude).astype(np.int64)
    assert ex.shape == (n,)
    return o, d, n, lo, hi, rq, ok, ex


def _consulted_chunk(ref, o, d, rq_c, lo_c, hi_c):
    """[m, spheres] bool: every inner ancestor's widened box passes; rq_c, lo_c, hi_c [m, 1]"""
    path = np.zeros((o.shape[0], ref.n - 1), bool)
    for lvl, nodes in enumerate(ref.levels):
        p = box_pass(o[:, 0:1], o[:, 1:2], o[:, 2:3], d[:, 0:1], d[:, 1:2], d[:, 2:3], [ref.bmin[nodes, a][None, :] for a in range(3)],
                     [ref.bmax[nodes, a][None, :] for a in range(3)], rq_c, lo_c, hi_c)
        if lvl > 0:
            p = p & path[:, ref.parent[nodes]]
        path[:, nodes] = p
    return path[:, ref.leaf_parent]


def _dense_contacts(ref, o, d, lo, hi, rq, ok, ex, boxes):
    """kind [m, n] uint8, tau [m, n], R [m, n] of one chunk of queries against every sphere; boxes: restrict to the consulted leaves"""
    m = o.shape[0]
    # (an invalid query's bounds and radius are replaced; its contacts are dropped below anyway)
    lo_c = np.where(ok, lo, F(0))[:, None]
    hi_c = np.where(ok, hi, F(0))[:, None]
    rq_c = np.where(ok, rq, F(0))[:, None]
    ox, oy, oz = o[:, 0:1], o[:, 1:2], o[:, 2:3]
    dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    t1, t2, good, R = swept_roots(ox, oy, oz, dx, dy, dz, ref.pos[None, :, 0], ref.pos[None, :, 1], ref.pos[None, :, 2], ref.rad[None, :], rq_c)
    kind, tau = contact_rule(t1, t2, good, lo_c, hi_c)
    live = ok[:, None] & (np.arange(ref.n)[None, :] != ex[:, None])
    if boxes:
        live = live & _consulted_chunk(ref, o, d, rq_c, lo_c, hi_c)
    return np.where(live, kind, 0).astype(np.uint8), tau, R


def _sweep_dense(ref, o, d, radius, t_min, t_max, k, exclude, chunk, boxes):
    o, d, n, lo, hi, rq, ok, ex = _queries(o, d, radius, t_min, t_max, exclude)
    count = np.zeros(n, np.int32)
    index = np.full((n, k), -1, np.int32)
    start = np.zeros((n, k), np.uint8)
    hit = np.zeros((n, k, 7), F)
    jj = np.arange(ref.n)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        m = e - s
        oo, dd = o[s:e], d[s:e]
        kind, tau, R = _dense_contacts(ref, oo, dd, lo[s:e], hi[s:e], rq[s:e], ok[s:e], ex[s:e], boxes)
        have_all = kind > 0
        count[s:e] = have_all.sum(axis=1)
        key_t = np.where(have_all, tau, F(np.inf))                       # (a contact's tau is finite: tau < t_max <= 1e9)
        order = np.lexsort((np.broadcast_to(jj, (m, ref.n)), key_t), axis=1)[:, :k]
        rows = np.arange(m)[:, None]
        have = have_all[rows, order]
        tk = np.where(have, tau[rows, order], F(0)).astype(F)
        with np.errstate(all="ignore"):
            p = oo[:, None, :] + tk[:, :, None] * dd[:, None, :]         # point_at_param: the moving centre at contact
            nrm = (F(1.0) / R[rows, order])[:, :, None] * (p - ref.pos[order])
        kk = order.shape[1]
        index[s:e, :kk] = np.where(have, order, -1)
        start[s:e, :kk] = np.where(have & (kind[rows, order] == 2), 1, 0)
        hit[s:e, :kk, 0] = tk
        hit[s:e, :kk, 1:4] = np.where(have[:, :, None], p, F(0))
        hit[s:e, :kk, 4:7] = np.where(have[:, :, None], nrm, F(0))
    return count, index, start, hit


def contact_kinds(ref, o, d, radius, t_min, t_max, exclude=None, boxes=True, chunk=256):
    """[n, spheres] uint8: the kind of every (query, sphere) contact (0 none, 1 entry, 2 overlap at the start); boxes=False: without the tree"""
    o, d, n, lo, hi, rq, ok, ex = _queries(o, d, radius, t_min, t_max, exclude)
    out = np.zeros((n, ref.n), np.uint8)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        out[s:e] = _dense_contacts(ref, o[s:e], d[s:e], lo[s:e], hi[s:e], rq[s:e], ok[s:e], ex[s:e], boxes)[0]
    return out


def sweep(ref, o, d, radius, t_min, t_max, k, exclude=None, chunk=256):
    """(count [n] int32, index [n, k] int32, start [n, k] uint8, hit [n, k, 7] float32); radius / t_min / t_max scalars or [n] arrays;
    exclude None or an [n] integer array"""
    return _sweep_dense(ref, o, d, radius, t_min, t_max, k, exclude, chunk, boxes=True)


def sweep_brute(ref, o, d, radius, t_min, t_max, k, exclude=None, chunk=256):
    """sweep without the tree: the per-sphere rule over all spheres"""
    return _sweep_dense(ref, o, d, radius, t_min, t_max, k, exclude, chunk, boxes=False)


def consulted(ref, o, d, radius, t_min, t_max, chunk=256):
    """[n, spheres] bool: the leaves a query consults (every inner ancestor's widened box passes); nothing for an invalid query"""
    o, d, n, lo, hi, rq, ok, ex = _queries(o, d, radius, t_min, t_max, None)
    out = np.zeros((n, ref.n), bool)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        lo_c, hi_c, rq_c = (np.where(ok[s:e], v[s:e], F(0))[:, None] for v in (lo, hi, rq))
        out[s:e] = _consulted_chunk(ref, o[s:e], d[s:e], rq_c, lo_c, hi_c) & ok[s:e, None]
    return out


def sweep_walk(arrays, o, d, radius, t_min, t_max, k, exclude=None):
    """sweep over the pairs a breadth-first walk of the BVH {L, I} (`arrays`: OracleScene.arrays() / Prepared.bvh_arrays()) reaches"""
    o, d, n, lo, hi, rq, ok, ex = _queries(o, d, radius, t_min, t_max, exclude)
    L = np.asarray(arrays["L"], dtype=F)
    pos, rad = L[:, 0:3], L[:, 6]
    bmin, bmax = np.asarray(arrays["bmin"], dtype=F), np.asarray(arrays["bmax"], dtype=F)
    kids = np.stack([np.asarray(arrays["left"], np.int64), np.asarray(arrays["right"], np.int64)], axis=1)   # >= 0 inner, -2 - j leaf j
    ray = np.nonzero(ok)[0]
    node = np.zeros(ray.size, np.int64)
    lr, lj = [], []                                   # the (query, leaf) pairs reached
    while ray.size:
        oo, dd = o[ray], d[ray]
        p = box_pass(oo[:, 0], oo[:, 1], oo[:, 2], dd[:, 0], dd[:, 1], dd[:, 2], [bmin[node, a] for a in range(3)], [bmax[node, a] for a in range(3)],
                     rq[ray], lo[ray], hi[ray])
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
    keep = pj != ex[pr]
    pr, pj = pr[keep], pj[keep]
    oo, dd = o[pr], d[pr]
    t1, t2, good, R = swept_roots(oo[:, 0], oo[:, 1], oo[:, 2], dd[:, 0], dd[:, 1], dd[:, 2], pos[pj, 0], pos[pj, 1], pos[pj, 2], rad[pj], rq[pr])
    kind, tau = contact_rule(t1, t2, good, lo[pr], hi[pr])
    keep = kind > 0
    pr, pj, tau, kind, R = pr[keep], pj[keep], tau[keep], kind[keep], R[keep]
    order = np.lexsort((pj, tau, pr))                 # by query, then (tau, j)
    pr, pj, tau, kind, R = pr[order], pj[order], tau[order], kind[order], R[order]
    count = np.bincount(pr, minlength=n).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    slot = np.arange(pr.size) - first[pr]             # the contact's rank within its query
    sel = slot < k
    pr, pj, tau, kind, R, slot = pr[sel], pj[sel], tau[sel], kind[sel], R[sel], slot[sel]
    index = np.full((n, k), -1, np.int32)
    start = np.zeros((n, k), np.uint8)
    hit = np.zeros((n, k, 7), F)
    with np.errstate(all="ignore"):
        p = o[pr] + tau[:, None] * d[pr]              # point_at_param
        nrm = (F(1.0) / R)[:, None] * (p - pos[pj])
    index[pr, slot] = pj
    start[pr, slot] = kind == 2
    hit[pr, slot, 0] = tau
    hit[pr, slot, 1:4] = p
    hit[pr, slot, 4:7] = nrm
    return count, index, start, hit


def walk_counts(arrays, o, d, radius, t_min, t_max):
    """(boxes [n] int64, leaves [n] int64): the box tests a query's walk makes and the leaves it consults (tools/sweep_probe.py)"""
    o, d, n, lo, hi, rq, ok, ex = _queries(o, d, radius, t_min, t_max, None)
    bmin, bmax = np.asarray(arrays["bmin"], dtype=F), np.asarray(arrays["bmax"], dtype=F)
    kids = np.stack([np.asarray(arrays["left"], np.int64), np.asarray(arrays["right"], np.int64)], axis=1)
    boxes, leaves = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ray = np.nonzero(ok)[0]
    node = np.zeros(ray.size, np.int64)
    while ray.size:
        boxes += np.bincount(ray, minlength=n)
        oo, dd = o[ray], d[ray]
        p = box_pass(oo[:, 0], oo[:, 1], oo[:, 2], dd[:, 0], dd[:, 1], dd[:, 2], [bmin[node, a] for a in range(3)], [bmax[node, a] for a in range(3)],
                     rq[ray], lo[ray], hi[ray])
        ray, node = ray[p], node[p]
        rr, cc = np.repeat(ray, 2), kids[node].reshape(-1)
        leaf = cc < 0
        leaves += np.bincount(rr[leaf], minlength=n)
        ray, node = rr[~leaf], cc[~leaf]
    return boxes, leaves


def rule_cases(o, d, c, r, rq, lo, hi):
    """The per-sphere rule on one (ray, sphere, radius, interval) case per row -> (kind [m] uint8, tau [m] float32): what tools/sweep_check.cpp
    computes with query_core.h's sweep_contact"""
    o, d, c = (np.asarray(v, dtype=F) for v in (o, d, c))
    r, rq, lo, hi = (np.asarray(v, dtype=F) for v in (r, rq, lo, hi))
    t1, t2, good, _ = swept_roots(o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], c[:, 0], c[:, 1], c[:, 2], r, rq)
    return contact_rule(t1, t2, good, lo, hi)
