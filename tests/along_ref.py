"""numpy float32 restatement of rt_spheres_along_rays_count / _fill over the oracle's {L, I}, built from sweep_ref's pieces.

A query is sweep_ref's: a ray {o, d}, a radius rq, an interval (t_min, t_max).  Sphere j is selected for query i iff it is consulted (every inner
ancestor's box widened by rq passes aabb_hit over the interval: sweep_ref._consulted_chunk), sweep_ref.contact_rule on the roots of the ray
against (c, R = r + rq) (sweep_ref.swept_roots) gives a contact, j != exclude[i] and j >= first[i].  There is no k: the answer is CSR --
offsets [n + 1] int64, index [total] int32 in ascending j within a row, roots [total, 2] float32 = {t1, t2} as the rule compared them
(unclamped), start [total] uint8 (1: an overlap at the start).  A query failing sweep_ref.query_ok has an empty row.

along(.., boxes=False) is the brute force: the per-sphere rule over ALL spheres.  `mutant` names a deliberately wrong variant (MUTANTS); the
CPU suite shows that each is caught by a named input.  row_contacts / row_crossings are plain per-row twins of the package's helpers of
the same names: the rows as sweep_ref.sweep and multi_hit_ref.multi_hit list them.
"""
import numpy as np

from interval_ref import _bounds
from sweep_ref import _consulted_chunk, _radii, box_pass, contact_rule, query_ok, swept_roots

F = np.float32
MUTANTS = ("multi_hit_set", "boxes_not_widened", "exclude_ignored", "first_off_by_one", "tau_order", "roots_of_r", "tau_t1_at_start")


def along(ref, o, d, radius, t_min, t_max, exclude=None, first=None, boxes=True, chunk=256, mutant=None):
    """(offsets [n + 1] int64, index [total] int32, roots [total, 2] float32, start [total] uint8); radius / t_min / t_max scalars or [n]
    arrays; exclude, first: None or [n] integer arrays"""
    assert mutant is None or mutant in MUTANTS, mutant
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    n = o.shape[0]
    lo, hi = _bounds(n, t_min, t_max)
    rq = _radii(n, radius)
    ok = query_ok(lo, hi, rq)
    ex = np.full(n, -1, np.int64) if exclude is None or mutant == "exclude_ignored" else np.asarray(exclude).astype(np.int64)
    fi = np.zeros(n, np.int64) if first is None else np.asarray(first).astype(np.int64)
    if mutant == "first_off_by_one" and first is not None:
        fi = fi + 1
    assert ex.shape == (n,) and fi.shape == (n,)
    jj = np.arange(ref.n)
    counts = np.zeros(n, np.int64)
    out_j, out_r, out_s = [], [], []
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        oo, dd, okc = o[s:e], d[s:e], ok[s:e]
        # (an invalid query's bounds and radius are replaced; its row is dropped below)
        lo_c, hi_c, rq_c = (np.where(okc, v[s:e], F(0))[:, None] for v in (lo, hi, rq))
        ox, oy, oz, dx, dy, dz = (a[:, k:k + 1] for a in (oo, dd) for k in range(3))
        px, py, pz, rad = ref.pos[None, :, 0], ref.pos[None, :, 1], ref.pos[None, :, 2], ref.rad[None, :]
        t1, t2, good, _ = swept_roots(ox, oy, oz, dx, dy, dz, px, py, pz, rad, rq_c)
        kind, tau = contact_rule(t1, t2, good, lo_c, hi_c)
        if mutant == "multi_hit_set":
            with np.errstate(invalid="ignore"):
                kind = np.where((kind == 2) & ~(t2 < hi_c), 0, kind)
        live = okc[:, None] & (jj[None, :] != ex[s:e, None]) & (jj[None, :] >= fi[s:e, None]) & (kind > 0)
        if boxes:
            live = live & _consulted_chunk(ref, oo, dd, F(0) * rq_c if mutant == "boxes_not_widened" else rq_c, lo_c, hi_c)
        if mutant == "roots_of_r":
            t1, t2, _, _ = swept_roots(ox, oy, oz, dx, dy, dz, px, py, pz, rad, F(0) * rq_c)
        counts[s:e] = live.sum(axis=1)
        r, j = np.nonzero(live)                                           # row-major: by query, then ascending j
        if mutant == "tau_order":
            order = np.lexsort((j, tau[r, j], r))
            r, j = r[order], j[order]
        out_j.append(j.astype(np.int32))
        out_r.append(np.stack([t1[r, j], t2[r, j]], axis=1).astype(F))
        out_s.append((kind[r, j] == 2).astype(np.uint8))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if not out_j:
        return offsets, np.zeros(0, np.int32), np.zeros((0, 2), F), np.zeros(0, np.uint8)
    return offsets, np.concatenate(out_j), np.concatenate(out_r).reshape(-1, 2), np.concatenate(out_s)


def along_brute(ref, o, d, radius, t_min, t_max, exclude=None, first=None, chunk=256):
    """along without the tree: the per-sphere rule over all spheres"""
    return along(ref, o, d, radius, t_min, t_max, exclude, first, boxes=False, chunk=chunk)


def along_walk(arrays, o, d, radius, t_min, t_max, exclude=None, first=None):
    """along over the pairs a breadth-first walk of the BVH {L, I} (`arrays`: OracleScene.arrays() / Prepared.bvh_arrays()) reaches, with the
    same elementwise arithmetic: for scenes too large for the dense form.  The CPU suite holds the two equal."""
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    n = o.shape[0]
    lo, hi = _bounds(n, t_min, t_max)
    rq = _radii(n, radius)
    ok = query_ok(lo, hi, rq)
    ex = np.full(n, -1, np.int64) if exclude is None else np.asarray(exclude).astype(np.int64)
    fi = np.zeros(n, np.int64) if first is None else np.asarray(first).astype(np.int64)
    L = np.asarray(arrays["L"], dtype=F)
    pos, rad = L[:, 0:3], L[:, 6]
    bmin, bmax = np.asarray(arrays["bmin"], dtype=F), np.asarray(arrays["bmax"], dtype=F)
    kids = np.stack([np.asarray(arrays["left"], np.int64), np.asarray(arrays["right"], np.int64)], axis=1)   # >= 0 inner, -2 - j leaf j
    ray = np.nonzero(ok)[0]
    node = np.zeros(ray.size, np.int64)
    lr, lj = [], []
    while ray.size:
        oo, dd = o[ray], d[ray]
        p = box_pass(oo[:, 0], oo[:, 1], oo[:, 2], dd[:, 0], dd[:, 1], dd[:, 2], [bmin[node, a] for a in range(3)], [bmax[node, a] for a in range(3)],
                     rq[ray], lo[ray], hi[ray])
        ray, node = ray[p], node[p]
        rr, cc = np.repeat(ray, 2), kids[node].reshape(-1)
        leaf = cc < 0
        lr.append(rr[leaf])
        lj.append(-2 - cc[leaf])
        ray, node = rr[~leaf], cc[~leaf]
    pr = np.concatenate(lr) if lr else np.zeros(0, np.int64)
    pj = np.concatenate(lj) if lj else np.zeros(0, np.int64)
    keep = (pj != ex[pr]) & (pj >= fi[pr])
    pr, pj = pr[keep], pj[keep]
    oo, dd = o[pr], d[pr]
    t1, t2, good, _ = swept_roots(oo[:, 0], oo[:, 1], oo[:, 2], dd[:, 0], dd[:, 1], dd[:, 2], pos[pj, 0], pos[pj, 1], pos[pj, 2], rad[pj], rq[pr])
    kind, _ = contact_rule(t1, t2, good, lo[pr], hi[pr])
    keep = kind > 0
    pr, pj, t1, t2, kind = pr[keep], pj[keep], t1[keep], t2[keep], kind[keep]
    order = np.lexsort((pj, pr))
    pr, pj, t1, t2, kind = pr[order], pj[order], t1[order], t2[order], kind[order]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(pr, minlength=n))]).astype(np.int64)
    return offsets, pj.astype(np.int32), np.stack([t1, t2], axis=1).astype(F).reshape(-1, 2), (kind == 2).astype(np.uint8)


def rule_cases(o, d, c, r, rq, lo, hi):
    """The per-sphere rule on one (ray, sphere, radius, interval) case per row -> (kind [m] uint8, tau [m] float32, good [m] bool, t1 [m], t2 [m]
    float32, zero where not good): what tools/along_check.cpp computes with query_core.h's sweep_contact_roots"""
    o, d, c = (np.asarray(v, dtype=F) for v in (o, d, c))
    r, rq, lo, hi = (np.asarray(v, dtype=F) for v in (r, rq, lo, hi))
    t1, t2, good, _ = swept_roots(o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], c[:, 0], c[:, 1], c[:, 2], r, rq)
    kind, tau = contact_rule(t1, t2, good, lo, hi)
    return kind, tau, good, np.where(good, t1, F(0)).astype(F), np.where(good, t2, F(0)).astype(F)


def _bound(n, b):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=F), (n,)))


def row_contacts(offsets, index, roots, start, t_min, k, mutant=None):
    """(count [n] int32, index [n, k] int32, start [n, k] uint8, tau [n, k] float32): every row in (tau, j) order, tau = t_min + 0.0 for an
    overlap at the start and t1 otherwise, the first min(count, k), padded with -1, 0, 0.0 -- a loop over the rows"""
    n = offsets.size - 1
    lo = _bound(n, t_min)
    count = np.diff(offsets).astype(np.int32)
    idx, st, tk = np.full((n, k), -1, np.int32), np.zeros((n, k), np.uint8), np.zeros((n, k), F)
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        if a == b:
            continue
        s = start[a:b] != 0
        tau = np.where(s & (mutant != "tau_t1_at_start"), lo[i] + F(0), roots[a:b, 0]).astype(F)
        order = np.lexsort((index[a:b], tau))[:k]
        m = order.size
        idx[i, :m], st[i, :m], tk[i, :m] = index[a:b][order], start[a:b][order], tau[order]
    return count, idx, st, tk


def row_crossings(offsets, index, roots, t_min, t_max, k):
    """(count [n] int32, index [n, k] int32, root [n, k] uint8, t [n, k] float32): the roots of every row's entries strictly inside
    (t_min, t_max) in (t, j, root) order (root 1: t1, 2: t2), the first min(count, k), padded with -1, 0, 0.0 -- a loop over the rows"""
    n = offsets.size - 1
    lo, hi = _bound(n, t_min), _bound(n, t_max)
    count = np.zeros(n, np.int32)
    idx, rt, tk = np.full((n, k), -1, np.int32), np.zeros((n, k), np.uint8), np.zeros((n, k), F)
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        if a == b:
            continue
        t = np.concatenate([roots[a:b, 0], roots[a:b, 1]])
        j = np.concatenate([index[a:b], index[a:b]])
        which = np.repeat(np.array([1, 2], np.uint8), b - a)
        with np.errstate(invalid="ignore"):
            keep = (t > lo[i]) & (t < hi[i])
        t, j, which = t[keep], j[keep], which[keep]
        count[i] = t.size
        order = np.lexsort((which, j, t))[:k]
        m = order.size
        idx[i, :m], rt[i, :m], tk[i, :m] = j[order], which[order], t[order]
    return count, idx, rt, tk
