"""Edge inputs for the sphere casts (plain numpy), on top of edge_rays.py: the edge scenes plus one with zero-radius spheres, and small named
families of queries -- a ray, a radius rq and an interval each -- that sit on the edges of the contact rule (sweep_ref.py): a root equal to
t_min or t_max bit for bit, a zero discriminant of the inflated sphere, stationary queries, many contacts at one tau, origins on a widened
box face, radii that absorb the coordinates and inflated radii of zero.

`sweep_families` returns {name: (rays [m, 6], radius [m], t_min [m], t_max [m])}, all float32; `sweep_targets` returns, for the same
arguments, {name: j [m]}: the sphere each query was aimed at (-1 where it has none).  A family that a scene cannot give (no integer sphere
for `grazing`, no zero-radius sphere for `zero_radius`) is absent from both.
"""
import numpy as np

import edge_rays as E
from multi_hit_ref import _pair_roots

F = np.float32
NEG0 = E.NEG0
INF = F(np.inf)
RQ_EDGES = (F(0.0), NEG0, F(1e-40), None, F(40.0), F(1e8), F(1e9))      # None: the scene's median radius
T_MINS = (F(0.1), F(0.5))
DYADIC_RQ = (F(0.0), F(0.5), F(2.0), F(0.25))


def _random600_r0():
    # random600 with 20 radii set to zero, every other one of them to -0.0: with rq = 0 the inflated radius R is 0 (1 / R is inf), with a
    # denormal rq it is denormal (R * R underflows to 0)
    s = E.SCENES["random600"][0].copy()
    j = np.random.default_rng(4321).permutation(s.shape[0])[:20]
    s[j[0::2], 6] = F(0.0)
    s[j[1::2], 6] = NEG0
    return s


SCENES = dict(E.SCENES)
SCENES["random600_r0"] = (_random600_r0(),) + E.SCENES["random600"][1:]
INTEGER_SCENES = ("two_apart", "two_same", "same64", "nan_grid", "overlap")     # the scenes that have spheres with integer centres and radii


def median_radius(arrays):
    return F(np.median(np.asarray(arrays["L"], dtype=F)[:, 6]))


def _pack(rays, radius, t_min, t_max, target):
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    m = rays.shape[0]
    out = [rays]
    for v in (radius, t_min, t_max):
        out.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=F), (m,))).copy())
    out.append(np.ascontiguousarray(np.broadcast_to(np.asarray(target, dtype=np.int64), (m,))).copy())
    return tuple(out)


def _cat(parts):
    parts = [p for p in parts if p[0].shape[0] > 0]
    if not parts:
        return None
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))


def _take(fam, rng, m):
    if fam is None:
        return None
    keep = np.sort(rng.permutation(fam[0].shape[0])[:m])
    return tuple(v[keep] for v in fam)


def _roots(L, rays, j, rq):
    """(t1, t2, discriminant > 0) of each ray against its own sphere j inflated by rq: sweep_ref.swept_roots' arithmetic, one pair per row"""
    with np.errstate(all="ignore"):
        R = (L[j, 6] + (rq + F(0))).astype(F)
        return _pair_roots(L[j, :3], R, rays[:, :3], rays[:, 3:])


def _aimed(L, rng, m, rq):
    """m rays from outside sphere j's inflated surface towards a point inside it, at speeds 0.1 .. 10: (rays, j)"""
    n = L.shape[0]
    j = rng.integers(0, n, m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    R = (L[j, 6] + rq).astype(np.float64)
    dist = R * rng.uniform(1.2, 4.0, m) + rng.uniform(0.5, 20.0, m)
    o = L[j, :3] + u * dist[:, None]
    aim = L[j, :3] + rng.normal(size=(m, 3)) * (0.4 * R[:, None])
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= 10.0 ** rng.uniform(-1, 1, (m, 1))
    return E._rays(o.astype(F), d.astype(F)), j


def _int_spheres(L):
    """the spheres whose centre and radius are integers (and the radius at least 1): their grazing arithmetic is exact"""
    return np.nonzero((L[:, :3] == np.round(L[:, :3])).all(axis=1) & (L[:, 6] == np.round(L[:, 6])) & (L[:, 6] >= 1))[0]


# ------------------------------------------------------------------------------------------------------------- the families
def _ray_edges(arrays, seed, per, cap):
    fam = E.ray_families(arrays, seed=seed, per=per)
    rays = np.concatenate([v[:cap] for v in fam.values()])
    m = rays.shape[0]
    r0 = median_radius(arrays)
    radii = np.array([r0 if v is None else v for v in RQ_EDGES], F)
    lo, hi, _ = E.edge_intervals(arrays, rays, seed=seed)
    return _pack(rays, radii[np.arange(m) % len(radii)], lo, hi, -1)


def _root_families(arrays, rng, per):
    """entry_at_t_min, entry_just_past_t_min, exit_at_t_min, entry_at_t_max: found by search for t_min / t_max in T_MINS, and with the bound
    set to the query's own root"""
    L = np.asarray(arrays["L"], dtype=F)
    n = L.shape[0]
    r0 = median_radius(arrays)
    out = {k: [] for k in ("entry_at_t_min", "entry_just_past_t_min", "exit_at_t_min", "entry_at_t_max")}
    # by search: the root equals the fixed bound
    for j in rng.permutation(n)[:4]:
        for axis in range(3):
            for sign in (1.0, -1.0):
                for rq in (F(0.0), F(0.5), r0):
                    R = F(L[j, 6] + rq)
                    for t in T_MINS:
                        nxt = np.nextafter(t, INF, dtype=F)
                        r = E._search_root(L[j, :3], R, axis, t, sign, which=(1,))
                        out["entry_at_t_min"].append(_pack(r, rq, t, 1e9, j))
                        out["entry_at_t_max"].append(_pack(r, rq, 0.0, t, j))
                        out["entry_at_t_max"].append(_pack(r, rq, 0.0, nxt, j))
                        r = E._search_root(L[j, :3], R, axis, nxt, sign, which=(1,))
                        out["entry_just_past_t_min"].append(_pack(r, rq, t, 1e9, j))
                        r = E._search_root(L[j, :3], R, axis, t, sign, which=(2,))
                        out["exit_at_t_min"].append(_pack(r, rq, t, 1e9, j))
    found = {k: _take(_cat(v), rng, per // 2) for k, v in out.items()}
    # the query's own roots as bounds
    own = {k: [] for k in out}
    for rq in (F(0.0), r0, F(40.0)):
        rays, j = _aimed(L, rng, per // 3, rq)
        t1, t2, ok = _roots(L, rays, j, rq)
        with np.errstate(invalid="ignore"):
            good = ok & np.isfinite(t1) & np.isfinite(t2) & (t1 > F(1e-3)) & (t2 < F(1e8))
        rays, j, t1, t2 = rays[good], j[good], t1[good], t2[good]
        below = np.nextafter(t1, -INF, dtype=F)
        own["entry_at_t_min"].append(_pack(rays, rq, t1, 1e9, j))
        own["entry_just_past_t_min"].append(_pack(rays, rq, below, 1e9, j))
        own["exit_at_t_min"].append(_pack(rays, rq, t2, 1e9, j))
        own["entry_at_t_max"].append(_pack(rays, rq, 0.0, t1, j))
        own["entry_at_t_max"].append(_pack(rays, rq, 0.0, np.nextafter(t1, INF, dtype=F), j))
    return {k: _cat([p for p in (found[k], _cat(own[k])) if p is not None]) for k in out}


def _grazing(arrays, rng, per):
    """axis-aligned rays offset from an integer sphere's centre by exactly R = r + rq (rq dyadic): b * b == a * c, disc == 0; and the two
    neighbours an ulp inside and outside"""
    L = np.asarray(arrays["L"], dtype=F)
    cand = _int_spheres(L)
    if cand.size == 0:
        return None
    parts = []
    per = per // 2
    for which in (0, 1, 2):                  # exactly tangent, one ulp inside, one ulp outside
        j = cand[rng.integers(0, cand.size, per)]
        ax = rng.integers(0, 3, per)
        perp = (ax + rng.integers(1, 3, per)) % 3
        sgn = np.where(rng.random(per) < 0.5, F(1), F(-1))
        side = np.where(rng.random(per) < 0.5, F(1), F(-1))
        rq = np.array(DYADIC_RQ, F)[rng.integers(0, len(DYADIC_RQ), per)]
        speed = np.array([0.5, 1.0, 2.0], F)[rng.integers(0, 3, per)]
        R = (L[j, 6] + rq).astype(F)
        rows = np.arange(per)
        o = L[j, :3].copy()
        o[rows, ax] -= sgn * F(48.0)
        off = (L[j, perp] + side * R).astype(F)
        if which == 1:
            off = np.nextafter(off, L[j, perp], dtype=F)
        elif which == 2:
            off = np.nextafter(off, side * INF, dtype=F)
        o[rows, perp] = off
        d = np.zeros((per, 3), F)
        d[rows, ax] = sgn * speed
        parts.append(_pack(E._rays(o, d), rq, 0.0, 1e9, j))
    return _cat(parts)


def _stationary(arrays, rng, per):
    """d = +0 and d = -0: at a centre, inside the inflated sphere and outside it.  a = b = 0, so disc = 0 - 0 * c is 0 (NaN when c
    overflows): no contact, however deep the overlap"""
    L = np.asarray(arrays["L"], dtype=F)
    r0 = median_radius(arrays)
    parts = []
    per = per // 2
    for rq, (lo, hi) in ((F(0.0), (0.0, 1e9)), (r0, (0.0, 1.0)), (F(40.0), (0.5, 1e9)), (F(1e9), (0.0, 1e9))):
        j = rng.integers(0, L.shape[0], per)
        u = rng.normal(size=(per, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        R = (L[j, 6] + rq).astype(np.float64)
        where = np.array([0.0, 0.5, 2.0])[np.arange(per) % 3]
        o = (L[j, :3] + u * (R * where)[:, None]).astype(F)
        d = np.where((np.arange(per) % 2 == 0)[:, None], F(0.0), NEG0) * np.ones((per, 3), F)
        parts.append(_pack(E._rays(o, d.astype(F)), rq, lo, hi, j))
    return _cat(parts)


def _tie_groups(L):
    """(groups of exact duplicates (centre and radius), pairs of equal integer spheres that differ along one axis)"""
    key = np.ascontiguousarray(L[:, [0, 1, 2, 6]]).view(np.uint32).reshape(L.shape[0], 4)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    dupes = [np.nonzero(inv == g)[0] for g in np.nonzero(cnt > 1)[0]]
    ints = _int_spheres(L)[:64]
    pairs = []
    for a in ints:
        for b in ints:
            diff = L[b, :3] - L[a, :3]
            if a < b and L[a, 6] == L[b, 6] and (diff != 0).sum() == 1:
                pairs.append((a, b, int(np.nonzero(diff)[0][0])))
    return dupes, pairs


def _ties(arrays, rng, per):
    L = np.asarray(arrays["L"], dtype=F)
    n = L.shape[0]
    r0 = median_radius(arrays)
    dupes, pairs = _tie_groups(L)
    parts = []
    # equal entry times: axis-aligned rays from outside at a group of coincident spheres ...
    for g in dupes[: per // 8 + 1]:
        for axis in range(3):
            e = np.zeros(3, F)
            e[axis] = 1
            for sign, rq in ((F(1), F(0.0)), (F(-1), F(0.5))):
                parts.append(_pack(E._rays(L[g[0], :3] - sign * F(32.0) * e, sign * e), rq, 0.0, 1e9, g[0]))
    # ... and from the mid-plane of two equal integer spheres: o - c differs between them in one sign only, so the two entries are equal
    for a, b, axis in [pairs[i] for i in rng.permutation(len(pairs))[: per // 2]]:
        other = (axis + 1 + int(rng.integers(0, 2))) % 3
        mid = ((L[a, :3] + L[b, :3]) * F(0.5)).astype(F)
        half = abs(float(L[b, axis] - L[a, axis])) * 0.5
        rq = F(max(0.0, np.ceil(half) + 1.0 - float(L[a, 6])))
        e = np.zeros(3, F)
        e[other] = 1
        parts.append(_pack(E._rays(mid - F(64.0) * e, e), rq, 0.0, 1e9, a))
    # more than 32 overlaps at the start: origins at and near sphere centres, a radius that spans many spheres
    for rq, lo in ((r0, 0.0), (F(40.0), 0.0), (F(40.0), 0.25), (F(16.0), NEG0)):
        j = rng.integers(0, n, per // 4)
        o = (L[j, :3] + rng.normal(size=(per // 4, 3)) * 0.25 * float(r0)).astype(F)
        d = rng.normal(size=(per // 4, 3)).astype(F)
        parts.append(_pack(E._rays(o, d), rq, lo, 1e9, j))
    # one entry at nextafter(t_min) behind a block of overlaps at t_min: t_min is the ulp below the earliest entry of a sphere that the
    # query does not overlap yet
    per = per // 3
    for rq in (r0, F(8.0), F(40.0)):
        j = rng.integers(0, n, per)
        o = (L[j, :3] + rng.normal(size=(per, 3)) * 0.25 * float(r0)).astype(F)
        to = L[rng.integers(0, n, per), :3] + rng.normal(size=(per, 3)).astype(F)
        d = (to - o).astype(F)
        rays = E._rays(o, d)
        with np.errstate(all="ignore"):
            R = (L[None, :, 6] + rq).astype(F)
            pos = np.broadcast_to(L[None, :, :3], (per, n, 3)).reshape(-1, 3)
            t1, t2, ok = _pair_roots(pos, np.broadcast_to(R, (per, n)).reshape(-1), np.repeat(o, n, axis=0), np.repeat(d, n, axis=0))
            t1, t2, ok = t1.reshape(per, n), t2.reshape(per, n), ok.reshape(per, n)
            ahead = ok & (t1 > F(1e-3)) & np.isfinite(t1)
        first = np.where(ahead, t1, INF)
        tgt = np.argmin(first, axis=1)
        t = first[np.arange(per), tgt]
        lo = np.nextafter(t, -INF, dtype=F)
        with np.errstate(invalid="ignore"):
            block = (ok & (t1 <= lo[:, None]) & (t2 > lo[:, None])).sum(axis=1)
        keep = np.isfinite(t) & (block >= 1)
        parts.append(_pack(rays[keep], rq, lo[keep], 1e9, tgt[keep]))
    return _cat(parts)


def _widened_face(arrays, rng, per):
    """the origin exactly on fl(bmin - rq) or fl(bmax + rq) of a random inner node, the direction's component on that axis +0 or -0:
    aabb_hit meets (face - origin) * (1 / +-0) = 0 * inf = NaN"""
    bmin, bmax = np.asarray(arrays["bmin"], dtype=F), np.asarray(arrays["bmax"], dtype=F)
    m = per
    node = rng.integers(0, bmin.shape[0], m)
    axis = rng.integers(0, 3, m)
    rq = np.array([0.5, 2.0, 0.25, 8.0], F)[rng.integers(0, 4, m)]
    wlo, whi = (bmin[node] - rq[:, None]).astype(F), (bmax[node] + rq[:, None]).astype(F)
    o = (wlo + rng.random((m, 3)).astype(F) * (whi - wlo)).astype(F)
    rows = np.arange(m)
    o[rows, axis] = np.where(rng.random(m) < 0.5, whi[rows, axis], wlo[rows, axis])
    d = rng.normal(size=(m, 3)).astype(F)
    d[rows, axis] = np.where(rng.random(m) < 0.5, F(0.0), NEG0)
    d[: m // 3, (axis[: m // 3] + 1) % 3] = NEG0
    return _pack(E._rays(o, d), rq, 0.0, 1e9, -1)


def _absorbed(arrays, rng, per):
    """rq = 1e8 and 1e9 absorb every coordinate of these scenes: every widened box is (-rq, rq), and from origins inside the scene and half
    a radius away from it every leaf is consulted"""
    L = np.asarray(arrays["L"], dtype=F)
    parts = []
    for rq in (F(1e8), F(1e9)):
        o_in = E._anchors(arrays, rng, per // 4)
        u = rng.normal(size=(per // 4, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o_out = (L[rng.integers(0, L.shape[0], per // 4), :3] + u * (0.5 * float(rq))).astype(F)
        o = np.concatenate([o_in, o_out])
        d = rng.normal(size=(o.shape[0], 3)).astype(F) * F(10.0) ** rng.integers(-2, 8, (o.shape[0], 1)).astype(F)
        hi = np.where(np.arange(o.shape[0]) % 2 == 0, F(1e9), F(1.0))
        parts.append(_pack(E._rays(o, d.astype(F)), rq, 0.0, hi, -1))
    return _cat(parts)


def _zero_radius(arrays, rng, per):
    """rays through the centres of the zero-radius spheres with rq in {0, -0, 1e-45, 1e-40}: R is zero or denormal, R * R is 0, the
    discriminant is rounding noise of either sign, and a contact's normal is (1 / R) (p - c) with 1 / R = inf"""
    L = np.asarray(arrays["L"], dtype=F)
    zero = np.nonzero(L[:, 6] == 0)[0]
    if zero.size == 0:
        return None
    m = 2 * per
    j = zero[rng.integers(0, zero.size, m)]
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = rng.uniform(1.0, 60.0, m)
    d = (u * 10.0 ** rng.uniform(-1, 1, (m, 1))).astype(F)
    o = (L[j, :3] - u * dist[:, None]).astype(F)
    rq = np.array([0.0, -0.0, 1e-45, 1e-40], F)[np.arange(m) % 4]
    return _pack(E._rays(o, d), rq, 0.0, 1e9, j)


def _spread(v, cap):
    n = v[0].shape[0]
    if cap is None or n <= cap:
        return v
    pick = np.unique(np.linspace(0, n - 1, cap).astype(np.int64))
    return tuple(a[pick] for a in v)


def _families(arrays, seed, per, cap):
    rng = np.random.default_rng([seed, 20261017])
    fam = {"ray_edges": _ray_edges(arrays, seed, per, cap)}
    fam.update(_root_families(arrays, rng, per))
    fam["grazing"] = _grazing(arrays, rng, per)
    fam["stationary"] = _stationary(arrays, rng, per)
    fam["ties"] = _ties(arrays, rng, per)
    fam["widened_face"] = _widened_face(arrays, rng, per)
    fam["absorbed"] = _absorbed(arrays, rng, per)
    fam["zero_radius"] = _zero_radius(arrays, rng, per)
    return {k: (v if k == "ray_edges" else _spread(v, cap)) for k, v in fam.items() if v is not None}


def sweep_families(arrays, seed=0, per=48, cap=None):
    """{name: (rays [m, 6], radius [m], t_min [m], t_max [m])}, float32, for the scene with BVH arrays `arrays`.  cap: at most that many
    queries of every family, spread evenly over it (of ray_edges: the first `cap` rays of every family of edge_rays.ray_families)"""
    return {k: v[:4] for k, v in _families(arrays, seed, per, cap).items()}


def sweep_targets(arrays, seed=0, per=48, cap=None):
    """{name: j [m] int64}: the sphere each query of sweep_families(arrays, seed, per, cap) was built against, -1 where it has none"""
    return {k: v[4] for k, v in _families(arrays, seed, per, cap).items()}


def joined(fam):
    """(rays, radius, t_min, t_max, label [m] index into list(fam)) of all the families in one"""
    parts = list(fam.values())
    label = np.concatenate([np.full(v[0].shape[0], i) for i, v in enumerate(parts)])
    return tuple(np.concatenate([v[i] for v in parts]) for i in range(4)) + (label,)
