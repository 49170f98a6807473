"""Edge inputs for the caller-ray queries (plain numpy): scenes where the BVH code goes wrong, rays whose arithmetic is delicate, and intervals
at the ends of the interval rule.

Scenes are `spheres7` arrays {pos.xyz, colour.rgb, radius} for `Context.scene_from_spheres` and `OracleScene("custom", ...)`; SCENES maps a name
to (spheres7, look_from, look_at, fov).  Ray families are small and named (`ray_families`), so that a failure says which one broke; every
family is built from the scene's own BVH arrays ({L, I}: OracleScene.arrays() / Prepared.bvh_arrays()).  `edge_intervals` gives per-ray
(t_min, t_max) for the ranged entries, labelled the same way.
"""
import numpy as np

from multi_hit_ref import _pair_roots
from ray_query_ref import RefScene

F = np.float32
NEG0 = F(-0.0)
DENORM = F(1e-40)
TINY_DENORM = F(-1e-45)         # the smallest negative denormal


def same_bits(got, want, what):
    """Assert got == want bit for bit, except that any NaN matches any NaN in the same position (the CPU's default NaN is not the GPU's).
    At least one finite value must be compared, so that NaN on both sides cannot hide a wholesale mismatch."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    assert want.size > 0, f"{what}: nothing compared"
    if want.dtype == F:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32)))
        assert np.isfinite(want).any(), f"{what}: no finite value compared"
    else:
        bad = got != want
    rows = np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0]
    assert rows.size == 0, f"{what}: {rows.size} rays differ, first {rows[:5]}"


# ---------------------------------------------------------------------------------------------------------------- scenes
def _colours(n):
    return np.linspace(0.3, 1.0, 3 * n, dtype=F).reshape(n, 3)


def _line(n, same):
    s = np.zeros((n, 7), F)
    s[:, 3:6] = _colours(n)
    s[:, 6] = 2.0
    if not same:
        s[:, 0] = np.arange(n, dtype=F) * 7.0 - 7.0
    return s


def _tall(dupes):
    # single-bit Morton codes make a 30-level chain; exact duplicates at the origin add log2(dupes) levels (height 41 at 1100)
    pts = [(1023.0, 1023.0, 1023.0)]
    for a in range(3):
        for m in range(10):
            p = [0.0, 0.0, 0.0]
            p[a] = float(2 ** m)
            pts.append(tuple(p))
    pts += [(0.0, 0.0, 0.0)] * dupes
    s = np.zeros((len(pts), 7), F)
    s[:, 0:3] = np.array(pts, F)
    s[:, 3:6] = _colours(len(pts))
    s[:, 6] = 0.4
    return s


def _nan_grid():
    # box faces on x = 0 and y = 0: an axis-aligned ray in those planes meets (face - origin) * inf = 0 * inf = NaN in aabb_hit
    g = np.array([-9.0, -3.0, 3.0, 9.0], F)
    xs, ys, zs = np.meshgrid(g, g, np.array([-6.0, 0.0, 6.0], F), indexing="ij")
    s = np.zeros((xs.size, 7), F)
    s[:, 0], s[:, 1], s[:, 2] = xs.ravel(), ys.ravel(), zs.ravel()
    s[:, 3:6] = np.linspace(0.4, 1.0, 3 * xs.size, dtype=F).reshape(-1, 3)
    s[:, 6] = 3.0
    return s


def _random_dupes():
    rng = np.random.default_rng(1234)
    n = 600
    s = np.zeros((n, 7), F)
    s[:, 0:3] = rng.uniform(-40, 40, (n, 3))
    s[:, 3:6] = rng.uniform(0.2, 1.0, (n, 3))
    s[:, 6] = rng.uniform(0.5, 4.0, n)
    s[100:140, 0:3] = s[0:40, 0:3]          # coincident centres, different colours / radii
    s[140:150] = s[40:50]                   # exact duplicates
    return s


def _overlap():
    # 40 large spheres that all contain the origin (a ray from there crosses each once: more than 32 crossings), and a chain of touching
    # unit spheres on the x axis at x = 20, 22, ..., 34: an axis-aligned ray along it meets sphere i's exit and sphere i+1's entry at the
    # same t, a tie in t between different spheres and different roots
    rng = np.random.default_rng(77)
    m = 40
    s = np.zeros((m + 8, 7), F)
    s[:m, 0:3] = rng.uniform(-3, 3, (m, 3)).astype(F)
    s[:m, 6] = rng.uniform(8.0, 16.0, m).astype(F)
    s[m:, 0] = 20.0 + 2.0 * np.arange(8, dtype=F)
    s[m:, 6] = 1.0
    s[:, 3:6] = _colours(m + 8)
    return s


SCENES = {
    "two_apart": (_line(2, same=False), (0.0, 3.0, 30.0), (0.0, 0.0, 0.0), 50.0),
    "two_same": (_line(2, same=True), (0.0, 3.0, 30.0), (0.0, 0.0, 0.0), 50.0),
    "same64": (_line(64, same=True), (0.0, 3.0, 30.0), (0.0, 0.0, 0.0), 50.0),
    "tall1100": (_tall(1100), (30.0, 20.0, 60.0), (0.0, 0.0, 0.0), 40.0),
    "nan_grid": (_nan_grid(), (0.0, 0.0, 40.0), (0.0, 0.0, 0.0), 40.0),
    "random600": (_random_dupes(), (5.0, 25.0, 70.0), (0.0, 0.0, 0.0), 60.0),
    "overlap": (_overlap(), (0.0, 5.0, 60.0), (0.0, 0.0, 0.0), 50.0),
}
TALL_HEIGHT = 41


# ---------------------------------------------------------------------------------------------------------------- rays
def _rays(o, d):
    o = np.asarray(o, dtype=F).reshape(-1, 3)
    d = np.asarray(d, dtype=F).reshape(-1, 3)
    o, d = np.broadcast_arrays(o, d)
    return np.concatenate([o, d], axis=1).astype(F)


def _anchors(arrays, rng, m):
    """m origins around the scene: sphere centres, the scene's centre, points inside its box and outside it."""
    L = np.asarray(arrays["L"], dtype=F)
    lo, hi = L[:, :3].min(0) - L[:, 6].max(), L[:, :3].max(0) + L[:, 6].max()
    ext = np.maximum(hi - lo, F(1))
    k = m // 4
    cen = L[rng.integers(0, L.shape[0], k), :3]
    mid = np.broadcast_to(((lo + hi) * F(0.5)).astype(F), (k, 3))
    inside = lo + rng.random((k, 3)) * ext
    outside = lo - ext + rng.random((m - 3 * k, 3)) * 3 * ext
    return np.concatenate([cen, mid, inside, outside]).astype(F)


def _axis_signed_zero_dirs():
    """One axis +-1, the other two +0.0 / -0.0 in every sign combination: 3 * 2 * 4 directions."""
    out = []
    for a in range(3):
        for s in (F(1), F(-1)):
            for z1 in (F(0.0), NEG0):
                for z2 in (F(0.0), NEG0):
                    d = [z1, z2]
                    d.insert(a, s)
                    out.append(d)
    return np.array(out, F)


def _search_root(pos, rad, axis, target, sign=1.0, steps=8, scales=96, which=(1, 2)):
    """Rays along +-axis toward a sphere whose root 1 or root 2 (`which`) equals `target` exactly, searched in sphere_hit's float32 arithmetic
    (multi_hit_ref._pair_roots): direction lengths from 0.5 to 3 and origins stepped a float32 ulp at a time from the nominal one.
    `rad` is the radius the roots are taken against (the sphere casts pass R = fl(r + rq)).  [m, 6] (m may be 0)."""
    e = np.zeros(3, F)
    e[axis] = F(sign)
    s = np.linspace(0.5, 3.0, scales).astype(F)
    found = []
    for which in which:
        dist = (F(rad) + F(target) * s) if which == 1 else (F(target) * s - F(rad))   # centre - origin along the ray
        o = (pos[None, :] - e[None, :] * dist[:, None]).astype(F)
        o = np.repeat(o, 2 * steps + 1, axis=0)
        v = o[:, axis].reshape(scales, 2 * steps + 1)
        for i in range(steps):
            v[:, steps + 1 + i] = np.nextafter(v[:, steps + i], F(np.inf), dtype=F)
            v[:, steps - 1 - i] = np.nextafter(v[:, steps - i], F(-np.inf), dtype=F)
        o[:, axis] = v.reshape(-1)
        d = (np.repeat(s, 2 * steps + 1)[:, None] * e[None, :]).astype(F)
        r1, r2, ok = _pair_roots(np.broadcast_to(pos, o.shape).astype(F), np.full(o.shape[0], rad, F), o, d)
        hit = ok & ((r1 if which == 1 else r2) == F(target))
        found.append(_rays(o[hit], d[hit]))
    return np.concatenate(found) if found else np.zeros((0, 6), F)


def ray_families(arrays, seed=0, per=48):
    """{name: [m, 6] float32 rays} for the scene with BVH arrays `arrays`.  On the edge scenes every family is non-empty
    (test_ray_edges_cpu checks); on others root_at_eps may be."""
    rng = np.random.default_rng(seed)
    L = np.asarray(arrays["L"], dtype=F)
    bmin, bmax = np.asarray(arrays["bmin"], dtype=F), np.asarray(arrays["bmax"], dtype=F)
    n = L.shape[0]
    fam = {}

    # axis-aligned rays with +-0.0 in every sign combination, from origins that sit inside the slabs of the zero axes
    dirs = _axis_signed_zero_dirs()
    o = _anchors(arrays, rng, per)
    fam["axis_signed_zero"] = _rays(np.repeat(o, len(dirs), axis=0), np.tile(dirs, (per, 1)))

    # the zero direction
    o = _anchors(arrays, rng, per // 2)
    fam["zero_dir"] = np.concatenate([_rays(o, np.zeros(3, F)), _rays(o, np.full(3, NEG0))])

    # denormal components next to ordinary ones
    o = _anchors(arrays, rng, per)
    d = rng.normal(size=(per, 3)).astype(F)
    cols = rng.integers(0, 3, per)
    d[np.arange(per), cols] = np.where(rng.random(per) < 0.5, DENORM, TINY_DENORM)
    d[: per // 4] = np.where(rng.random((per // 4, 3)) < 0.5, DENORM, TINY_DENORM)
    fam["denormal"] = _rays(o, d)

    # |d| ~ 1e-22 with |o - p| ~ 1e3: a = d.d underflows (to 0 or a denormal) while b = oc.d does not
    tgt = L[rng.integers(0, n, per), :3]
    u = rng.normal(size=(per, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (tgt - 1e3 * u).astype(F)
    fam["tiny_dir"] = _rays(o, (u * 1e-22).astype(F))

    # |d| ~ 1e20: a overflows to inf
    o = _anchors(arrays, rng, per)
    tgt = L[rng.integers(0, n, per), :3]
    v = (tgt - o).astype(np.float64)
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)
    v[: per // 4] = rng.normal(size=(per // 4, 3))
    fam["huge_dir"] = _rays(o, (v * 1e20).astype(F))

    # NaN, +inf or -inf in exactly one component of o or d
    base = np.concatenate([_anchors(arrays, rng, 6 * 3), rng.normal(size=(18, 3)).astype(F)], axis=1).astype(F)
    rows = []
    for c in range(6):
        for i, bad in enumerate((np.nan, np.inf, -np.inf)):
            r = base[3 * c + i].copy()
            r[c] = F(bad)
            rows.append(r)
    fam["non_finite"] = np.array(rows, F)

    # origins exactly on a box face, with a zero direction component on that axis (the other two random, one of them sometimes -0.0)
    ni = bmin.shape[0]
    node = rng.integers(0, ni, per)
    axis = rng.integers(0, 3, per)
    use_max = rng.random(per) < 0.5
    o = (bmin[node] + rng.random((per, 3)).astype(F) * (bmax[node] - bmin[node])).astype(F)
    face = np.where(use_max, bmax[node, axis], bmin[node, axis])
    o[np.arange(per), axis] = face
    d = rng.normal(size=(per, 3)).astype(F)
    d[np.arange(per), axis] = np.where(rng.random(per) < 0.5, F(0.0), NEG0)
    d[: per // 3, (axis[: per // 3] + 1) % 3] = NEG0
    fam["box_face"] = _rays(o, d)

    # origins at a sphere centre and on its surface (centre + radius along an axis)
    j = rng.integers(0, n, per)
    ax = rng.integers(0, 3, per)
    surf = L[j, :3].copy()
    surf[np.arange(per), ax] += np.where(rng.random(per) < 0.5, L[j, 6], -L[j, 6])
    d = rng.normal(size=(2 * per, 3)).astype(F)
    d[per: per + per // 2] = 0
    d[np.arange(per, per + per // 2), ax[: per // 2]] = np.where(rng.random(per // 2) < 0.5, F(1), F(-1))
    fam["centre_surface"] = _rays(np.concatenate([L[j, :3], surf]), d)

    # exactly tangent rays: axis-aligned, offset by the radius, so that b * b == a * c (disc == 0) when centre and radius are integers
    j = rng.integers(0, n, per)
    ax = rng.integers(0, 3, per)
    perp = (ax + rng.integers(1, 3, per)) % 3
    sgn = np.where(rng.random(per) < 0.5, F(1), F(-1))
    o = L[j, :3].copy()
    o[np.arange(per), ax] -= sgn * F(50.0)
    o[np.arange(per), perp] += np.where(rng.random(per) < 0.5, L[j, 6], -L[j, 6])
    d = np.zeros((per, 3), F)
    d[np.arange(per), ax] = sgn
    fam["tangent"] = _rays(o, d)

    # rays whose root equals np.float32(0.1) (kEps, the fold's t_min), found by search in float32
    found = []
    for j in rng.permutation(n)[:6]:
        for axis in range(3):
            for sign in (1.0, -1.0):
                found.append(_search_root(L[j, :3], L[j, 6], axis, F(0.1), sign))
    r = np.concatenate(found)
    fam["root_at_eps"] = r[rng.permutation(r.shape[0])[: 2 * per]]

    return fam


def tangent_disc(arrays, rays):
    """[m] bool: the ray is exactly tangent to some sphere, b * b - a * c == 0 in sphere_hit's arithmetic."""
    ref = RefScene.__new__(RefScene)
    L = np.asarray(arrays["L"], dtype=F)
    ref.pos, ref.rad = L[:, :3], L[:, 6]
    o, d = rays[:, :3], rays[:, 3:]
    ocx, ocy, ocz = (o[:, i:i + 1] - ref.pos[None, :, i] for i in range(3))
    dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    with np.errstate(all="ignore"):
        a = (dx * dx + dy * dy) + dz * dz
        b = (ocx * dx + ocy * dy) + ocz * dz
        c = ((ocx * ocx + ocy * ocy) + ocz * ocz) - ref.rad[None, :] * ref.rad[None, :]
        disc = b * b - a * c
    return (disc == 0).any(axis=1)


# ---------------------------------------------------------------------------------------------------------------- intervals
def roots_of(arrays, rays):
    """(root 1, root 2) of each ray's nearest sphere with a positive discriminant and finite roots (NaN where there is none): bounds equal
    to a ray's own roots."""
    L = np.asarray(arrays["L"], dtype=F)
    ref = RefScene.__new__(RefScene)
    ref.pos, ref.rad = L[:, :3], L[:, 6]
    r1, r2, ok = RefScene.roots(ref, rays[:, :3], rays[:, 3:])
    with np.errstate(invalid="ignore"):
        good = ok & np.isfinite(r1) & np.isfinite(r2) & (r1 >= 0) & (r2 <= F(1e9))
    key = np.where(good, r1, F(np.inf))
    j = np.argmin(key, axis=1)
    rows = np.arange(rays.shape[0])
    have = good[rows, j]
    return np.where(have, r1[rows, j], F(np.nan)).astype(F), np.where(have, r2[rows, j], F(np.nan)).astype(F)


INTERVAL_KINDS = ("neg0_neg0", "neg0_x", "x_x", "full", "past_1e9", "denormal_lo", "own_r1_r2", "own_r1_max", "zero_own_r1",
                  "own_r2_r2")


def edge_intervals(arrays, rays, seed=0):
    """(t_min [m], t_max [m], kind [m] index into INTERVAL_KINDS): each ray one of the edge intervals, in turn.  Bounds equal to the ray's
    own roots fall back to (0, 1e9) for a ray without finite roots."""
    m = rays.shape[0]
    rng = np.random.default_rng(seed)
    r1, r2 = roots_of(arrays, rays)
    x = rng.uniform(0.05, 60.0, m).astype(F)
    kind = (np.arange(m) + rng.integers(0, len(INTERVAL_KINDS))) % len(INTERVAL_KINDS)
    lo = np.zeros(m, F)
    hi = np.full(m, F(1e9))
    past = np.nextafter(F(1e9), F(np.inf), dtype=F)
    has = np.isfinite(r1)
    for k, name in enumerate(INTERVAL_KINDS):
        s = kind == k
        if name == "neg0_neg0":
            lo[s], hi[s] = NEG0, NEG0
        elif name == "neg0_x":
            lo[s], hi[s] = NEG0, x[s]
        elif name == "x_x":
            lo[s], hi[s] = x[s], x[s]
        elif name == "full":
            lo[s], hi[s] = 0.0, 1e9
        elif name == "past_1e9":
            lo[s], hi[s] = 0.0, past
        elif name == "denormal_lo":
            lo[s], hi[s] = F(1e-45), 1e9
        else:
            t = s & has
            if name == "own_r1_r2":
                lo[t], hi[t] = r1[t], r2[t]
            elif name == "own_r1_max":
                lo[t], hi[t] = r1[t], 1e9
            elif name == "zero_own_r1":
                lo[t], hi[t] = 0.0, r1[t]
            else:
                lo[t], hi[t] = r2[t], r2[t]
    return lo, hi, kind
