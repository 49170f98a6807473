"""CPU checks of the sphere casts: the restatement (sweep_ref.py) against the multi-hit and range-query restatements, its dense form against its
walk form, its tree-defined answer against the brute force over all spheres, the per-sphere rule against the C++ arithmetic
(build/sweep_check runs query_core.h's sweep_contact), and the loader's symbols and Python signatures."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import interval_ref as V
import multi_hit_ref as M
import occlusion_ref as X
import oracle_lib as O
import proximity_ref as P
import ray_query_ref as Q
import sweep_ref as S
import within_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [("rgbbox", {}, 17), ("irreg", {}, 29), ("floor", {"n": 37, "k": 222.0}, 41)]
NRAYS = 1024
F = np.float32


@pytest.fixture(scope="module", params=SCENES, ids=[s[0] for s in SCENES])
def scene(request):
    name, kw, seed = request.param
    arr = O.OracleScene(name, **kw).arrays()
    return Q.RefScene(arr), X.seeded_rays(arr, NRAYS, seed), arr


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same(got, want, what):
    for name, g, w in zip(("count", "index", "start", "hit7"), got, want):
        assert g.shape == w.shape, (what, name)
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} queries, first {bad[:5]}"


def _scale_radius(arr):
    """a scene-scale query radius: the median sphere radius"""
    return float(np.median(arr["L"][:, 6]))


@pytest.mark.parametrize("t_min,t_max", [(0.0, 1e9), (0.1, 1e9), (0.5, 30.0), (7.0, 7.0)])
def test_radius_zero_against_multi_hit(scene, t_min, t_max):
    # with rq = 0 the consulted leaves are multi-hit's, the entry contacts are its root-1 crossings (same t, same j), and there is one overlap
    # at the start for every visited sphere with t1 <= t_min < t2 (t_min < t_max), at tau = t_min
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    mc, mi, mr, mh = M.multi_hit(ref, o, d, t_min, t_max, M.KMAX)
    for radius in (0.0, -0.0):
        count, index, start, hit = S.sweep(ref, o, d, radius, t_min, t_max, S.KMAX)
        fits = np.nonzero(mc <= M.KMAX)[0]
        assert fits.size > NRAYS // 2
        entries = starts = 0
        for s in range(0, NRAYS, 256):
            oo, dd = o[s:s + 256], d[s:s + 256]
            r1, r2, pos = ref.roots(oo, dd)
            with np.errstate(invalid="ignore"):
                over = ref.visited(oo, dd, F(t_min), F(t_max)) & pos & (r1 <= F(t_min)) & (r2 > F(t_min)) & (F(t_min) < F(t_max))
            for i in fits[(fits >= s) & (fits < s + 256)]:
                m = int(mc[i])
                first = mr[i, :m] == 1
                want = [(float(F(t_min) + F(0)), int(j), 1) for j in np.nonzero(over[i - s])[0]]
                want += [(float(t), int(j), 0) for t, j in zip(mh[i, :m, 0][first], mi[i, :m][first])]
                want.sort()
                assert int(count[i]) == len(want), (i, radius)
                n = min(len(want), S.KMAX)
                got = list(zip(hit[i, :n, 0].tolist(), index[i, :n].tolist(), start[i, :n].tolist()))
                assert got == want[:n], (i, radius)
                entries += int(first.sum())
                starts += len(want) - int(first.sum())
        if t_min < t_max:
            assert entries > 0 and (starts > 0 or t_min == 0.0), (entries, starts)
        else:
            assert not count.any()


@pytest.mark.parametrize("t_min,t_max", [(0.0, 1.0), (0.0, 1e9), (0.1, 30.0), (3.0, 3.0)])
def test_walk_equals_dense(scene, t_min, t_max):
    ref, rays, arr = scene
    o, d = rays[:, :3], rays[:, 3:]
    rng = np.random.default_rng(3)
    ex = rng.integers(-2, ref.n + 2, NRAYS)
    for radius in (0.0, _scale_radius(arr), 250.0):
        for k in (1, 5, S.KMAX):
            _same(S.sweep_walk(arr, o, d, radius, t_min, t_max, k), S.sweep(ref, o, d, radius, t_min, t_max, k), (radius, t_min, t_max, k))
        _same(S.sweep_walk(arr, o, d, radius, t_min, t_max, 8, ex), S.sweep(ref, o, d, radius, t_min, t_max, 8, ex), ("exclude", radius))
    lo, hi, _ = V.mixed_intervals(NRAYS, seed=5)
    lo[::97] = np.nan
    rq = rng.uniform(0.0, 3.0, NRAYS).astype(F)
    rq[::89] = np.nan
    rq[5::89] = -1.0
    _same(S.sweep_walk(arr, o, d, rq, lo, hi, 8, ex), S.sweep(ref, o, d, rq, lo, hi, 8, ex), "per-query")


def test_prefix_in_k_and_order(scene):
    ref, rays, arr = scene
    o, d = rays[:, :3], rays[:, 3:]
    for radius, t_min in ((0.0, 0.0), (_scale_radius(arr), 0.25)):
        full = S.sweep(ref, o, d, radius, t_min, 1e9, S.KMAX)
        assert full[0].max() > 1
        for k in (1, 3, 8):
            part = S.sweep(ref, o, d, radius, t_min, 1e9, k)
            assert np.array_equal(part[0], full[0])
            for a, b in zip(part[1:], full[1:]):
                assert np.array_equal(_bits(a), _bits(b[:, :k])), k
        cnt, idx, start, hit = full
        filled = np.arange(S.KMAX)[None, :] < np.minimum(cnt, S.KMAX)[:, None]
        assert np.array_equal(idx >= 0, filled) and not hit[~filled].any() and not start[~filled].any()
        # an overlap at the start is at tau = t_min, an entry contact inside the interval; a sphere is listed once; the order is (tau, j)
        assert (hit[filled & (start == 1), 0] == F(t_min)).all() and (hit[filled & (start == 0), 0] > F(t_min)).all()
        for i in np.nonzero(cnt > 1)[0][:200]:
            m = min(int(cnt[i]), S.KMAX)
            keys = list(zip(hit[i, :m, 0].tolist(), idx[i, :m].tolist()))
            assert keys == sorted(keys) and len(set(idx[i, :m].tolist())) == m, i


def test_invalid_queries_miss_and_buckets(scene):
    ref, rays, arr = scene
    o, d = rays[:, :3], rays[:, 3:]
    r0 = _scale_radius(arr)
    lo, hi, rq = np.full(NRAYS, 0.0, F), np.full(NRAYS, 1e9, F), np.full(NRAYS, r0, F)
    bad = [(np.nan, 1.0, r0), (0.0, np.nan, r0), (0.0, np.inf, r0), (-1.0, 1.0, r0), (2.0, 1.0, r0), (0.0, 2e9, r0),
           (0.0, 1e9, np.nan), (0.0, 1e9, np.inf), (0.0, 1e9, -1.0), (0.0, 1e9, 2e9), (0.0, 1e9, -np.inf)]
    where = np.arange(len(bad)) * 37 + 3
    for i, (a, b, c) in zip(where, bad):
        lo[i], hi[i], rq[i] = a, b, c
    ok = S.query_ok(lo, hi, rq)
    assert ok.sum() == NRAYS - len(bad)
    cnt, idx, start, hit = S.sweep(ref, o, d, rq, lo, hi, 4)
    full = S.sweep(ref, o, d, r0, 0.0, 1e9, 4)
    assert full[0][where].any()
    assert not cnt[where].any() and (idx[where] == -1).all() and not start[where].any() and not hit[where].any()
    for g, w in zip((cnt, idx, start, hit), full):
        assert np.array_equal(_bits(g[ok]), _bits(w[ok]))
    # -0.0 is a valid radius and a valid bound, and behaves as 0.0
    _same(S.sweep(ref, o, d, np.full(NRAYS, -0.0, F), np.full(NRAYS, -0.0, F), 1e9, 4), S.sweep(ref, o, d, 0.0, 0.0, 1e9, 4), "-0.0")
    # mixed per-query intervals and radii: bucket by bucket the scalar form
    lo, hi, b1 = V.mixed_intervals(NRAYS, seed=7)
    radii = np.asarray([0.0, r0, 40.0], F)
    b2 = np.random.default_rng(8).integers(0, 3, NRAYS)
    got = S.sweep(ref, o, d, radii[b2], lo, hi, 8)
    assert got[0].any() and not got[0].all()
    for a in np.unique(b1):
        for b in range(3):
            m = (b1 == a) & (b2 == b)
            _same(tuple(g[m] for g in got), S.sweep(ref, o[m], d[m], radii[b], lo[m][0], hi[m][0], 8), (a, b))


def test_exclude(scene):
    # excluding sphere e from a query removes exactly that sphere's contact: the un-excluded answer with k + 1 slots, minus e
    ref, rays, arr = scene
    o, d = rays[:, :3], rays[:, 3:]
    r0, k = _scale_radius(arr), 6
    cnt, idx, start, hit = S.sweep(ref, o, d, r0, 0.0, 1e9, k + 1)
    ex = np.where(cnt > 0, idx[:, 0], 5).astype(np.int64)
    ex[::3] = np.where(cnt[::3] > 1, idx[::3, 1], ex[::3])
    ex[::11] = -1
    ex[1::11] = ref.n
    got = S.sweep(ref, o, d, r0, 0.0, 1e9, k, ex)
    listed = (idx == ex[:, None]) & (idx >= 0)
    assert listed.any(axis=1).sum() > NRAYS // 4
    assert not ((got[1] == ex[:, None]) & (got[1] >= 0)).any()
    for i in range(NRAYS):
        keep = ~listed[i]
        assert got[0][i] == cnt[i] - (1 if listed[i].any() else 0) or cnt[i] > k + 1, i
        assert np.array_equal(got[1][i], idx[i][keep][:k]) and np.array_equal(_bits(got[3][i]), _bits(hit[i][keep][:k])), i
        assert np.array_equal(got[2][i], start[i][keep][:k]), i


def _overlap_check(ref, L, o, d, rq, t_min):
    """(removed, compared, mismatches): the overlaps at the start of every query against within_ref's selection at p = o + t_min d, bound rq,
    after removing the pairs whose two float32 predicates may legitimately differ.

    The rule.  within selects j iff gap = |p - c| - r <= rq, with p = fl(o + t_min d).  The sweep reports j iff t1 <= t_min < t2, the roots of
    the ray against (c, R = r + rq).  By E1 (lane_core.h) the point at a computed root lies within 2^-18 (D^2 / R + R) of the
    sphere (c, R), D = |o - c|; p itself and the gap carry a few ulps of the coordinates.  A pair is removed when
        |gap - rq| <= 2^-17 (D^2 / R + R) + 2^-20 (max|p| + max|c| + R):
    twice E1's distance plus 8 ulps of the coordinate scale.  Everywhere else the two predicates must agree exactly."""
    n = o.shape[0]
    with np.errstate(all="ignore"):
        p = (o + F(t_min) * d).astype(F)
    kinds = S.contact_kinds(ref, o, d, rq, t_min, 1e9)
    removed = compared = 0
    bad = []
    for s in range(0, n, 256):
        e = min(n, s + 256)
        gap = P.gaps(L, p[s:e]).astype(np.float64)
        R = (L[None, :, 6] + F(rq)).astype(np.float64)
        D2 = ((o[s:e, None, :].astype(np.float64) - L[None, :, :3]) ** 2).sum(axis=2)
        scale = np.abs(p[s:e]).max(axis=1)[:, None] + np.abs(L[:, :3]).max(axis=1)[None, :] + R
        with np.errstate(all="ignore"):
            tol = 2.0 ** -17 * (D2 / R + R) + 2.0 ** -20 * scale
        near = ~(np.abs(gap - float(F(rq))) > tol)
        sel = gap <= float(F(rq))
        got = kinds[s:e] == 2
        removed += int(near.sum())
        compared += int((~near).sum())
        r, c = np.nonzero((sel != got) & ~near)
        bad += [(int(i) + s, int(j)) for i, j in zip(r, c)]
    return removed, compared, bad, int((kinds == 2).sum())


def test_start_overlaps_against_within(scene):
    ref, rays, arr = scene
    L = np.asarray(arr["L"], dtype=F)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    r0 = _scale_radius(arr)
    total = 0
    for rq, t_min in ((0.0, 0.0), (r0, 0.0), (r0, 0.5), (40.0, 2.0)):
        removed, compared, bad, overlaps = _overlap_check(ref, L, o, d, rq, t_min)
        share = removed / (removed + compared)
        print(f"rq={rq} t_min={t_min}: {overlaps} overlaps at the start, removed share {share:.3e} ({removed} of {removed + compared} pairs)")
        assert not bad, f"rq={rq} t_min={t_min}: {len(bad)} pairs differ outside the band (removed share {share:.3e}), first {bad[:5]}"
        assert share < 1e-2, share
        total += overlaps
        # the whole rows agree with within()'s where no pair of the query was removed: count of start overlaps == the row's length
    assert total > 0
    # the chosen input on which nothing is removed: queries at rest positions on a coarse lattice (every coordinate a multiple of 1/4, so
    # o - c is exact wherever c is one too) with a radius far from every gap's rounding
    rng = np.random.default_rng(2)
    lo, hi = L[:, :3].min(0), L[:, :3].max(0)
    o2 = (np.round(rng.uniform(lo, hi, (256, 3)) * 4) / 4).astype(F)
    d2 = rng.normal(size=(256, 3)).astype(F)
    removed, compared, bad, overlaps = _overlap_check(ref, L, o2, d2, 0.7109375, 0.0)
    assert removed == 0 and not bad, f"lattice input: removed share {removed / (removed + compared):.3e}, {len(bad)} pairs differ"
    # and there the count of overlaps at the start IS the range query's row length, row by row
    off, idx, _ = W.within(L, o2, 0.7109375)
    kinds = S.contact_kinds(ref, o2, d2, 0.7109375, 0.0, 1e9)
    assert np.array_equal((kinds == 2).sum(axis=1), np.diff(off))
    assert np.array_equal(np.nonzero(kinds == 2)[1], idx)


def test_tree_answer_against_brute_force(scene):
    # the answer is defined by the tree: the brute force (the same per-sphere rule over ALL spheres) may only have MORE contacts, and each
    # extra one is a leaf the walk does not consult (some widened ancestor box fails aabb_hit).  An explained difference, not a tolerance.
    ref, rays, arr = scene
    o, d = rays[:, :3], rays[:, 3:]
    for radius, t_min, t_max in ((0.0, 0.0, 1e9), (_scale_radius(arr), 0.0, 1.0), (40.0, 0.1, 30.0)):
        tree = S.contact_kinds(ref, o, d, radius, t_min, t_max)
        brute = S.contact_kinds(ref, o, d, radius, t_min, t_max, boxes=False)
        seen = S.consulted(ref, o, d, radius, t_min, t_max)
        diff = tree != brute
        print(f"radius={radius} ({t_min}, {t_max}): {int(diff.sum())} of {int((brute > 0).sum())} brute-force contacts are not in the tree's answer "
              f"({diff.any(axis=1).mean():.3%} of the queries)")
        assert not (tree[diff] != 0).any(), "the tree's answer has a contact the brute force has not"
        assert not seen[diff].any(), "a differing contact is on a consulted leaf"
        assert np.array_equal(tree[seen], brute[seen])
        # and the listed answers agree on every query without such a leaf
        same = ~diff.any(axis=1)
        a, b = S.sweep(ref, o[same], d[same], radius, t_min, t_max, 8), S.sweep_brute(ref, o[same], d[same], radius, t_min, t_max, 8)
        _same(a, b, radius)


def rule_case_set(seed=20261017, m=4000):
    """(m', 13) float32 cases for build/sweep_check: random ones, grazing rays, origins inside and on the surface of the swept sphere, radius 0 on
    either side and on both, NaN and inf components, empty and degenerate intervals"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50, 50, (m, 3))
    r = rng.uniform(0.1, 5.0, m)
    rq = rng.uniform(0.0, 5.0, m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(m, 3)))
    w /= np.linalg.norm(w, axis=1)[:, None]
    speed = 10.0 ** rng.uniform(-2, 2, m)
    dist = rng.uniform(0.0, 30.0, m)
    kind = rng.integers(0, 8, m)
    R = r + rq
    off = np.where(kind == 1, R * (1 + rng.choice([-1e-7, 0.0, 1e-7, 1e-4, -1e-4], m)), rng.uniform(0, 1.5, m) * R)   # 1: grazing
    o = c - u * dist[:, None] + w * off[:, None]
    inside = kind == 2
    o[inside] = (c + u * (rng.uniform(0, 1, m) * R)[:, None])[inside]                                                  # 2: starts inside
    surf = kind == 3
    o[surf] = (c + u * R[:, None])[surf]                                                                             # 3: starts on the surface
    d = u * speed[:, None]
    d[surf & (rng.random(m) < 0.5)] *= -1
    r[kind == 4] = 0.0
    rq[kind == 5] = 0.0
    r[kind == 6] = 0.0
    rq[kind == 6] = 0.0
    lo = np.where(rng.random(m) < 0.5, 0.0, rng.uniform(0, 2, m) * dist / speed)
    hi = np.where(rng.random(m) < 0.3, 1e9, lo + rng.uniform(0, 3, m) * (dist + R) / speed)
    hi[::53] = lo[::53]
    cases = np.concatenate([o, d, c, r[:, None], rq[:, None], lo[:, None], hi[:, None]], axis=1).astype(F)
    special = cases[: 13 * 12].copy()
    for i in range(13 * 12):
        special[i, i % 13] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 1e-30, 3e38, np.nan, 0.0, np.inf][i // 13]
    lo0 = cases[200:400].copy()
    lo0[:, 11] = -0.0
    lo0[:, 0:3] = lo0[:, 6:9]                      # centred on the sphere: an overlap at the start, reported at +0.0
    return np.concatenate([cases, special, lo0]).astype(F)


def test_sweep_check_agrees_with_the_restatement(tmp_path):
    exe = os.path.join(ROOT, "build", "sweep_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/sweep_check"], check=True, capture_output=True)
    cases = rule_case_set()
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    cases.tofile(src)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, dtype=np.uint32).reshape(-1, 2)
    assert got.shape[0] == cases.shape[0]
    kind, tau = S.rule_cases(cases[:, 0:3], cases[:, 3:6], cases[:, 6:9], cases[:, 9], cases[:, 10], cases[:, 11], cases[:, 12])
    bad = np.nonzero((got[:, 0] != kind) | (got[:, 1] != _bits(tau)))[0]
    assert bad.size == 0, f"{bad.size} cases differ, first {bad[:5]}: {cases[bad[:3]]}"
    # the case set reaches every outcome, and an overlap at a -0.0 start is reported at +0.0
    assert all((kind == v).sum() > 100 for v in (0, 1, 2)), np.bincount(kind)
    neg0 = (_bits(cases[:, 11]) == 0x80000000) & (kind == 2)
    assert neg0.sum() > 50 and (got[neg0, 1] == 0).all()


def test_library_exports_sweep():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_sweep_spheres", "rt_sweep_spheres_ranged"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_sweep_spheres.argtypes) == 12
    assert len(_lib.lib.rt_sweep_spheres_ranged.argtypes) == 13
    for name in ("sweep_spheres", "sweep_spheres_into", "sweep_spheres_ranged_into"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.sweep_spheres).parameters) == ["prepared", "rays", "radius", "k", "t_min", "t_max", "exclude"]
    sig = inspect.signature(R.sweep_spheres)
    assert (sig.parameters["k"].default, sig.parameters["t_min"].default, sig.parameters["t_max"].default, sig.parameters["exclude"].default) \
        == (1, 0.0, 1.0, None)
    assert list(inspect.signature(R.sweep_spheres_into).parameters) == [
        "rays_ptr", "n", "prepared", "radius", "k", "count_ptr", "index_ptr", "start_ptr", "hit_ptr", "t_min", "t_max"]
    assert list(inspect.signature(R.sweep_spheres_ranged_into).parameters) == [
        "rays_ptr", "n", "prepared", "radius_ptr", "t_min_ptr", "t_max_ptr", "k", "count_ptr", "index_ptr", "start_ptr", "hit_ptr", "exclude_ptr"]


def test_header_declares_sweep():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_sweep_spheres(", "rt_sweep_spheres_ranged(", "family=sweep k="):
        assert sym in h, sym
