"""CPU checks of the multi-hit query: the restatement (multi_hit_ref.py) against the occlusion, objs_hit and per-ray interval restatements,
and the loader's symbols and Python signatures."""
import inspect

import numpy as np
import pytest

import interval_ref as V
import multi_hit_ref as M
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q

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


@pytest.mark.parametrize("t_min,t_max", [(0.0, 1e9), (0.1, 1e9), (0.5, 30.0), (0.0, 0.05), (7.0, 7.0)])
def test_count_is_occlusion(scene, t_min, t_max):
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    count, index, root, hit = M.multi_hit(ref, o, d, t_min, t_max, 4)
    occ = X.occluded(ref, o, d, t_min, t_max)
    assert np.array_equal(count > 0, occ)
    if t_min == t_max:
        assert not count.any()
    # a slot is filled iff it is below the count, and a filled slot's t lies inside the interval
    filled = np.arange(4)[None, :] < np.minimum(count, 4)[:, None]
    assert np.array_equal(index >= 0, filled) and np.array_equal(root > 0, filled)
    assert ((hit[filled, 0] > F(t_min)) & (hit[filled, 0] < F(t_max))).all()
    assert not hit[~filled].any() and (root[filled] <= 2).all()


@pytest.mark.parametrize("t_max", [1e9, 30.0])
def test_first_crossing_is_objs_hit(scene, t_max):
    # at t_min = 0.1 crossing 0 is objs_hit's winner (same index, same t) whenever objs_hit hits and its root is below 2^23 (the
    # re-hit over (0.1, t + 1) then returns the fold's root); the hit records agree bit for bit there too
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    idx, hit = ref.objs_hit(o, d, F(0.1), F(t_max))
    count, index, root, mh = M.multi_hit(ref, o, d, 0.1, t_max, 1)
    small = (idx >= 0) & (hit[:, 0] < 2.0 ** 23)
    assert small.sum() > NRAYS // 10
    assert (count[small] > 0).all()
    assert np.array_equal(index[small, 0], idx[small])
    assert np.array_equal(_bits(mh[small, 0]), _bits(hit[small]))


def test_prefix_in_k(scene):
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    full = M.multi_hit(ref, o, d, 0.0, 1e9, M.KMAX)
    assert full[0].max() > 1
    for k in (1, 3, 8):
        part = M.multi_hit(ref, o, d, 0.0, 1e9, k)
        assert np.array_equal(part[0], full[0])
        for a, b in zip(part[1:], full[1:]):
            assert np.array_equal(_bits(a), _bits(b[:, :k])), k
    # the kept crossings are in (t, j, root) order
    cnt, idx, root, hit = full
    for i in np.nonzero(cnt > 1)[0][:200]:
        m = min(int(cnt[i]), M.KMAX)
        keys = list(zip(hit[i, :m, 0].tolist(), idx[i, :m].tolist(), root[i, :m].tolist()))
        assert keys == sorted(keys), i


def test_both_roots_of_a_sphere(scene):
    # a ray through a sphere crosses it twice, entry (root 1) before exit (root 2), unless an end of the interval cuts one off
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    cnt, idx, root, hit = M.multi_hit(ref, o, d, 0.0, 1e9, M.KMAX)
    pairs = 0
    for i in np.nonzero((cnt >= 2) & (cnt <= M.KMAX))[0]:
        m = int(cnt[i])
        for j in np.unique(idx[i, :m]):
            rj = root[i, :m][idx[i, :m] == j]
            if rj.size == 2:
                assert list(rj) == [1, 2], (i, j)
                pairs += 1
    assert pairs > 0


def test_mixed_intervals_equal_buckets(scene):
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    lo, hi, k = V.mixed_intervals(NRAYS, seed=7)
    got = M.multi_hit(ref, o, d, lo, hi, 8)
    assert got[0].any() and not got[0].all()
    for b in np.unique(k):
        m = k == b
        want = M.multi_hit(ref, o[m], d[m], lo[m][0], hi[m][0], 8)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g[m]), _bits(w)), b


def test_invalid_intervals_miss(scene):
    ref, rays, _ = scene
    o, d = rays[:, :3], rays[:, 3:]
    lo, hi = np.full(NRAYS, 0.0, F), np.full(NRAYS, 1e9, F)
    bad = [(np.nan, 1.0), (0.0, np.nan), (0.0, np.inf), (-np.inf, 1.0), (-1.0, 1.0), (2.0, 1.0), (0.0, 2e9), (np.inf, np.inf)]
    where = np.arange(len(bad)) * 37 + 3
    for i, (a, b) in zip(where, bad):
        lo[i], hi[i] = a, b
    ok = V.interval_ok(lo, hi)
    cnt, idx, root, hit = M.multi_hit(ref, o, d, lo, hi, 4)
    full = M.multi_hit(ref, o, d, 0.0, 1e9, 4)
    assert full[0][where].any()          # the rays the rule turns into misses were not misses
    assert not cnt[where].any() and (idx[where] == -1).all() and not root[where].any() and not hit[where].any()
    for g, w in zip((cnt, idx, root, hit), full):
        assert np.array_equal(_bits(g[ok]), _bits(w[ok]))
    # -0.0 is a valid bound and behaves as 0.0
    neg = M.multi_hit(ref, o, d, np.full(NRAYS, -0.0, F), np.full(NRAYS, 1e9, F), 4)
    for g, w in zip(neg, full):
        assert np.array_equal(_bits(g), _bits(w))


@pytest.mark.parametrize("t_min,t_max", [(0.0, 1e9), (0.1, 30.0), (3.0, 3.0)])
def test_walk_equals_dense(scene, t_min, t_max):
    # the breadth-first form (for scenes too large for the dense one) gives the same answer, bit for bit
    ref, rays, arr = scene
    o, d = rays[:, :3], rays[:, 3:]
    for k in (1, 5, M.KMAX):
        for g, w in zip(M.multi_hit_walk(arr, o, d, t_min, t_max, k), M.multi_hit(ref, o, d, t_min, t_max, k)):
            assert np.array_equal(_bits(g), _bits(w)), (t_min, t_max, k)
    lo, hi, _ = V.mixed_intervals(NRAYS, seed=5)
    lo[::97] = np.nan
    for g, w in zip(M.multi_hit_walk(arr, o, d, lo, hi, 8), M.multi_hit(ref, o, d, lo, hi, 8)):
        assert np.array_equal(_bits(g), _bits(w)), "per-ray"


def test_library_exports_multi_hit():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_multi_hit_rays", "rt_multi_hit_rays_ranged"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_multi_hit_rays.argtypes) == 11
    assert len(_lib.lib.rt_multi_hit_rays_ranged.argtypes) == 11
    for name in ("multi_hit_rays", "multi_hit_rays_into", "multi_hit_rays_ranged_into"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.multi_hit_rays_into).parameters) == [
        "rays_ptr", "n", "prepared", "k", "count_ptr", "index_ptr", "root_ptr", "hit_ptr", "t_min", "t_max"]
    assert list(inspect.signature(R.multi_hit_rays_ranged_into).parameters) == [
        "rays_ptr", "n", "prepared", "t_min_ptr", "t_max_ptr", "k", "count_ptr", "index_ptr", "root_ptr", "hit_ptr"]
    assert list(inspect.signature(R.multi_hit_rays).parameters) == ["prepared", "rays", "k", "t_min", "t_max"]
