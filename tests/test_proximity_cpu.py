"""CPU checks of the proximity query: the restatement (proximity_ref.py) -- its prefix property, its agreement with an independent float64
nearest-neighbour search on point clouds, its restricted form against the full brute force -- the box test's bound check
(build/proximity_bound_check: no counterexample with the slack, counterexamples without it), and the loader's symbols and signatures."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import proximity_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _points(L, m, seed):
    """points in and around the scene's box, some at centres and on surfaces"""
    rng = np.random.default_rng(seed)
    lo, hi = L[:, :3].min(axis=0), L[:, :3].max(axis=0)
    pad = 0.1 * (hi - lo) + 1.0
    p = rng.uniform(lo - pad, hi + pad, (m, 3)).astype(F)
    j = rng.integers(0, L.shape[0], m // 4)
    p[: j.size] = L[j, :3]
    d = rng.normal(size=(m // 4, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    j2 = rng.integers(0, L.shape[0], m // 4)
    p[j.size: j.size + j2.size] = (L[j2, :3] + d * L[j2, 6:7]).astype(F)
    return p


@pytest.fixture(scope="module", params=[("rgbbox", {}), ("irreg", {}), ("floor", {"n": 37, "k": 222.0})], ids=["rgbbox", "irreg", "floor"])
def scene(request):
    name, kw = request.param
    return O.OracleScene(name, **kw).arrays()["L"]


@pytest.mark.parametrize("max_dist", [0.0, 0.5, 3.0, 1e9])
def test_prefix_and_order(scene, max_dist):
    L = scene
    p = _points(L, 512, 5)
    full = P.nearest(L, p, max_dist, P.KMAX)
    if max_dist == 1e9:
        assert (full[0] == L.shape[0]).all()
    for k in (1, 3, 8):
        part = P.nearest(L, p, max_dist, k)
        assert np.array_equal(part[0], full[0])
        assert np.array_equal(part[1], full[1][:, :k]) and np.array_equal(_bits(part[2]), _bits(full[2][:, :k])), k
    cnt, idx, gap = full
    g = P.gaps(L, p)
    for i in range(0, 512, 7):
        m = min(int(cnt[i]), P.KMAX)
        keys = list(zip(gap[i, :m].tolist(), idx[i, :m].tolist()))
        assert keys == sorted(keys)
        assert (idx[i, m:] == -1).all() and not gap[i, m:].any()
        assert np.array_equal(_bits(gap[i, :m]), _bits(g[i, idx[i, :m]]))
        assert int(cnt[i]) == int((g[i] <= F(max_dist)).sum())


def test_invalid_points_and_bounds(scene):
    L = scene
    p = _points(L, 64, 9)
    p[3, 0] = np.nan
    p[4, 2] = np.inf
    md = np.full(64, 2.0, F)
    md[[10, 11, 12, 13, 14]] = [np.nan, np.inf, -np.inf, -1.0, 2e9]
    md[20] = -0.0
    cnt, idx, gap = P.nearest(L, p, md, 4)
    bad = [3, 4, 10, 11, 12, 13, 14]
    assert not cnt[bad].any() and (idx[bad] == -1).all() and not gap[bad].any()
    want = P.nearest(L, p[20:21], 0.0, 4)
    assert np.array_equal(cnt[20:21], want[0]) and np.array_equal(idx[20:21], want[1])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_point_cloud_equals_float64_knn(seed):
    # radius 0: plain k-nearest-neighbour search of the centres; where the float32 gaps are not tied, the float64 distances order the same
    rng = np.random.default_rng(seed)
    n = 700
    L = np.zeros((n, 7), F)
    L[:, :3] = rng.uniform(-50, 50, (n, 3))
    q = rng.uniform(-60, 60, (300, 3)).astype(F)
    k = 8
    cnt, idx, gap = P.nearest(L, q, 1e9, k)
    d64 = np.sqrt(((q[:, None, :].astype(np.float64) - L[None, :, :3].astype(np.float64)) ** 2).sum(axis=2))
    want = np.argsort(d64, axis=1, kind="stable")[:, :k]
    g32 = P.gaps(L, q)
    checked = 0
    for i in range(q.shape[0]):
        srt = np.sort(g32[i])
        if np.unique(srt[: k + 1]).size < k + 1:      # a float32 tie among the first k + 1: the orders may differ
            continue
        assert np.array_equal(idx[i], want[i]), i
        checked += 1
    assert checked > 250


@pytest.mark.parametrize("kind", ["irreg", "dups", "cloud"])
def test_near_equals_full(kind):
    rng = np.random.default_rng(4)
    if kind == "irreg":
        L = O.OracleScene("irreg").arrays()["L"]
    else:
        n = 900
        L = np.zeros((n, 7), F)
        L[:, :3] = rng.uniform(-30, 30, (n, 3))
        L[:, 6] = 0.0 if kind == "cloud" else rng.uniform(0.2, 2.0, n)
        if kind == "dups":
            L[n // 2:] = L[: n - n // 2]
    p = _points(L, 400, 11)
    md = rng.uniform(0.0, 8.0, 400).astype(F)
    md[::17] = np.nan
    for k in (1, 5, P.KMAX):
        for bound in (md, 4.0, 0.0):
            got, want = P.nearest_near(L, p, bound, k), P.nearest(L, p, bound, k)
            for g, w in zip(got, want):
                assert np.array_equal(_bits(g), _bits(w)), (k, bound if np.ndim(bound) == 0 else "per-point")


def _bound_check(*args):
    exe = os.path.join(ROOT, "build", "proximity_bound_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "build/proximity_bound_check"], check=True, capture_output=True)
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600, env=env)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bound_check_finds_no_counterexample(seed):
    r = _bound_check(300, seed)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "P1 violations 0" in r.stdout and "safety violations 0" in r.stdout, r.stdout
    assert " 0 tall scenes" not in r.stdout, r.stdout


def test_bound_check_sees_missing_slack():
    # the same search without the slack must find boxes that would drop a selected sphere -- the check can fail
    r = _bound_check(100, 2, 0.0)
    assert r.returncode == 1 and "safety violations 0" not in r.stdout, r.stdout


def test_bound_check_sees_partial_boxes():
    # ... and so must testing the partial boxes near the root of trees taller than the AABB propagation's sweeps
    r = _bound_check(100, 3, 1.0, 1)
    assert r.returncode == 1 and "safety violations 0" not in r.stdout, r.stdout


def test_library_exports_proximity():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_nearest_spheres", "rt_nearest_spheres_ranged", "rt_prepared_get_sphere_ids"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_nearest_spheres.argtypes) == 9
    assert len(_lib.lib.rt_nearest_spheres_ranged.argtypes) == 9
    assert len(_lib.lib.rt_prepared_get_sphere_ids.argtypes) == 3
    for name in ("nearest_spheres", "nearest_spheres_into", "nearest_spheres_ranged_into"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.nearest_spheres).parameters) == ["prepared", "points", "k", "max_dist", "count"]
    assert list(inspect.signature(R.nearest_spheres_into).parameters) == [
        "points_ptr", "n", "prepared", "k", "count_ptr", "index_ptr", "gap_ptr", "max_dist"]
    assert list(inspect.signature(R.nearest_spheres_ranged_into).parameters) == [
        "points_ptr", "n", "prepared", "max_dist_ptr", "k", "count_ptr", "index_ptr", "gap_ptr"]
    assert callable(R.Prepared.sphere_ids) and callable(R.Prepared.sphere_ids_into)


def test_header_declares_proximity():
    h = open(os.path.join(ROOT, "include", "rt_mi355x.h")).read()
    for sym in ("rt_nearest_spheres(", "rt_nearest_spheres_ranged(", "rt_prepared_get_sphere_ids("):
        assert sym in h, sym
