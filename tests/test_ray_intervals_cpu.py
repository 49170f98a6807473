"""CPU checks of the per-ray interval queries: the restatement (interval_ref.py) against the scalar restatements, bucket by bucket,
the invalid-interval rule, and the loader's symbols and Python signatures."""
import inspect

import numpy as np
import pytest

import interval_ref as V
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
    return Q.RefScene(arr), X.seeded_rays(arr, NRAYS, seed)


@pytest.mark.parametrize("t_min,t_max", [(0.0, 1e9), (0.1, 1e9), (0.1, 30.0), (1e-3, 1.0), (3.0, 3.0)])
def test_constant_arrays_equal_scalar(scene, t_min, t_max):
    ref, rays = scene
    o, d = rays[:, :3], rays[:, 3:]
    lo, hi = np.full(NRAYS, t_min, F), np.full(NRAYS, t_max, F)
    assert np.array_equal(V.occluded(ref, o, d, lo, hi), X.occluded(ref, o, d, t_min, t_max))
    idx, hit = V.objs_hit(ref, o, d, lo, hi)
    want_idx, want_hit = ref.objs_hit(o, d, F(t_min), F(t_max))
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(hit.view(np.uint32), want_hit.view(np.uint32))


def test_mixed_intervals_equal_buckets(scene):
    ref, rays = scene
    o, d = rays[:, :3], rays[:, 3:]
    lo, hi, k = V.mixed_intervals(NRAYS, seed=7)
    occ = V.occluded(ref, o, d, lo, hi)
    idx, hit = V.objs_hit(ref, o, d, lo, hi)
    assert occ.any() and not occ.all()
    for b in np.unique(k):
        m = k == b
        t0, t1 = lo[m][0], hi[m][0]
        assert np.array_equal(occ[m], X.occluded(ref, o[m], d[m], t0, t1)), (t0, t1)
        want_idx, want_hit = ref.objs_hit(o[m], d[m], t0, t1)
        assert np.array_equal(idx[m], want_idx), (t0, t1)
        assert np.array_equal(hit[m].view(np.uint32), want_hit.view(np.uint32)), (t0, t1)


def test_invalid_intervals_miss(scene):
    ref, rays = scene
    o, d = rays[:, :3], rays[:, 3:]
    lo, hi = np.full(NRAYS, 0.0, F), np.full(NRAYS, 1e9, F)
    bad = [(np.nan, 1.0), (0.0, np.nan), (0.0, np.inf), (-np.inf, 1.0), (-1.0, 1.0), (2.0, 1.0), (0.0, 2e9), (np.inf, np.inf)]
    where = np.arange(len(bad)) * 37 + 3
    for i, (a, b) in zip(where, bad):
        lo[i], hi[i] = a, b
    ok = V.interval_ok(lo, hi)
    assert not ok[where].any() and ok.sum() == NRAYS - len(bad)
    occ = V.occluded(ref, o, d, lo, hi)
    idx, hit = V.objs_hit(ref, o, d, lo, hi)
    assert not occ[where].any()
    assert (idx[where] == -1).all() and not hit[where].any()
    full = X.occluded(ref, o, d, 0.0, 1e9)
    full_idx, full_hit = ref.objs_hit(o, d, F(0.0), F(1e9))
    assert full[where].any()          # the rays the rule turns into misses were not misses
    assert np.array_equal(occ[ok], full[ok])
    assert np.array_equal(idx[ok], full_idx[ok])
    assert np.array_equal(hit[ok].view(np.uint32), full_hit[ok].view(np.uint32))
    # -0.0 is a valid bound and behaves as 0.0
    assert V.interval_ok(F(-0.0), F(1.0)) and V.interval_ok(F(0.0), F(-0.0))
    assert np.array_equal(V.occluded(ref, o, d, np.full(NRAYS, -0.0, F), hi), V.occluded(ref, o, d, np.zeros(NRAYS, F), hi))


def test_normalised_shadow_rays_match_segments():
    # the normalised rays over (0, |L - p| - eps) and the unnormalised ones over (eps, 1) are different floating-point problems; they
    # agree on nearly every ray, which is the point of carrying the interval per ray rather than rescaling
    sc = O.OracleScene("rgbbox")
    ref = Q.RefScene(sc.arrays())
    rays = Q.camera_rays(sc.camera_floats(24, 24), 24, 24)
    idx, hit = ref.objs_hit(rays[:, :3], rays[:, 3:], 0.0, 1e9)
    sh, t_max = V.normalised_shadow_rays(idx, hit, X.LIGHTS["rgbbox"])
    assert sh.shape == (int((idx >= 0).sum()), 6) and t_max.shape == (sh.shape[0],)
    assert np.allclose(np.linalg.norm(sh[:, 3:], axis=1), 1.0, atol=1e-5)
    occ = V.occluded(ref, sh[:, :3], sh[:, 3:], 1e-3, t_max)
    seg = X.occluded(ref, sh[:, :3], X.shadow_rays(idx, hit, X.LIGHTS["rgbbox"])[:, 3:], 1e-3, 1.0)
    assert 0.1 < occ.mean() < 0.9
    assert (occ == seg).mean() > 0.98


def test_library_exports_ranged_entries():
    from raytracers_amd import _lib
    import raytracers_amd as R
    for sym in ("rt_intersect_rays_ranged", "rt_occluded_rays_ranged"):
        assert hasattr(_lib.lib, sym), sym
        assert sym in _lib.RT_SYMBOLS, sym
    assert len(_lib.lib.rt_intersect_rays_ranged.argtypes) == 8
    assert len(_lib.lib.rt_occluded_rays_ranged.argtypes) == 7
    for name in ("intersect_rays_ranged_into", "occluded_rays_ranged_into"):
        assert callable(getattr(R, name)), name
    assert list(inspect.signature(R.intersect_rays_ranged_into).parameters) == [
        "rays_ptr", "n", "prepared", "t_min_ptr", "t_max_ptr", "index_ptr", "hit_ptr"]
    assert list(inspect.signature(R.occluded_rays_ranged_into).parameters) == [
        "rays_ptr", "n", "prepared", "t_min_ptr", "t_max_ptr", "out_ptr"]
    from raytracers_amd import api
    assert api._is_bound_array(np.zeros(3, F)) and not api._is_bound_array(0.5) and not api._is_bound_array(F(0.5))
