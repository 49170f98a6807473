"""CPU checks of the occlusion query: the restatement (occlusion_ref.py) against objs_hit and a brute-force sphere test, and the
loader's symbols."""
import numpy as np
import pytest

import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q

SCENES = [("rgbbox", {}, 17), ("irreg", {}, 29), ("floor", {"n": 37, "k": 222.0}, 41)]
NRAYS = 2048


@pytest.fixture(scope="module", params=SCENES, ids=[s[0] for s in SCENES])
def scene(request):
    name, kw, seed = request.param
    arr = O.OracleScene(name, **kw).arrays()
    return Q.RefScene(arr), X.seeded_rays(arr, NRAYS, seed)


@pytest.mark.parametrize("t_max", [1e9, 30.0])
def test_agrees_with_objs_hit_at_scene_epsilon(scene, t_max):
    # at t_min = 0.1 the box interval and the set of accepted roots are objs_hit's: occluded == (index >= 0) while the
    # closest root is below 2^23 (the re-hit over (0.1, t + 1) then cannot fail)
    ref, rays = scene
    o, d = rays[:, :3], rays[:, 3:]
    idx, hit = ref.objs_hit(o, d, np.float32(0.1), np.float32(t_max))
    occ = X.occluded(ref, o, d, 0.1, t_max)
    small = ~((idx >= 0) & (hit[:, 0] >= 2.0 ** 23))
    assert occ.any() and not occ.all()
    bad = np.nonzero((occ != (idx >= 0)) & small)[0]
    assert bad.size == 0, f"{bad.size} rays differ, first {bad[:5]}"


@pytest.mark.parametrize("t_min,t_max", [(0.1, 1e9), (0.0, 1e9), (0.5, 30.0), (0.0, 0.05)])
def test_agrees_with_brute_force(scene, t_min, t_max):
    # without the box tests: any sphere with a root in the interval (grazing rays could differ; these seeds have none)
    ref, rays = scene
    occ = X.occluded(ref, rays[:, :3], rays[:, 3:], t_min, t_max)
    brute = X.any_sphere(ref, rays[:, :3], rays[:, 3:], t_min, t_max)
    bad = np.nonzero(occ != brute)[0]
    assert bad.size == 0, f"{bad.size} rays differ, first {bad[:5]}"


def test_empty_interval_occludes_nothing(scene):
    ref, rays = scene
    assert not X.occluded(ref, rays[:, :3], rays[:, 3:], 7.0, 7.0).any()


def test_shadow_rays_toward_the_light():
    sc = O.OracleScene("rgbbox")
    ref = Q.RefScene(sc.arrays())
    rays = Q.camera_rays(sc.camera_floats(24, 24), 24, 24)
    idx, hit = ref.objs_hit(rays[:, :3], rays[:, 3:], 0.0, 1e9)
    sh = X.shadow_rays(idx, hit, X.LIGHTS["rgbbox"])
    assert sh.shape == (int((idx >= 0).sum()), 6)
    assert np.array_equal(sh[:, :3], hit[idx >= 0, 1:4])
    assert np.allclose(sh[:, :3] + sh[:, 3:], np.float32(X.LIGHTS["rgbbox"]), atol=1e-4)
    occ = X.occluded(ref, sh[:, :3], sh[:, 3:], 1e-3, 1.0)
    assert 0.1 < occ.mean() < 0.9


def test_library_exports_occlusion():
    from raytracers_amd import _lib
    assert hasattr(_lib.lib, "rt_occluded_rays")
    assert "rt_occluded_rays" in _lib.RT_SYMBOLS
    import raytracers_amd as R
    for name in ("occluded_rays", "occluded_rays_into"):
        assert callable(getattr(R, name)), name
