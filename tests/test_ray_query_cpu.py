"""CPU checks of the caller-ray entries: the numpy restatement (ray_query_ref.py) against the oracle, and the loader's symbols."""
import numpy as np
import pytest

import oracle_lib as O
import ray_query_ref as Q

SCENES = [("rgbbox", {}), ("irreg", {}), ("floor", {"n": 37, "k": 222.0})]


def _scene(name, kw):
    return O.OracleScene(name, **kw)


@pytest.mark.parametrize("name,kw", SCENES, ids=[s[0] for s in SCENES])
@pytest.mark.parametrize("h,w", [(40, 56), (1, 1), (37, 53)])
def test_restatement_reproduces_oracle_images(name, kw, h, w):
    sc = _scene(name, kw)
    ref = Q.RefScene(sc.arrays())
    rays = Q.camera_rays(sc.camera_floats(h, w), h, w)
    for depth in (0, 1, 2, 50):
        want, _ = sc.render(h, w, max_depth=depth)
        got = Q.colour_to_pixel(ref.ray_colour(rays[:, :3], rays[:, 3:], depth)).reshape(h, w)
        assert np.array_equal(got, want), f"{name} {h}x{w} depth {depth}: {int((got != want).sum())} pixels differ"


def test_restatement_custom_camera():
    sc = _scene("rgbbox", {})
    ref = Q.RefScene(sc.arrays())
    cam = sc.camera_floats(30, 30)
    cam[0:3] += np.float32([3.0, -2.0, 7.5])   # a moved origin: the same llc / horizontal / vertical
    rays = Q.camera_rays(cam, 30, 30)
    for depth in (1, 50):
        want, _ = sc.render(30, 30, max_depth=depth, cam=cam)
        got = Q.colour_to_pixel(ref.ray_colour(rays[:, :3], rays[:, 3:], depth)).reshape(30, 30)
        assert np.array_equal(got, want)


def test_restatement_interval_and_rehit():
    # objs_hit with the render path's interval: the hit's t is what the re-hit returns, p / normal from it
    sc = _scene("rgbbox", {})
    ref = Q.RefScene(sc.arrays())
    rays = Q.camera_rays(sc.camera_floats(24, 24), 24, 24)
    idx, hit = ref.objs_hit(rays[:, :3], rays[:, 3:], 0.0, 1e9)
    assert (idx >= 0).any() and (idx < 0).any()
    assert (hit[idx < 0] == 0).all()
    # an empty interval (t, t) hits nothing: every box fails
    idx0, hit0 = ref.objs_hit(rays[:, :3], rays[:, 3:], 5.0, 5.0)
    assert (idx0 == -1).all() and (hit0 == 0).all()


def test_library_exports_ray_query_symbols():
    from raytracers_amd import _lib
    for name in ("rt_trace_rays", "rt_intersect_rays", "rt_camera_rays", "rt_copy_to_device"):
        assert hasattr(_lib.lib, name), name
        assert name in _lib.RT_SYMBOLS, name
    import raytracers_amd as R
    for name in ("trace_rays", "intersect_rays", "camera_rays", "trace_rays_into", "intersect_rays_into", "camera_rays_into"):
        assert callable(getattr(R, name)), name
