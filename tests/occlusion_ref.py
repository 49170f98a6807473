"""numpy float32 restatement of rt_occluded_rays over the oracle's {L, I}, on top of ray_query_ref.RefScene.

occluded(r, t_min, t_max) is bvh_fold (bvh.fut:61-84) with `contains = aabb_hit _ r t_min t_max` and an OR of
`sphere_hit L[j] r t_min t_max is #some`: some leaf whose every inner ancestor's box passes over (t_min, t_max) and whose
sphere has root1 or root2 strictly inside (t_min, t_max).  The OR does not depend on the order of the walk.
"""
import numpy as np

F = np.float32


def _inside(t, lo, hi):
    with np.errstate(invalid="ignore"):
        return (t > lo) & (t < hi)


def occluded(ref, o, d, t_min, t_max, chunk=256):
    """[n] bool: the contract of rt_occluded_rays for rays {o, d} over the scalar interval (t_min, t_max)."""
    return _fold(ref, o, d, t_min, t_max, chunk, boxes=True)


def any_sphere(ref, o, d, t_min, t_max, chunk=256):
    """[n] bool: the same without the box tests -- some sphere of the scene with a root inside (t_min, t_max)."""
    return _fold(ref, o, d, t_min, t_max, chunk, boxes=False)


def _fold(ref, o, d, t_min, t_max, chunk, boxes):
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    lo, hi = F(t_min), F(t_max)
    out = np.zeros(o.shape[0], bool)
    for s in range(0, o.shape[0], chunk):
        e = min(o.shape[0], s + chunk)
        r1, r2, pos = ref.roots(o[s:e], d[s:e])
        acc = pos & (_inside(r1, lo, hi) | _inside(r2, lo, hi))
        if boxes:
            acc &= ref.visited(o[s:e], d[s:e], lo, hi)
        out[s:e] = acc.any(axis=1)
    return out


def seeded_rays(sc_arrays, n, seed):
    """Arbitrary rays around a scene: origins inside its box, far outside it and inside spheres; directions random, axis-aligned, with a
    zero component, magnitudes 1e-3 .. 1e3.  [n, 6] float32."""
    rng = np.random.default_rng(seed)
    L = sc_arrays["L"]
    lo, hi = L[:, :3].min(0) - L[:, 6:7].max(), L[:, :3].max(0) + L[:, 6:7].max()
    ext = hi - lo
    k = n // 4
    o_in = lo + rng.random((k, 3)) * ext
    o_out = lo - ext + rng.random((k, 3)) * 3 * ext
    pick = rng.integers(0, L.shape[0], k)
    o_sph = L[pick, :3] + (rng.random((k, 3)) - 0.5) * L[pick, 6:7]
    o_mix = lo + rng.random((n - 3 * k, 3)) * ext
    o = np.concatenate([o_in, o_out, o_sph, o_mix]).astype(F)
    d = rng.normal(size=(n, 3))
    axis = rng.integers(0, 3, n // 8)
    d[: n // 8] = 0
    d[np.arange(n // 8), axis] = rng.choice([-1.0, 1.0], n // 8)
    d[n // 8: n // 4, rng.integers(0, 3)] = 0.0
    d *= 10.0 ** rng.uniform(-3, 3, (n, 1))
    return np.concatenate([o, d.astype(F)], axis=1).astype(F)


# A point light per scene for the shadow-ray sets (tools/occlusion_probe.py, tests/test_occlusion_gpu.py)
LIGHTS = {"rgbbox": (40.0, 10.0, 40.0), "irreg": (0.0, 8.0, 0.0)}   # about 57 % and 35 % of the camera rays' shadow rays blocked


def shadow_rays(index, hit7, light):
    """Shadow rays from the hit points of a closest-hit query (index >= 0) toward a point light: o = p, d = light - p; the query's
    interval is then (eps, 1).  [m, 6] float32, m = the number of hits."""
    p = np.asarray(hit7, dtype=F)[np.asarray(index) >= 0, 1:4]
    d = np.asarray(light, dtype=F)[None, :] - p
    return np.concatenate([p, d], axis=1).astype(F)
