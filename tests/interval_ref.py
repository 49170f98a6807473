"""numpy float32 restatement of the per-ray interval queries (rt_occluded_rays_ranged, rt_intersect_rays_ranged).

Ray i gets exactly what the scalar query gives it alone at (t_min[i], t_max[i]); a ray whose interval fails
0 <= t_min <= t_max <= 1e9 (NaN and +-inf included) is a miss: occluded False, index -1 and seven zeros.
"""
import numpy as np

from occlusion_ref import _inside

F = np.float32
TMAX = F(1e9)


def interval_ok(t_min, t_max):
    """[n] bool: the interval rule, ray by ray (every compare is False on a NaN)."""
    lo, hi = np.asarray(t_min, dtype=F), np.asarray(t_max, dtype=F)
    with np.errstate(invalid="ignore"):
        return (lo >= 0) & (lo <= hi) & (hi <= TMAX)


def _bounds(n, t_min, t_max):
    return (np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=F), (n,))),
            np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, dtype=F), (n,))))


def occluded(ref, o, d, t_min, t_max, chunk=256):
    """[n] bool: rt_occluded_rays_ranged for rays {o, d}; t_min / t_max scalars or [n] arrays."""
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    lo_all, hi_all = _bounds(o.shape[0], t_min, t_max)
    ok_all = interval_ok(lo_all, hi_all)
    out = np.zeros(o.shape[0], bool)
    for s in range(0, o.shape[0], chunk):
        e = min(o.shape[0], s + chunk)
        ok = ok_all[s:e]
        # (an invalid ray's bounds are replaced by an empty interval before the fold; its answer is forced to False below anyway)
        lo = np.where(ok, lo_all[s:e], F(0))[:, None]
        hi = np.where(ok, hi_all[s:e], F(0))[:, None]
        r1, r2, pos = ref.roots(o[s:e], d[s:e])
        acc = pos & (_inside(r1, lo, hi) | _inside(r2, lo, hi))
        acc &= ref.visited(o[s:e], d[s:e], lo, hi)
        out[s:e] = acc.any(axis=1) & ok
    return out


def objs_hit(ref, o, d, t_min, t_max, chunk=256):
    """(index [n] int32, hit [n, 7] float32): rt_intersect_rays_ranged -- RefScene.objs_hit with per-ray bounds, misses where the
    interval is invalid."""
    o = np.ascontiguousarray(o, dtype=F)
    lo, hi = _bounds(o.shape[0], t_min, t_max)
    ok = interval_ok(lo, hi)
    idx, hit = ref.objs_hit(o, d, np.where(ok, lo, F(0)), np.where(ok, hi, F(0)), chunk)
    idx[~ok] = -1
    hit[~ok] = 0
    return idx, hit


def normalised_shadow_rays(index, hit7, light, eps=1e-3):
    """Shadow rays with unit directions from the hit points (index >= 0) toward a point light, and each one's t_max = |L - p| - eps:
    (rays [m, 6] float32, t_max [m] float32).  The same segments as occlusion_ref.shadow_rays over (eps, 1), rescaled."""
    p = np.asarray(hit7, dtype=F)[np.asarray(index) >= 0, 1:4]
    v = np.asarray(light, dtype=F)[None, :] - p
    dist = np.sqrt((v * v).sum(axis=1)).astype(F)
    d = (v / dist[:, None]).astype(F)
    return np.concatenate([p, d], axis=1).astype(F), (dist - F(eps)).astype(F)


def mixed_intervals(n, seed, choices=((0.0, 1e9), (0.1, 1e9), (0.1, 30.0), (1e-3, 1.0), (3.0, 3.0), (0.5, 5.0))):
    """[n] t_min, [n] t_max, [n] bucket: each ray one of `choices`, assigned at random."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(choices), n)
    c = np.asarray(choices, dtype=F)
    return c[k, 0].copy(), c[k, 1].copy(), k
