"""The numpy restatements of the ray queries (ray_query_ref, interval_ref, occlusion_ref, multi_hit_ref) against the C oracle's literal
bvh_fold walk (oracle/ray_oracle.c: orc_*_rays) on the edge scenes and ray families of edge_rays.py.  The restatements replace the walk
with an order-independent rule; these are the inputs where that argument is delicate (NaN and +-inf components, zero, denormal, tiny and
huge directions, -0.0 slab swaps, tangent rays, roots on the interval's ends, ties in t).  No GPU needed."""
import functools

import numpy as np
import pytest

import edge_rays as E
import interval_ref as V
import multi_hit_ref as M
import occlusion_ref as X
import oracle_lib as O
import ray_query_ref as Q

F = np.float32
SCENES = tuple(E.SCENES)
same_bits = E.same_bits


@functools.lru_cache(maxsize=None)
def _scene(name):
    s, lf, la, fov = E.SCENES[name]
    orc = O.OracleScene("custom", spheres7=s, look_from=lf, look_at=la, fov=fov)
    arr = orc.arrays()
    fam = E.ray_families(arr, seed=1)
    rays = np.concatenate(list(fam.values()))
    label = np.concatenate([np.full(v.shape[0], i) for i, v in enumerate(fam.values())])
    lo, hi, _ = E.edge_intervals(arr, rays, seed=2)
    return orc, arr, Q.RefScene(arr), fam, rays, label, lo, hi


def _by_family(check, name):
    """Run check(rays, lo, hi, tag) once on all the scene's edge rays, and again family by family if it fails, so that the failure names
    the family."""
    orc, arr, ref, fam, rays, label, lo, hi = _scene(name)
    try:
        check(rays, lo, hi, name)
    except AssertionError:
        for i, f in enumerate(fam):
            m = label == i
            check(rays[m], lo[m], hi[m], f"{name}/{f}")
        raise


def test_edge_inputs_cover_every_family():
    total = 0
    for name in SCENES:
        orc, arr, ref, fam, rays, label, lo, hi = _scene(name)
        assert all(v.shape[0] > 0 for v in fam.values()), name
        total += rays.shape[0]
        if name in ("two_apart", "same64", "nan_grid"):     # integer centres and radii: the tangent rays are exactly tangent
            assert E.tangent_disc(arr, fam["tangent"]).all(), name
        # the -0.0 slabs and the non-finite components are really there
        assert (np.signbit(fam["axis_signed_zero"][:, 3:]) & (fam["axis_signed_zero"][:, 3:] == 0)).any(), name
        assert np.isnan(fam["non_finite"]).any() and np.isinf(fam["non_finite"]).any(), name
        # roots exactly at kEps, and bounds equal to a ray's own roots
        r1, r2, ok = ref.roots(fam["root_at_eps"][:, :3], fam["root_at_eps"][:, 3:])
        assert (ok & ((r1 == F(0.1)) | (r2 == F(0.1)))).any(), name
        o1, o2 = E.roots_of(arr, rays)
        assert ((lo == o1) & np.isfinite(o1)).any() and ((hi == o2) & np.isfinite(o2)).any(), name
        assert (~V.interval_ok(lo, hi)).any() and V.interval_ok(lo, hi).any(), name
    assert total >= 10000, total
    # the tall tree is as tall as the render path's test says
    assert len(_scene("tall1100")[2].levels) == E.TALL_HEIGHT


@pytest.mark.parametrize("name", SCENES)
def test_objs_hit_scalar_and_per_ray(name):
    orc, arr, ref, *_ = _scene(name)

    def check(rays, lo, hi, tag):
        o, d = rays[:, :3], rays[:, 3:]
        for t0, t1 in ((0.0, 1e9), (0.1, 40.0), (F(0.1), F(0.1))):
            gi, gh = orc.objs_hit_rays(rays, t0, t1)
            wi, wh = ref.objs_hit(o, d, F(t0), F(t1))
            same_bits(gi, wi, f"{tag} ({t0}, {t1}) index")
            same_bits(gh, wh, f"{tag} ({t0}, {t1}) hit7")
        gi, gh = orc.objs_hit_rays(rays, lo, hi)
        wi, wh = V.objs_hit(ref, o, d, lo, hi)
        same_bits(gi, wi, f"{tag} per-ray index")
        same_bits(gh, wh, f"{tag} per-ray hit7")
    _by_family(check, name)


@pytest.mark.parametrize("name", SCENES)
def test_ray_colour(name):
    orc, arr, ref, *_ = _scene(name)

    def check(rays, lo, hi, tag):
        for depth in (1, 2, 50):
            same_bits(orc.ray_colour_rays(rays, depth), ref.ray_colour(rays[:, :3], rays[:, 3:], depth), f"{tag} depth {depth}")
    _by_family(check, name)


@pytest.mark.parametrize("name", SCENES)
def test_occluded(name):
    orc, arr, ref, *_ = _scene(name)

    def check(rays, lo, hi, tag):
        o, d = rays[:, :3], rays[:, 3:]
        for t0, t1 in ((0.0, 1e9), (0.1, 30.0)):
            same_bits(orc.occluded_rays(rays, t0, t1), X.occluded(ref, o, d, t0, t1), f"{tag} ({t0}, {t1})")
        same_bits(orc.occluded_rays(rays, lo, hi), V.occluded(ref, o, d, lo, hi), f"{tag} per-ray")
    _by_family(check, name)


@pytest.mark.parametrize("name", SCENES)
def test_multi_hit(name):
    orc, arr, ref, *_ = _scene(name)

    def check(rays, lo, hi, tag):
        o, d = rays[:, :3], rays[:, 3:]
        for k in (1, 32):
            for bounds, what in (((0.0, 1e9), "(0, 1e9)"), ((lo, hi), "per-ray")):
                got = orc.crossings_rays(rays, *bounds, k)
                want = M.multi_hit(ref, o, d, *bounds, k)
                walk = M.multi_hit_walk(arr, o, d, *bounds, k)
                for part, g, w, wk in zip(("count", "index", "root", "hit7"), got, want, walk):
                    same_bits(g, w, f"{tag} {what} k={k} {part}")
                    same_bits(wk, w, f"{tag} {what} k={k} {part} (multi_hit_walk)")
    _by_family(check, name)


def test_crossing_ties_between_spheres():
    # the touching chain of the overlap scene: sphere i's exit and sphere i+1's entry at the same t, and more than 32 crossings from inside
    orc, arr, ref, fam, rays, *_ = _scene("overlap")
    cnt, idx, root, hit = orc.crossings_rays(rays, 0.0, 1e9, 32)
    t = hit[:, :, 0]
    tie = (t[:, 1:] == t[:, :-1]) & (idx[:, 1:] >= 0) & (idx[:, 1:] != idx[:, :-1])
    assert (tie & (root[:, :-1] == 2) & (root[:, 1:] == 1)).any()
    assert (cnt > 32).any()
