"""The GPU BVH builder's two large size classes -- CHAINED (24 577 .. 131 072 spheres) and the one beyond -- on the scenes of edge_builds.py:
all keys equal, seven keys, flat lines, chains of 30 levels over a hundred thousand duplicates, a forest of 21-level chains, and non-finite
spheres.  Every build is compared byte for byte with the oracle's {left, right, parent, L, bmin, bmax} and its height, through
prepare_scene and prepare_scene_from_spheres, with the device builder and (up to 131 073 spheres) the host builder; the traversal copy
through one small frame per kernel family (or, at 524 289 spheres, the camera's rays through intersect_rays) bit for bit against the
oracle; the consumers of the sweep count -- exact_depth in the proximity and range queries, the culling guard -- on the trees whose height
exceeds it; and update_spheres from a tall tree to a flat one and back.  test_build_edges_cpu.py shows, without a device, that these
scenes would catch an unstable sort, one sweep too many or too few, and a node that drops out of the sweeps one sweep early.

The non-finite families (`nan`, `nan_y`, `inf`, `zero_radius`) are compared with the oracle as well: its build is defined for them
(test_build_edges_cpu.test_oracle_build_is_defined_on_non_finite_spheres), so one expectation covers both builders."""
import functools

import numpy as np
import pytest

import edge_builds as B
import edge_cull as EC
import edge_rays as ER
import oracle_lib as O
import proximity_ref as P
import within_ref as W

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("left", "right", "parent", "L", "bmin", "bmax")
BUILD_CASES = B.finite_cases() + [(f, n) for f in B.NON_FINITE for n in B.NON_FINITE_SIZES]
FRAME_CASES = B.finite_cases(huge=False)
CONSUMER_CASES = [(f, n) for f in B.TALL for n in (24577, 131073)]
HOST_BUILDER_MAX_N = 131073
DEFAULTS = dict(lds_scene_bytes=-1, waves_per_wg=0, wgs_per_cu=1, cull=-1, gpu_build=1)
L2_16 = dict(waves_per_wg=16, wgs_per_cu=1, lds_scene_bytes=0)      # the shape the CULL instantiations exist for (test_cull_edges_gpu)
NO_VIEW = ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 40.0)
_id = lambda c: f"{c[0]}:{c[1]}"   # noqa: E731


@pytest.fixture(scope="module")
def R():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import raytracers_amd
    return raytracers_amd


@pytest.fixture(scope="module")
def ctx(R):
    c = R.Context(0)
    yield c
    c.close()


def _restore(R, ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.set_variant(R.VARIANT_AUTO)


def _view(family):
    return B.VIEWS.get(family, NO_VIEW)


@functools.lru_cache(maxsize=3)
def _expect(family, n):
    """(oracle scene, its arrays, its tree's height): computed once per scene, shared by the tests of that scene, never written to"""
    orc = O.OracleScene("custom", spheres7=B.scene(family, n), look_from=_view(family)[0], look_at=_view(family)[1], fov=_view(family)[2])
    a = orc.arrays()
    for v in a.values():
        v.setflags(write=False)
    return orc, a, B.height_of(a["left"], a["right"])


def _same_build(ps, family, n, what):
    _, want, height = _expect(family, n)
    got = ps.bvh_arrays()
    for k in KEYS:
        if got[k].tobytes() != want[k].tobytes():
            g, w = got[k].view(np.uint32).reshape(len(got[k]), -1), want[k].view(np.uint32).reshape(len(want[k]), -1)
            rows = np.nonzero((g != w).any(axis=1))[0]
            only_nan = bool(got[k].dtype == F and (np.isnan(got[k]) == np.isnan(want[k])).all() and
                            (g == w)[~np.isnan(want[k]).reshape(g.shape)].all())
            raise AssertionError(f"{what}: {k} differs from the oracle's in {rows.size} rows, first {rows[:5]}"
                                 + (" (only in the bits of NaNs)" if only_nan else ""))
    assert ps.height == height, f"{what}: height {ps.height}, the oracle's tree has {height}"
    s = B.scene(family, n)
    ids = ps.sphere_ids()
    assert ids.shape == (n,) and s[ids].tobytes() == got["L"].tobytes(), f"{what}: L != spheres[sphere_ids()]"
    if family in B.FINITE:
        assert (ids == B.ids_of(want["L"])).all(), f"{what}: sphere_ids"


@pytest.mark.parametrize("case", BUILD_CASES, ids=_id)
def test_large_class_build_equals_oracle(R, ctx, case):
    family, n = case
    s, view = B.scene(family, n), _view(family)
    try:
        for gpu_build in (1, 0) if n <= HOST_BUILDER_MAX_N else (1,):
            ctx.set_option("gpu_build", gpu_build)
            sc = ctx.scene_from_spheres(s, *view)
            ps = R.prepare_scene(48, 64, sc)
            sc.free()
            try:
                _same_build(ps, family, n, f"{family}:{n} prepare_scene gpu_build={gpu_build}")
            finally:
                ps.free()
            ps = R.prepare_scene_from_spheres(ctx, s, 48, 64, *view)
            try:
                _same_build(ps, family, n, f"{family}:{n} prepare_scene_from_spheres gpu_build={gpu_build}")
            finally:
                ps.free()
    finally:
        _restore(R, ctx)


def _hit_fraction(orc, h, w):
    idx, _ = orc.objs_hit_rays(B.primary_rays(orc.camera_floats(h, w), h, w), 0.0, 1e9)
    return float(np.mean(idx >= 0))


@pytest.mark.parametrize("case", FRAME_CASES, ids=_id)
def test_frames_through_the_traversal_copy(R, ctx, case):
    """One small frame in each kernel family (the pooled one three times: the first frame records the view, the second orders the record,
    then the policy), bit for bit the oracle's render: the treelet numbering and the depth sort of trees up to 47 levels."""
    family, n = case
    orc, _, _ = _expect(family, n)
    h, w = B.frame_of(family)
    want, _ = orc.render(h, w)
    assert _hit_fraction(orc, h, w) >= 0.05
    ps = R.prepare_scene_from_spheres(ctx, B.scene(family, n), h, w, *_view(family))
    try:
        for variant in (R.VARIANT_PIXEL, R.VARIANT_PERSISTENT, R.VARIANT_POOLED):
            ctx.set_variant(variant)
            for frame in range(3 if variant == R.VARIANT_POOLED else 1):
                bad = int((R.render(h, w, ps) != want).sum())
                assert bad == 0, f"{family}:{n} variant {variant} frame {frame} ({ctx.last_launch}): {bad} pixels differ from the oracle"
    finally:
        _restore(R, ctx)
        ps.free()


@pytest.mark.parametrize("family", B.HUGE_FAMILIES)
def test_rays_through_513_sort_tiles(R, ctx, family):
    """524 289 spheres: the camera's primary rays through intersect_rays against the oracle's objs_hit (the build itself is compared in
    test_large_class_build_equals_oracle)."""
    n = B.HUGE
    orc, _, _ = _expect(family, n)
    h, w = B.rays_of(family, n)
    ps = R.prepare_scene_from_spheres(ctx, B.scene(family, n), h, w, *_view(family))
    try:
        rays = R.camera_rays(ps, h, w)
        assert rays.shape == (h * w, 6)
        want_idx, want_hit = orc.objs_hit_rays(rays, 0.0, 1e9)
        assert np.mean(want_idx >= 0) >= 0.05
        idx, hit = R.intersect_rays(ps, rays)
        ER.same_bits(idx, want_idx, f"{family}:{n} index")
        rows = want_idx >= 0
        ER.same_bits(hit[rows], want_hit[rows], f"{family}:{n} hit")
    finally:
        ps.free()


def _points(L, m, seed):
    """m points: a quarter at sphere centres (half of those at centres of distinct keys: the chain, not the duplicates), a quarter on
    surfaces, the rest anywhere in and around the lattice's box"""
    rng = np.random.default_rng(seed)
    n, q = L.shape[0], m // 4
    p = rng.uniform(-8.0, 1031.0, (m, 3)).astype(F)
    _, first = np.unique(L[:, :3], axis=0, return_index=True)
    j = np.concatenate([rng.choice(first, q // 2), rng.integers(0, n, q - q // 2)])
    p[:q] = L[j, :3]
    d = rng.normal(size=(q, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    j2 = np.concatenate([rng.choice(first, q // 2), rng.integers(0, n, q - q // 2)])
    p[q:2 * q] = (L[j2, :3] + d * L[j2, 6:7]).astype(F)
    return p


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


@pytest.mark.parametrize("case", CONSUMER_CASES, ids=_id)
def test_consumers_of_the_sweep_count(R, ctx, case):
    """Trees whose height exceeds floor(log2 n) + 2: the boxes of the top levels have not converged, so the proximity and range queries may
    prune only below exact_depth = height - sweeps, and no launch may be culled.  256 points against proximity_ref / within_ref, bit for bit."""
    family, n = case
    orc, a, height = _expect(family, n)
    assert height > B.sweeps_of(n)
    h, w = B.frame_of(family)
    want_img, _ = orc.render(h, w)
    p = _points(a["L"], 256, n)
    ps = R.prepare_scene_from_spheres(ctx, B.scene(family, n), h, w, *_view(family))
    try:
        assert ps.bvh_arrays()["L"].tobytes() == a["L"].tobytes()
        want = P.nearest(a["L"], p, 1e9, 8, chunk=32)
        for count in (True, False):
            got = R.nearest_spheres(ps, p, 8, count=count)
            for name, g, wv in zip(("count", "index", "gap"), got, want):
                if name == "count" and not count:
                    assert g is None
                    continue
                bad = np.nonzero((_bits(g) != _bits(wv)).reshape(len(p), -1).any(axis=1))[0]
                assert bad.size == 0, f"{family}:{n} nearest count={count}: {name} differs on {bad.size} points, first {bad[:5]}"
        got = R.spheres_within(ps, p, 1.5)
        for name, g, wv in zip(("offsets", "index", "gap"), got, W.within(a["L"], p, 1.5)):
            assert g.shape == wv.shape and (_bits(g) == _bits(wv)).all(), f"{family}:{n} within: {name} differs"
        # a pooled frame with culling forced wherever the guards pass: the height guard must not
        ctx.set_variant(R.VARIANT_POOLED)
        ctx.set_option("cull", 1)
        for shape in (L2_16, {}):
            for k, v in shape.items():
                ctx.set_option(k, v)
            for frame in range(2):
                got_img = R.render(h, w, ps)
                ll = ctx.last_launch
                assert "+CULL" not in ll, (family, n, shape, frame, ll)
                assert int((got_img != want_img).sum()) == 0, (family, n, shape, frame, ll)
            for k in shape:
                ctx.set_option(k, DEFAULTS[k])
    finally:
        _restore(R, ctx)
        ps.free()


def test_flat_tree_of_equal_keys_is_culled(R, ctx):
    """`same` at 32 768 spheres: height 15 <= 17 sweeps, so the height guard admits what it refuses on the tall families -- +CULL appears
    wherever edge_cull's float64 restatement of the other guards admits the scene and the camera."""
    family, n = "same", 32768
    orc, a, height = _expect(family, n)
    assert height <= B.sweeps_of(n)
    s = B.scene(family, n)
    h, w = B.frame_of(family)
    g = EC.guards(s, height)
    expect = g["ok"] and EC.origin_ok(g, orc.camera_floats(h, w)[0:3])
    assert expect, "the scene was placed inside every guard"
    want, _ = orc.render(h, w)
    ps = R.prepare_scene_from_spheres(ctx, s, h, w, *_view(family))
    try:
        assert ps.height == height
        ctx.set_variant(R.VARIANT_POOLED)
        ctx.set_option("cull", 1)
        for k, v in L2_16.items():
            ctx.set_option(k, v)
        for frame in range(2):
            got = R.render(h, w, ps)
            ll = ctx.last_launch
            assert "waves=16" in ll and "+CULL" in ll, (frame, ll)
            assert int((got != want).sum()) == 0, (frame, ll)
    finally:
        _restore(R, ctx)
        ps.free()


@pytest.mark.parametrize("n", (24577, 131073))
def test_update_from_a_tall_tree_and_back(R, ctx, n):
    """A prepared `forest` (height 33 / 36) rebuilt in place as `few` (16 / 19) and as `forest` again: the arrays, the height and a frame
    of a fresh prepare -- no box, depth or `fin` value of the taller tree is left behind in the buffers the rebuild reuses."""
    view = _view("forest")
    h, w = B.frame_of("forest")
    ps = R.prepare_scene_from_spheres(ctx, B.scene("forest", n), h, w, *view)
    try:
        R.render(h, w, ps)
        for family in ("few", "forest"):
            ps.update_spheres(B.scene(family, n))
            _same_build(ps, family, n, f"forest -> {family}:{n} updated")
            fresh = R.prepare_scene_from_spheres(ctx, B.scene(family, n), h, w, *view)
            try:
                assert fresh.height == ps.height
                for variant in (R.VARIANT_POOLED, R.VARIANT_PIXEL):
                    ctx.set_variant(variant)
                    want = R.render(h, w, fresh)
                    want_ll = ctx.last_launch
                    got = R.render(h, w, ps)
                    assert ctx.last_launch == want_ll, (family, n, variant, ctx.last_launch, want_ll)
                    assert int((got != want).sum()) == 0, (family, n, variant, want_ll)
            finally:
                fresh.free()
    finally:
        _restore(R, ctx)
        ps.free()
